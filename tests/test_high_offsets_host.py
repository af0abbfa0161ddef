"""The case table of tests/test_high_offsets_gpu.py, checked on the CPU: every case is a plan y3_net_plan_hw accepts, puts what it says
above 2 GiB, looks at the images that matter, fits the memory budget -- and together the cases reach every (family, operand role) pair and
every tile id of tests/high_offset_cases.py."""
import pytest

from tests import high_offset_cases as hc

IDS = [c.name for c in hc.CASES]


@pytest.mark.parametrize("case", hc.CASES, ids=IDS)
def test_plan_is_accepted_and_fits_the_budget(case):
    sizes = {t: hc.tensor_bytes(case, t) for t in hc.plan_tensors(case)}
    assert max(sizes.values()) < hc.GUARD, sizes                      # 1. the plan is accepted (fp32 grids counted at 4 bytes)
    assert hc.total_bytes(case) < hc.BUDGET, hc.total_bytes(case)     # 5. a condition, not a measurement
    assert all(t is not None for t in hc.forcing(case).values()), hc.forcing(case)      # no launch left to a heuristic
    assert case.canvas[0] % 2 == 0 and case.canvas[1] % 2 == 0


@pytest.mark.parametrize("case", hc.CASES, ids=IDS)
def test_high_tensors_and_checked_images(case):
    high = hc.high_tensors(case)
    assert high and hc.roles(case), "the case puts nothing above 2 GiB"
    imgs = hc.checked_images(case)
    assert 0 in imgs and case.batch - 1 in imgs and len(imgs) <= 6
    for t, (b0, nb) in high.items():
        assert hc.tensor_bytes(case, t, nb) > hc.HIGH                                          # 2.
        s, per = hc.straddle_image(case, t), hc.image_bytes(case, t)
        assert s in imgs and (s - b0) * per <= hc.HIGH < (s - b0 + 1) * per and s < b0 + nb    # 3. its bytes hold offset 2^31 of the launch's view
        if case.mode == "i8" and hc.elem_bytes(case, t) == 1:
            assert hc.tensor_bytes(case, t, nb) // hc.elem_bytes(case, t) > hc.HIGH            # 4. more than 2^31 ELEMENTS: the index itself passes int
    if case.mode == "i8":
        p, _ = case.program()
        assert any(hc.elem_bytes(case, t) == 1 for t in high), "an int8 case needs an int8 tensor of more than 2^31 elements"
    if case.lanes > 1:
        b0, nb = hc.lane_ranges(case)[-1]
        assert b0 > 0 and all(v == (b0, nb) for v in high.values())
        assert all(hc.tensor_bytes(case, t, hc.lane_ranges(case)[0][1]) <= hc.HIGH for t in high), "the last lane ALONE is high"
        # a lane's region of an arena block starts where the lane before it ends, rounded up to 256 bytes (y3_lane_offset): with every
        # lane's bytes a multiple of 256 there is no gap, each region starts at its first image, and read_tensor sees the batch in order
        from yolo_v3_tf2_amd import _lib
        p, _ = case.program()
        arena = [t for t in hc.plan_tensors(case) if t != p.input_tensor and t not in p.outputs]
        assert all(b0 * hc.image_bytes(case, t) % 256 == 0 for t in arena)
        for t in arena:
            per = hc.image_bytes(case, t)
            offs = [_lib.load().y3_lane_offset(case.batch * per, case.batch, case.lanes, l) for l in range(case.lanes)]
            assert offs == [s * per for s, _ in hc.lane_ranges(case)], (case.name, t, offs)
    if case.border_skip:
        assert all(nb % 32 == 0 and nb >= 32 for _, nb in hc.lane_ranges(case))
    if case.near_guard:
        _, ops = case.program()
        src = ops[case.near_guard]
        assert src.size == 3 and src.stride == 1
        assert hc.GUARD - hc.image_bytes(case, src.src0) <= hc.tensor_bytes(case, src.src0) < hc.GUARD


def test_coverage_is_complete():
    pairs, tiles = hc.coverage()
    want_pairs = {(fam, role) for fam, rs in hc.FAMILY_ROLES.items() for role in rs}
    want_tiles = {(fam, t) for fam, (_, ts) in hc.FAMILY_TILES.items() for t in ts}
    assert all(role in hc.ROLES for _, role in want_pairs)
    assert not want_pairs - pairs, sorted(want_pairs - pairs)
    assert not want_tiles - tiles, sorted(want_tiles - tiles)
    assert sorted(hc.FAMILY_ROLES) == sorted(hc.FAMILY_TILES)


def test_every_operand_role_is_high_somewhere():
    pairs, _ = hc.coverage()
    assert {role for _, role in pairs} == set(hc.ROLES)


@pytest.mark.parametrize("case", hc.CASES, ids=IDS)
def test_forced_tiles_are_built_and_fit_by_the_library_s_rule(case):
    """A tile the library has not built, or that does not fit, is not an error at launch: family_tile falls back to the heuristic silently.
    So what forcing() picks is held to the library's own answers here -- y3_tile_built for the plan's format (for int8 the int8 form: the
    setter an int8 plan shares with bf16 validates against the bf16 table) and y3::tile_fits restated on the family's own padding and K
    step -- and the GPU test's setter call refuses the rest."""
    from yolo_v3_tf2_amd import _lib
    m = hc.MODES[case.mode]
    p, _ = case.program()
    for slot, o in enumerate(p.conv_ops()):
        t = hc.forcing(case)[slot]
        if t == hc.FIRST:
            assert o.cin == 3 and slot == 0
            continue
        assert _lib.tile_built(m["dtype"], t), (case.name, slot, t)
        if t == m["resident"]:
            continue
        bm, bn, _, bk = m["table"][t][:4]
        bk = m["bk"] or bk
        cout_pad = -(-o.cout // m["pad"]) * m["pad"]
        assert o.cin % bk == 0 and cout_pad % bn == 0 and (o.src1 < 0 or o.c0 % bk == 0), (case.name, slot, t)
        if case.mode == "i8":
            assert t in _lib.TILES_I8_BUILT and bk == 128 and m["pad"] == 64


def test_conv_first_source_cannot_be_high():
    """conv_first reads [B,H,W,3] fp32 and writes [B,H,W,32] in 2, 4 or 6 bytes an element: the source is at most 12 / 64 of a destination
    the guard accepts."""
    for eb in (2, 4, 6):
        assert (hc.GUARD - 1) * 12 // (32 * eb) < hc.HIGH


@pytest.mark.parametrize("family", sorted(hc.STEM_FAMILIES))
def test_a_fused_stem_has_no_operand_above_2_gib(family):
    """Why the table has no case for conv_stem_f32 and conv_stem16: the plan sizes conv0's destination [B,H,W,32] (the fused kernel keeps it
    on chip, the guard counts it all the same) and refuses it at 0xFFFFFFF0 bytes.  Per image of an H x W canvas, both % 32 == 0, in eb
    bytes an element: conv0's destination 32 H W eb; the stem's first destination (conv1, [H/2,W/2,64]) 16 H W eb, half; its second (the
    1x1, [H/2,W/2,32]) 8 H W eb; its source (the fp32 image) 12 H W.  So at the largest batch the guard accepts, on any canvas, the
    largest of them is below 2^31 bytes."""
    eb = hc.STEM_FAMILIES[family]
    for H, W in ((32, 32), (32, 64), (96, 64), (416, 416), (608, 608)):
        conv0 = 32 * H * W * eb
        B = (hc.GUARD - 1) // conv0                      # the largest batch y3_net_plan_hw accepts
        assert B >= 1 and (B + 1) * conv0 >= hc.GUARD
        dst, dst2, img = (H // 2) * (W // 2) * 64 * eb, (H // 2) * (W // 2) * 32 * eb, H * W * 3 * 4
        assert 2 * dst == conv0 and 4 * dst2 == conv0 and img * 2 < conv0
        assert max(B * dst, B * dst2, B * img) < hc.HIGH


def test_near_guard_cases_cover_every_element_size():
    sizes = set()
    for c in hc.CASES:
        if c.near_guard:
            _, ops = c.program()
            sizes.add(hc.elem_bytes(c, ops[c.near_guard].src0))
    assert sizes == {4, 2, 1}


def test_lanes_are_covered_in_fp32_and_16_bit():
    assert {c.mode for c in hc.CASES if c.lanes == 2} == {"f32", "bf16"}


def test_the_body_program_takes_every_launch_form():
    """What tests/helpers.tile_feature_program guarantees its suites, for body_program."""
    p, ops = hc.body_program(64, 128, 64, 64, 128)
    assert (ops["a"].size, ops["a"].residual, ops["a"].leaky) == (3, -1, True)
    assert ops["c"].residual == ops["a"].dst and not ops["c"].leaky
    assert ops["d"].stride == 2 and ops["f"].src0_upsample and ops["f"].src1 == ops["e"].dst and ops["f"].c0 == 64
    assert ops["h0"].cout == 127 and not ops["h0"].bn and p.outputs == [ops["h0"].dst, ops["h1"].dst, ops["h2"].dst]
    assert {p.tensors[t].div for t in p.outputs} == {2}
    p, ops = hc.body_program(64, 64, 64, 64, 64, out_c=True)
    assert p.outputs[2] == ops["c"].dst and hc.staged_outputs(p) == {ops["c"].dst}
