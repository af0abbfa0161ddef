"""The footprint suite's basis, on the CPU (tests/footprint_cases.py; the device side is tests/test_footprint_gpu.py).

1. y3_lane_offset -- the function Slice::ptr evaluates for every launch address of a multi-lane forward, exported pure like
   y3_persistent_grid -- swept over per-image sizes (every multiple of 16 up to 8192 and the shipped networks' own in all six modes),
   max_batch 1..8, batch 1..max_batch, lanes 1..4 and two block sizes: offsets 256-aligned, regions disjoint, the last one inside the
   block's slack, and the addresses of the shipped networks unchanged.  The rule it replaced fails the same sweep
   (test_the_old_rule_fails_the_sweep): the sweep is the proof that lanes cannot overlap; the device test of it is a race.
2. The case table of the guarded calls: every call and mode has a case, every conv-network case has a launch with ragged rows and one
   with a ragged width, every guard meets its size condition."""
import re

import pytest

from tests import footprint_cases as F
from yolo_v3_tf2_amd import _lib


def _offset(block_bytes, batch, lanes, lane):
    return int(_lib.load().y3_lane_offset(block_bytes, batch, lanes, lane))


# ---------------------------------------------------------------------------------------------- 1. lane regions
def test_lane_offset_is_declared_bound_and_exported():
    import os
    header = open(os.path.join(F.ROOT, "include", "y3.h")).read()
    assert "y3_lane_offset" in _lib.SYMBOLS and re.search(r"\blong long y3_lane_offset\s*\(", header)
    assert hasattr(_lib.load(), "y3_lane_offset")
    src = open(os.path.join(F.ROOT, "yolo-v3-tf2_amd", "csrc", "y3_forward.cpp")).read()
    ptr = src[src.index("void *ptr(int t) const"):src.index("y3::ConvArgs conv_args")]
    assert "y3_lane_offset(" in ptr and "+ 255" not in ptr, "Slice::ptr must take its lane regions from y3_lane_offset"


def test_lane_offset_refuses_what_no_forward_has():
    for args in ((-1, 4, 2, 0), (1024, 0, 1, 0), (1024, 4, 0, 0), (1024, 4, 5, 0), (1024, 8, 5, 4), (1024, 4, 2, -1), (1024, 4, 2, 2),
                 (1024, 2, 3, 0), (1024, 1, 2, 1)):
        assert _offset(*args) == -1, args
    assert [_offset(0, 4, 4, l) for l in range(4)] == [0, 0, 0, 0]
    assert _offset(0xFFFFFFF0 + 4096, 8, 4, 3) == ((0xFFFFFFF0 + 4096) * 6 // 8 + 255) // 256 * 256      # no 32-bit arithmetic inside


def test_the_issue_s_two_cases():
    """3200-byte images (5 x 5 pixels x 32 channels x fp32), batch 4 on four lanes: the old offsets [0, 3328, 6400, 9728] let lane 1's
    [3328, 6528) run 128 bytes into lane 2.  192-byte images, batch 6 on four lanes: [0, 256, 768, 768], two lanes on one start."""
    assert [F.old_lane_offset(12800, 4, 4, l) for l in range(4)] == [0, 3328, 6400, 9728]
    assert [F.old_lane_offset(1152, 6, 4, l) for l in range(4)] == [0, 256, 768, 768]
    assert [_offset(12800, 4, 4, l) for l in range(4)] == [0, 3328, 6656, 9984]
    assert [_offset(1152, 6, 4, l) for l in range(4)] == [0, 256, 768, 1024]
    assert F.check_lane_regions(F.old_lane_offset, 3200, 4, 4, 4, 12800) and F.check_lane_regions(F.old_lane_offset, 192, 6, 6, 4, 1152)


def test_lane_regions_sweep():
    """(a) 256-aligned, (b) nested for any tensor sharing the block, (c) inside block + 4096, (d) equal to block * start / batch wherever
    that is a multiple of 256 for every lane -- footprint_cases.check_lane_regions states each."""
    n, bad = F.lane_sweep(_offset)
    print(f"lane sweep: {n} combinations over {len(F.sweep_sizes())} per-image sizes, {len(bad)} violations")
    assert n > 100000 and not bad, (len(bad), bad[:5])


def test_the_old_rule_fails_the_sweep():
    """The rule before y3_lane_offset, restated (footprint_cases.old_lane_offset): the same conditions find its overlaps, and find none at
    the shipped networks' sizes on a full batch -- why no network test ever saw one."""
    n, bad = F.lane_sweep(F.old_lane_offset, sizes=range(16, 8192 + 1, 16))
    print(f"lane sweep of the old rule: {len(bad)} of {n} combinations violate a condition; the first: {bad[0] if bad else None}")
    assert len(bad) > 1000 and all(b.startswith(("(b", "(c")) for b in bad)
    for ib in F.shipped_image_bytes():
        if ib % 256:
            continue
        for max_batch in range(1, 9):
            for lanes in range(1, F.MAX_LANES + 1):
                assert F.check_lane_regions(F.old_lane_offset, ib, max_batch, max_batch, lanes, max_batch * ib) is None
                if lanes <= max_batch:      # and there the two rules agree: the shipped plans launch with the addresses they had
                    assert [_offset(max_batch * ib, max_batch, lanes, l) for l in range(lanes)] == \
                           [F.old_lane_offset(max_batch * ib, max_batch, lanes, l) for l in range(lanes)]


def test_the_lane_chain_reaches_unaligned_regions():
    """What the device test relies on: in each of its three modes the chain stores a tensor whose per-image bytes are no multiple of 256
    -- 3200 among them -- so that with three and four lanes the old rule's regions overlap for a tensor of the plan itself."""
    progs = F.lane_chain_program()
    want = {"f32": {3200, 9600}, "bf16": {3200, 6400}, "i8": {3200, 6400}}
    for mode, p in progs.items():
        sizes = F.stored_image_bytes(p, mode, F.LANE_CHAIN_CANVAS)
        assert set(sizes.values()) == want[mode], (mode, sizes)
        assert 3200 in sizes.values() and 3200 % 256
        for B in F.LANE_CHAIN_BATCHES:
            for batch in (B, B - 1):
                hit = [F.check_lane_regions(F.old_lane_offset, ib, B, batch, lanes, B * ib) for ib in sizes.values() for lanes in (3, 4)]
                assert any(hit) or batch < B, (mode, B, batch)      # a full batch on an exact block is where the old regions collide
                assert all(F.check_lane_regions(_offset, ib, B, batch, lanes, B * ib) is None for ib in sizes.values() for lanes in (3, 4))
    from yolo_v3_tf2_amd import quant
    p = progs["i8"]
    cut = quant.first_i8_conv(p)
    behind = [o for o in p.conv_ops()[cut:] if o.dst not in p.outputs]
    assert behind and any(o.cout == 128 for o in behind), "a 128-channel int8 tensor behind the cut"


# ---------------------------------------------------------------------------------------------- 2. the guarded calls
IDS = [c.name for c in F.CASES]


def test_every_call_and_mode_has_a_case():
    have = {(c.call, c.net, c.mode) for c in F.CASES}
    assert not set(F.REQUIRED) - have, sorted(set(F.REQUIRED) - have)
    assert {c.mode for c in F.CASES if c.net == "yolov3_nc80" and c.call == "y3_net_forward"} == set(F.MODES)
    assert {c.canvas for c in F.CASES if c.net == "yolov3_nc80" and c.call == "y3_net_forward"} == {96, F.RECT}
    assert all(set(c.batches) == {3, 4} and set(c.lanes) == {1, 2} and c.max_batch == 4
               for c in F.CASES if c.net == "yolov3_nc80" and c.call == "y3_net_forward")
    # a 16-bit plan of YOLOv3-tiny exists with the fused stem only (y3_net_set_tiny_stem_fusion): off is an fp32 case
    assert {(c.mode, dict(c.opts)["tiny_stem"]) for c in F.CASES if c.net == "tiny_nc80"} == {("f32", 0), ("f32", 1), ("bf16", 1), ("f16", 1)}
    from tests.class_count_cases import head_route
    assert head_route(F.NC_BELOW) == "composed" and head_route(F.NC_INSIDE) == "fused" and F.NC_INSIDE != 80
    for call in ("y3_net_detect", "y3_net_detect_grids"):
        opts = [dict(c.opts) for c in F.CASES if c.call == call]
        assert {o["per_class"] for o in opts} == {0, 1} and sum(o.get("multi_label", 0) for o in opts) == 1
    assert all(set(c.lanes) == {1, 2} for c in F.CASES if c.call == "y3_net_forward_decode")
    assert len(IDS) == len(set(IDS))


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_case_has_ragged_rows_and_a_ragged_width(case):
    """At least one launch with M % 64 != 0 (a partly filled tile of every height: the BM of every table is a multiple of 64) and at least
    one whose Cout is no multiple of its tile's width, at every batch the case runs."""
    for batch in case.batches:
        ls = F.launches(case, batch)
        assert any(M % 64 for _, M, _, _ in ls), (case.name, batch)
        if case.net == "unfolded":
            # unfolded_program is in the table for the stores of the stand-alone add / up-sample / concat kernels, which have no tile; all
            # of its conv widths are 32 or 64 and no tile of a ragged width fits them.  The ragged width of a raw-feature program is
            # tile_feature_program's head 0 (63 channels), in the table beside it.
            assert all(cout % 32 == 0 and cout % bn == 0 for _, _, cout, bn in ls)
            assert any(c.net == "tile64" and c.mode == case.mode for c in F.CASES)
            continue
        assert any(bn and cout % bn for _, _, cout, bn in ls), (case.name, batch, ls)
    assert all(t[0] % 64 == 0 for tab in (_lib.TILES, _lib.TILES_BF16, _lib.TILES_X3) for t in tab)
    if case.call == "y3_net_forward_decode":
        assert min(M for _, M, _, _ in F.launches(case, 3)) == 27       # the coarsest head: 27 pixels in a 64-pixel tile


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_guards_meet_the_size_condition(case):
    widest = max(t[1] for tab in (_lib.TILES, _lib.TILES_BF16, _lib.TILES_X3) for t in tab)
    tallest = max(t[0] for tab in (_lib.TILES, _lib.TILES_BF16, _lib.TILES_X3) for t in tab)
    assert tallest <= F.GUARD_ROWS and widest <= 256
    for what, shape, dtype in F.guarded_outputs(case):
        itemsize = {"float32": 4, "int32": 4, "int64": 8}[dtype]
        g = F.guard_bytes(shape, itemsize)
        row = F.row_elems(shape) * itemsize
        assert g >= 64 * 1024 and g >= 256 * row and g % 256 == 0, (case.name, what, g)
        if what.startswith("grid"):
            assert row == shape[-1] * (3 if len(shape) == 5 else 1) * 4
            # a row mask missing on the tallest tile writes fewer than 256 rows past the end; a column mask missing on the widest
            # fewer than 256 columns past a row's end, which is less than one more row of these grids or inside the 64 KiB
            assert g >= tallest * row and g >= widest * 4


def test_stand_alone_op_guards():
    for shape, stride in F.POOL_CASES:
        for itemsize in (4, 2):
            out = (shape[0], shape[1] // stride, shape[2] // stride, shape[3])
            assert F.guard_bytes(out, itemsize) >= max(65536, 256 * shape[3] * itemsize)
            assert shape[3] * itemsize % 16 == 0
    assert ((2, 4, 4, 8), 1) in F.POOL_CASES and 8 * 2 == 16         # 16-bit: one 16-byte vector per pixel
    assert F.row_elems((3, 100, 4)) == 4 and F.row_elems((3, 100)) == 1 and F.row_elems((3,)) == 1 and F.row_elems((3, 2, 2, 3, 85)) == 255


def test_poison_word():
    import numpy as np
    w = np.array([F.POISON], np.uint32)
    assert np.isnan(w.view(np.float32)[0]) and (F.POISON >> 22) & 1, "a quiet NaN as fp32"
    assert w.view(np.int32)[0] > 4096 and w.view(np.uint8).tolist() == [0xA5, 0xA5, 0xC5, 0x7F]
