"""Conv epilogues at trained-like batch-norm statistics, judged per channel, on the GPU (tests/bn_stat_cases.py states the recipe and
the bars; tests/test_bn_stats_host.py holds both to the reference alone).

Every launch is teacher-forced: restated by the oracle (helpers.oracle_launch, double accumulation) from the launch's OWN input tensors on
the device, and held with check_per_channel -- an fp32 output within 2e-5 of m_c in every channel c, a stored bf16 / fp16 output within
its own ulp + 1e-5 m_c of the rounded reference with at most 2e-3 / 1e-2 of the launch's elements different at all.  The fused stems,
which keep conv0 (and in fp32 plans conv1) on chip, are judged the way their existing tests judge them, with the bound per channel.
Every test asserts that what it forces took: the tile (its setter's acceptance), split_k(slot), the stem's launch structure."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import bn_stat_cases as C  # noqa: E402
from tests.class_count_cases import head_route  # noqa: E402
from tests.f16_oracle import round_f16  # noqa: E402
from tests.test_tile_matrix_gpu import MODES, MUST_FORCE  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

DTYPES = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16, "f32x3": _lib.Y3_DTYPE_F32X3,
          "f32x2": _lib.Y3_DTYPE_F32X2}
SIXTEEN = ("bf16", "f16")
TILE_MODES = {**{m: (spec[1], spec[2], spec[3], spec[4]) for m, spec in MODES.items()},
              "f16": (_lib.TILES_BF16, MODES["bf16"][2], "set_tile_bf16", 3)}        # fp16 plans share the bf16 table, ids and setter
TILE_CASES = [(mode, t) for mode, spec in TILE_MODES.items() for t in spec[1]]


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def _ref_mode(mode):
    """The reference a plan mode is held to: fp32, f32x3 and f32x2 plans compute the fp32 function."""
    return mode if mode in SIXTEEN else "f32"


def _host_input(x, mode):
    """The input as the plan sees it, in fp32: rounded to the 16-bit format where it feeds an MFMA conv directly."""
    from oracle import oracle as O
    if mode in SIXTEEN and x.shape[-1] != 3:
        return round_f16(x) if mode == "f16" else O.round_bf16(x)
    return np.ascontiguousarray(x, np.float32)


def _feed(rt, mode, x):
    """The device input of a plan of `mode` (x as _host_input returns it)."""
    if x.shape[-1] == 3 or mode == "f32":
        return _cuda(x)
    if mode in SIXTEEN:
        return _cuda(x).to(torch.bfloat16 if mode == "bf16" else torch.float16)
    return rt.split3_planes(_cuda(x)) if mode == "f32x3" else rt.split2_planes(_cuda(x))


def _tensors(net, p, x, grids, B):
    """tensor id -> fp32 NHWC of the device's own tensors (the plan keeps its activations), read once."""
    cache = {p.input_tensor: x}
    cache.update({t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(p.outputs, grids)})

    def dev(t):
        if t not in cache:
            cache[t] = net.read_tensor(t, B).cpu().numpy()
        return cache[t]
    return dev


def _judge(p, w, mode, dev, ops=None, tag=""):
    """Every launch in `ops` (default: all of the program) against the oracle on the launch's own device inputs, per channel.
    -> (worst share of a bar, worst differing fraction of a stored launch)."""
    from oracle import oracle as O
    rm = _ref_mode(mode)
    worst, worst_frac = 0.0, 0.0
    with C.mode_oracle(rm):
        for o in (p.conv_ops() if ops is None else ops):
            ref = C.launch_reference(O, o, w, dev, rm)
            m = C.channel_magnitude(O, o, C.mode_weights(w, o, rm), dev)
            stored = rm if rm in SIXTEEN and o.dst not in p.outputs else None
            bar = C.F32_CHANNEL_BAR_OVERRIDES.get((tag, o.conv_index), C.F32_CHANNEL_BAR)
            share, frac = C.check_per_channel(dev(o.dst), ref, m, (tag, mode, f"conv{o.conv_index}"), stored=stored, bar=bar)
            assert float(np.abs(ref).max()) > 0.5      # not a comparison of two empty buffers
            worst, worst_frac = max(worst, share), max(worst_frac, frac)
    return worst, worst_frac


def _run(rt, p, w, x, mode, B, canvas, setup=None):
    """A net of p planned in `mode` with its activations kept, one forward: -> (net, dev accessor, grids)."""
    net = rt.Net(p)
    net.load_weights(w)
    if setup:
        setup(net)
    net.keep_activations(True)
    net.plan(B, canvas, DTYPES[mode])
    xh = _host_input(x, mode)
    grids = [g.clone() for g in net.forward(_feed(rt, mode, xh))]
    torch.cuda.synchronize()
    return net, _tensors(net, p, xh, grids, B), grids


# ---------------------------------------------------------------------------------------------- a. generic tiles
@pytest.mark.parametrize("mode,tile", TILE_CASES, ids=[f"{m}-t{t}" for m, t in TILE_CASES])
def test_every_tile_per_channel(rt, mode, tile):
    table, _, setter, bk_col = TILE_MODES[mode]
    bn, bk = table[tile][1], (table[tile][bk_col] if bk_col is not None else 32)
    p, ops, w, x = C.tile_case(bn, bk)
    forced = []

    def force(net):
        for slot, o in enumerate(net.conv_ops):
            try:
                getattr(net, setter)(slot, tile)
            except rt.Y3Error as e:
                if "tile does not" not in str(e):
                    raise
                continue
            forced.append(o)

    net, dev, _ = _run(rt, p, w, x, mode, C.TILE_BATCH, C.TILE_CANVAS, force)
    missed = [k for k in MUST_FORCE if not any(o is ops[k] for o in forced)]
    assert not missed, f"tile {tile} was refused on conv(s) {missed}"
    worst, frac = _judge(p, w, mode, dev, tag=f"tile-bn{bn}-bk{bk}")
    print(f"bn-stats {mode} tile {tile}: forced {len(forced)} convs, worst {worst:.3f} of the per-channel bar, worst differing fraction {frac:.2e}")


# ---------------------------------------------------------------------------------------------- b. weight-resident kernels
RESIDENT_CASES = [("f32", 32, *c) for c in C.RESIDENT_F32] + [(m, *c) for m in SIXTEEN for c in C.RESIDENT_16]


@pytest.mark.parametrize("mode,cin,cout,S,B", RESIDENT_CASES)
def test_weight_resident_kernels_per_channel(rt, mode, cin, cout, S, B):
    """fp32 tile 33 / tile 32 of the 16-bit plans on every 3x3 conv of the program: per channel against the oracle, and every tensor bit
    for bit the generic tile's of the same MFMA shape."""
    p, w, x = C.resident_case(cin, cout, S, B)
    setter = "set_tile" if mode == "f32" else "set_tile_bf16"
    resident, generic = (33, 11) if mode == "f32" else (32, 5 if cin == 32 else 10)
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    got = {}
    for tile in (resident, generic):
        n3 = []

        def force(net):
            for slot, o in enumerate(net.conv_ops):
                if o.size == 3:
                    getattr(net, setter)(slot, tile)
                    n3.append(slot)
        net, dev, grids = _run(rt, p, w, x, mode, B, S, force)
        assert len(n3) == 3
        got[tile] = grids + [net.read_tensor(t, B).clone() for t in stored]
        if tile == resident:
            worst, frac = _judge(p, w, mode, dev, tag=f"resident-{cin}-{cout}-{S}x{B}")
    assert all(torch.equal(a, b) for a, b in zip(got[resident], got[generic])), "the weight-resident kernel differs from the generic tile"
    print(f"bn-stats {mode} weight-resident {cin}->{cout} @{S} x{B}: worst {worst:.3f} of the per-channel bar, worst differing fraction {frac:.2e}")


# ---------------------------------------------------------------------------------------------- c. split-K finish kernels
SPLIT_CASES = [("f32", *c) for c in C.SPLITK_F32] + [(m, *c) for m in SIXTEEN for c in C.SPLITK_16]


@pytest.mark.parametrize("mode,name,S,tile", SPLIT_CASES)
def test_split_k_finish_per_channel(rt, mode, name, S, tile):
    p, w, x, B, size, slots = C.splitk_case(mode != "f32", name)
    sfx = {"f32": "", "bf16": "_bf16", "f16": "_f16"}[mode]

    def force(net):
        for slot in slots:
            getattr(net, "set_tile" if mode == "f32" else "set_tile_bf16")(slot, tile)
            getattr(net, "set_split_k" + sfx)(slot, S)
    net, dev, _ = _run(rt, p, w, x, mode, B, size, force)
    assert [getattr(net, "split_k" + sfx)(i) for i in range(len(net.conv_ops))] == [S if i in slots else 1 for i in range(len(net.conv_ops))]
    split_ops = [net.conv_ops[i] for i in slots]
    worst, frac = _judge(p, w, mode, dev, ops=split_ops, tag=f"splitk-{'f32' if mode == 'f32' else '16'}-{name}")
    print(f"bn-stats {mode} split-K {name} S={S} tile {tile}: worst {worst:.3f} of the per-channel bar, worst differing fraction {frac:.2e}")


# ---------------------------------------------------------------------------------------------- d. stems
def _stem_switch(net, mode, on):
    (net.set_stem_fusion_f16 if mode == "f16" else net.set_stem_fusion)(on)


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16", "f32x3", "f32x2"])
@pytest.mark.parametrize("S,B", C.STEM_SIZES)
def test_first_layer_alone_per_channel(rt, S, B, mode):
    """conv_first on its own (a plan that keeps its activations launches every conv by itself), in every format it stores (fp32, bf16,
    fp16, three bf16 planes, two fp16 planes), and the convs behind it, teacher-forced."""
    p, w, x = C.stem_case("block", S, B)
    net, dev, _ = _run(rt, p, w, x, mode, B, S)
    ms = net.profile_convs(_cuda(x))
    assert ms[0] > 0.0 and ms[1] > 0.0 and ms[2] > 0.0, "a plan that keeps its activations fused the stem"
    worst, frac = _judge(p, w, mode, dev, tag=f"stem-block-{S}x{B}")
    print(f"bn-stats {mode} first layer alone {S} x{B}: worst {worst:.3f} of the per-channel bar, worst differing fraction {frac:.2e}")


@pytest.mark.parametrize("S,B", C.STEM_SIZES)
def test_fused_fp32_stem_per_channel(rt, S, B):
    """conv_stem_f32 (conv0, conv1 and the 1x1 in one kernel): the program's outputs, two convs further on, against the oracle's own walk
    (double sums) and against the one-launch-per-conv form, per channel at the fp32 bar (tests/test_bn_stats_host.py: the oracle's walk
    with fp32 sums stays under 0.06 of it)."""
    from oracle import oracle as O
    p, w, x = C.stem_case("block", S, B)
    ref = O.forward(p, w, x, acc64=True)
    kept = C.oracle_tensors(p, w, x)
    by_dst = {o.dst: o for o in p.conv_ops()}
    ms_ = [C.channel_magnitude(O, by_dst[t], w, kept.__getitem__) for t in p.outputs]
    xd = _cuda(x)
    outs = {}
    for fused in (True, False):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S)
        net.set_stem_fusion(fused)
        outs[fused] = [g.cpu().numpy().reshape(r.shape) for g, r in zip(net.forward(xd), ref)]
        ms = net.profile_convs(xd)
        assert (ms[0] == 0.0) == fused and (ms[2] == 0.0) == fused, "fused stem did not engage" if fused else "fusion could not be switched off"
    worst = 0.0
    for k, (r, m) in enumerate(zip(ref, ms_)):
        for what, a, b in (("fused vs oracle", outs[True][k], r), ("unfused vs oracle", outs[False][k], r), ("fused vs unfused", outs[True][k], outs[False][k])):
            worst = max(worst, C.check_per_channel(a, b, m, (S, B, k, what))[0])
    print(f"bn-stats f32 fused stem {S} x{B}: worst {worst:.3f} of the per-channel bar")


@pytest.mark.parametrize("mode", SIXTEEN)
@pytest.mark.parametrize("S,B", C.STEM_SIZES)
def test_fused_16bit_stem_third_layer_bit_identical_to_its_own_launch(rt, S, B, mode):
    """conv_stem16: the 1x1 after conv1 computed from the staged tile (mode 1) against its own launch (mode 2), bit for bit on every
    head, with trained-like conv0 / conv1 / conv2."""
    p, w, x = C.stem_case("block", S, B)
    xd = _cuda(x)
    outs = {}
    for fusion in (1, 2):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S, DTYPES[mode])
        net.set_lanes(1)
        _stem_switch(net, mode, fusion)
        outs[fusion] = [g.clone() for g in net.forward(xd)]
        ms = net.profile_convs(xd)
        assert ms[0] == 0.0 and ms[1] > 0.0, "fused stem did not engage"
        assert (ms[2] == 0.0) == (fusion == 1), "the 1x1 third layer: wrong launch structure for this mode"
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.5 for g in outs[fusion])
    assert all(torch.equal(a, b) for a, b in zip(outs[1], outs[2])), "phase 3 differs from the stand-alone 1x1 launch"
    print(f"bn-stats {mode} fused stem third layer {S} x{B}: bit-identical to its own launch, worst 0.000 of the bar")


@pytest.mark.parametrize("mode", SIXTEEN)
@pytest.mark.parametrize("S,B", C.STEM_SIZES)
def test_fused_16bit_stem_conv0_error_bounded_per_channel(rt, S, B, mode):
    """conv_stem16's conv0 (split 16-bit operands; fp16: weights normalised per channel by pack_stem28_norm) through identity heads: conv1's
    stored output from the fused kernel, from the one-launch-per-conv form and from the oracle, pairwise, every element within its own
    ulp + one ulp-at-unit-scale of m_c, the differing fractions within the caps (bn_stat_cases.STEM_*).  conv0's channel 9 has every raw
    weight below 2^-14, channels 3 and 19 gamma 0."""
    p, w, x = C.stem_case("identity", S, B)
    r = C.stem_references(S, B, mode)
    xd = _cuda(x)
    outs = {}
    for fused in (True, False):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S, DTYPES[mode])
        net.set_lanes(1)
        _stem_switch(net, mode, 2 if fused else 0)
        outs[fused] = net.forward(xd)[0].cpu().numpy().reshape(r["oracle"].shape)
        assert (net.profile_convs(xd)[0] == 0.0) == fused, "the fused stem did not engage" if fused else "fused without the switch"
        assert np.isfinite(outs[fused]).all()
    worst_all = 0.0
    for name, a, b in (("fused vs two-launch", outs[True], outs[False]), ("fused vs oracle", outs[True], r["oracle"]),
                       ("two-launch vs oracle", outs[False], r["oracle"])):
        frac, beyond, worst = C.stem_compare(a, b, r["m"], mode)
        print(f"bn-stats {mode} stem {S} x{B}, {name}: {frac:.3e} differ (cap {C.STEM_DIFFER_CAP[mode]:.1e}), {beyond:.3e} beyond their own ulp "
              f"(cap {C.STEM_BEYOND_CAP[mode]:.1e}), worst {worst:.3f} of the per-channel bar")
        assert worst <= 1.0, (name, worst)
        assert frac <= C.STEM_DIFFER_CAP[mode] and beyond <= C.STEM_BEYOND_CAP[mode], (name, frac, beyond)
        worst_all = max(worst_all, worst)
    print(f"bn-stats {mode} fused stem conv0 {S} x{B}: worst {worst_all:.3f} of the per-channel bar")


# ---------------------------------------------------------------------------------------------- e. fused head decode
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nc", C.HEAD_CLASS_COUNTS)
def test_head_decode_bit_identical_and_raw_grid_per_channel(rt, anchors, nc, mode):
    """One head conv per scale with trained-like biases: forward_decode (nc = 80: the head convs decode their own tiles and never store
    the grid; nc = 7: the composed route) bit for bit forward + yolo_decode_scores, and the raw grids per channel against the oracle."""
    p, w, x = C.head_case(nc)
    B = C.HEAD_BATCH
    assert head_route(nc) == ("fused" if nc == 80 else "composed") and tuple(p.grid_sizes(C.HEAD_CANVAS)) == C.HEAD_GRIDS
    xh = _host_input(x, mode)
    xin = _feed(rt, mode, xh)
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, C.HEAD_CANVAS, DTYPES[mode])
    net.set_stem_fusion(0)          # conv0 and conv1 launched one by one, as in the plan below that keeps its activations
    grids = [g.clone() for g in net.forward(xin)]
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, nc)
    for _ in range(2):
        fb, fc, fs = net.forward_decode(xin, anchors)
        torch.cuda.synchronize()
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss), "forward_decode differs from the composed route"
    assert bool(torch.isfinite(ss).all()) and int(cc.max()) < nc and float(ss.max()) > 0.1
    net, dev, kept_grids = _run(rt, p, w, x, mode, B, C.HEAD_CANVAS)
    assert all(torch.equal(a, b) for a, b in zip(grids, kept_grids))        # the grids the decode was checked on are the ones judged
    worst, frac = _judge(p, w, mode, dev, tag=f"heads-nc{nc}")
    print(f"bn-stats {mode} heads nc={nc} ({head_route(nc)} route): decode bit-identical, raw grids worst {worst:.3f} of the per-channel bar")


# ---------------------------------------------------------------------------------------------- f. the whole network
@pytest.mark.parametrize("mode,low_latency", [("f32", False), ("bf16", False), ("f16", False), ("f32", True)],
                         ids=["f32", "bf16", "f16", "f32-low-latency-b1"])
def test_network_every_layer_teacher_forced_per_channel(rt, program, mode, low_latency):
    """YOLOv3 at 64 x 64 with calibrated trained-like statistics: every fused launch recomputed by the oracle from the device's own input
    tensors, as test_bf16_every_layer_teacher_forced_within_one_ulp does, with the per-channel bars."""
    w, x = C.network_case(program)
    B = 1 if low_latency else C.NET_B
    net, dev, _ = _run(rt, program, w, x[:B], mode, B, C.NET_S, (lambda n: n.set_low_latency(True)) if low_latency else None)
    splits = [net.split_k(i) for i in range(len(net.conv_ops))]
    assert (max(splits) > 1) == low_latency, splits
    worst, frac = _judge(program, w, mode, dev, tag="network")
    print(f"bn-stats {mode}{' low-latency' if low_latency else ''} network {B} x {C.NET_S}^2: 75 launches, worst {worst:.3f} of the per-channel bar, "
          f"worst differing fraction {frac:.2e}" + (f", {sum(s > 1 for s in splits)} convs split" if low_latency else ""))


# ---------------------------------------------------------------------------------------------- g. the two-plane mode's range check
def test_x2_range_check_refuses_by_name_at_65504(rt):
    """A BN-scaled weight of 65504 x (1 + 1e-3) in one channel: plan(Y3_DTYPE_F32X2) refuses the net by name, fp32 plans it and passes per
    channel; at 65504 x (1 - 1e-3) the two-plane mode plans too and passes."""
    for over in (True, False):
        p, w, x = C.range_case(over)
        net = rt.Net(p)
        net.load_weights(w)           # loading succeeds: the other modes can use these weights
        if over:
            with pytest.raises(rt.Y3Error, match="conv 0 has a BN-scaled weight outside the fp16 range"):
                net.plan(2, 8, _lib.Y3_DTYPE_F32X2)
        for mode in ("f32",) if over else ("f32", "f32x2"):
            net, dev, _ = _run(rt, p, w, x, mode, 2, 8)
            worst, _ = _judge(p, w, mode, dev, tag="range-over" if over else "range-under")
            top = float(np.abs(w["conv0.w"][..., C.RANGE_CHANNEL]).max())
            print(f"bn-stats range check, {'over' if over else 'under'} 65504, {mode}: worst {worst:.3f} of the per-channel bar (raw |w|max {top:.3g})")
