"""Conv widths outside YOLOv3's own on the device (tests/odd_width_cases.py): 96, 160, 192 and 384 channels, so that tile counts in N of
3, 5 and 6, a Cin that only the K step of 32 divides, concat boundaries at odd multiples of 32 and three K chunks are launched at all.
Every launch of the program is held to the oracle on the launch's OWN device inputs (teacher-forced), double accumulation on the
reference side, under the project's existing bars:

  fp32, f32x3, f32x2 and every fp32 head of a 16-bit plan:  helpers.f32_conv_bar (K <= 3456 here, inside its stated K <= 4608);
  bf16 stored outputs:  every element within its own bf16 ulp (+ 1e-5 |ref|max) of the rounded reference, at most 2e-3 of a launch's
  elements different at all (tests/test_tile_matrix_gpu.py);  fp16 stored outputs: the same with f16_ulp_elem and 1e-2
  (tests/test_f16_tile_matrix_gpu.py);  tests/test_odd_widths_host.py shows the reference alone stays under half of either cap;
  int8 (g, h1, h2):  bit for bit against quant.conv_i8 on the device's bytes (tests/test_i8_gpu.py::_check_convs).

The three nets of odd_width_cases.unrunnable_programs are refused by plan() in bf16, fp16 and int8 -- by the host, before anything is
allocated or enqueued -- and run in the three fp32-accurate modes."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import odd_width_cases as W  # noqa: E402
from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16  # noqa: E402
from tests.helpers import f32_conv_bar, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import _lib, quant  # noqa: E402

DTYPES = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f32x3": _lib.Y3_DTYPE_F32X3, "f32x2": _lib.Y3_DTYPE_F32X2,
          "f16": _lib.Y3_DTYPE_F16, "i8": _lib.Y3_DTYPE_I8}
SIXTEEN = ("bf16", "f16", "i8")
BIG_B, BIG_CANVAS = 32, (8, 8)          # 32 images: whole 32-row blocks (border skip), tilesM * tilesN >= 64 (XCD order)


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def _bf16_ulp_elem(a, b):
    """Per element: the spacing of bf16 numbers (8 significand bits) in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


_cases = {}


def _case(mode, canvas, batch=W.BATCH, program="odd"):
    """(program, {name: op}, weights, the input in the values the mode's plan is fed): made once, shared, read-only."""
    fmt = "bf16" if mode == "bf16" else "f16" if mode in ("f16", "i8") else "f32"
    key = (program, fmt, canvas, batch)
    if key not in _cases:
        from oracle import oracle as O
        if program == "odd":
            p, ops = W.odd_width_program()
        else:
            p = W.unrunnable_programs()[program][0]
            ops = {f"conv{o.conv_index}": o for o in p.conv_ops()}
        w, x = W.inputs(p, canvas, batch)
        if x.shape[-1] != 3:        # an input that feeds an MFMA conv directly is handed over in the plan's own format
            x = O.round_bf16(x) if fmt == "bf16" else round_f16(x) if fmt == "f16" else x
        x.setflags(write=False)
        _cases[key] = (p, ops, w, x)
    return _cases[key]


_scales = {}


def _i8_scales(rt, canvas, batch=W.BATCH, program="odd"):
    if (program, canvas, batch) not in _scales:
        p, _, w, x = _case("i8", canvas, batch, program)
        cal = rt.Net(p)
        cal.load_weights(w)
        _scales[(program, canvas, batch)] = cal.calibrate_i8(_cuda(x))
    return _scales[(program, canvas, batch)]


def _feed(rt, mode, x):
    """The input in the form a plan of `mode` takes (a 3-channel image is fp32 in every mode)."""
    t = _cuda(x)
    if x.shape[-1] == 3 or mode == "f32":
        return t
    if mode == "f32x3":
        return rt.split3_planes(t)
    if mode == "f32x2":
        return rt.split2_planes(t)
    return t.to(torch.bfloat16 if mode == "bf16" else torch.float16)      # x holds bf16- / fp16-exact values already


def _net(rt, mode, canvas, batch=W.BATCH, program="odd", setup=None, keep=True):
    p, ops, w, x = _case(mode, canvas, batch, program)
    net = rt.Net(p)
    net.load_weights(w)
    if mode == "i8":
        net.set_act_scales(_i8_scales(rt, canvas, batch, program))
    if setup:
        setup(net)
    net.keep_activations(keep)
    net.plan(batch, canvas, DTYPES[mode])
    return net


def _run(rt, net, mode, x):
    """One forward of x[B, ...] -> ([the three grids as [B, h, w, C]] + [every stored conv output], as torch tensors on the device)."""
    p, B = net.program, x.shape[0]
    grids = net.forward(_feed(rt, mode, x))
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    return [g.reshape(B, g.shape[1], g.shape[2], -1) for g in grids] + [net.read_tensor(t, B) for t in stored]


def _dev(p, x, tensors):
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    dev = {t: g.cpu().numpy() for t, g in zip(list(p.outputs) + stored, tensors)}
    dev[p.input_tensor] = np.asarray(x)
    return dev


def _check_launches(mode, p, ops, w, dev, what, only=None):
    """Every launch (or those named in `only`) of a plan of `mode` that is not an int8 launch, against the oracle on the launch's own
    device inputs.  -> (worst deviation as a fraction of the bar, worst fraction of differing 16-bit elements)."""
    from oracle import oracle as O
    cut = quant.first_i8_conv(p) if mode == "i8" else len(p.conv_ops())
    worst, worst_frac = 0.0, 0.0
    for slot, o in enumerate(p.conv_ops()):
        name = next(k for k, v in ops.items() if v is o)
        if slot >= cut or (only and name not in only):
            continue
        w16 = mode in SIXTEEN and o.cin != 3        # the Cin = 3 first layer reads the fp32 image with fp32 weights in every mode
        if mode in ("f16", "i8"):
            with f16_emulation():
                ref = oracle_launch(O, o, w, dev.__getitem__, acc64=True, bf16_weights=w16)
        else:
            ref = oracle_launch(O, o, w, dev.__getitem__, acc64=True, bf16_weights=w16)
        got = dev[o.dst]
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        assert float(np.abs(ref).max()) > 0.1, (what, name)      # not a comparison of two empty buffers
        if mode in SIXTEEN and o.dst not in p.outputs:
            rnd, ulp, cap = (O.round_bf16, _bf16_ulp_elem, W.BF16_DIFFER_CAP) if mode == "bf16" else (round_f16, f16_ulp_elem, W.F16_DIFFER_CAP)
            assert np.array_equal(rnd(got), got), (what, name)                                 # what is stored is 16-bit
            exp = rnd(ref)
            diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
            bar = ulp(got, exp) + 1e-5 * float(np.abs(exp).max())
            frac = float((diff > 0).mean())
            print(f"odd widths {what} conv {name}: worst {float((diff / bar).max()):.3f} of the bar, {frac:.2e} of the elements differ (cap {cap:.0e})")
            assert (diff <= bar).all(), (what, name, float((diff / bar).max()))
            assert frac <= cap, (what, name, frac)
            worst, worst_frac = max(worst, float((diff / bar).max())), max(worst_frac, frac)
        else:
            err, bar = float(np.abs(got - ref).max()), f32_conv_bar(ref)
            print(f"odd widths {what} conv {name}: worst {err / bar:.3f} of the bar")
            assert err <= bar, (what, name, err, bar)
            worst = max(worst, err / bar)
    return worst, worst_frac


def _check_i8(net, p, w, scales, B, tensors, dev):
    """The int8 launches behind the cut, bit for bit, and the boundary copy of what crosses it."""
    from tests.test_i8_gpu import _check_convs
    cut = net.i8_first_conv()
    assert cut == quant.first_i8_conv(p)
    convs = p.conv_ops()
    behind = {o.dst for o in convs[cut:]}
    crossing = {t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind}
    for t in crossing:      # quantize16_to_i8 of the fp16 tensor the device itself holds
        assert np.array_equal(net.read_tensor_i8(t, B).cpu().numpy(), quant.quantize(dev[t], scales[t])), t
    grids = [g.reshape(B, g.shape[1], g.shape[2], -1) for g in tensors[:3]]
    assert _check_convs(net, p, w, scales, B, grids, cut) == len(convs) - cut
    return len(crossing)


# ---------------------------------------------------------------------------------------------- 1. every mode runs the program
@pytest.mark.parametrize("canvas", W.CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("mode", list(DTYPES))
def test_every_mode_runs_the_odd_width_program(rt, mode, canvas):
    """All ten launches under the mode's bars; two forwards of one plan bit-equal; image 0 alone == image 0 of the batch."""
    p, ops, w, x = _case(mode, canvas)
    B = W.BATCH
    net = _net(rt, mode, canvas)
    first = [t.clone() for t in _run(rt, net, mode, x)]
    again = _run(rt, net, mode, x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two forwards of one plan differ"
    dev = _dev(p, x, again)
    what = f"{mode} {canvas[0]}x{canvas[1]}"
    worst, frac = _check_launches(mode, p, ops, w, dev, what)
    if mode == "i8":
        scales = _i8_scales(rt, canvas)
        assert _check_i8(net, p, w, scales, B, again, dev) == 1      # f crosses the cut
        print(f"odd widths {what}: convs g, h1, h2 bit-exact against quant.conv_i8; the int8 copy of f against quant.quantize")
    print(f"odd widths {what} summary: worst {worst:.3f} of the bar, worst differing fraction {frac:.2e}")
    alone = _run(rt, net, mode, x[0:1])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b[0:1]) for a, b in zip(alone, first)), "image 0 alone differs from image 0 of the batch"


# ---------------------------------------------------------------------------------------------- 2. fp32: K order, XCD order, border skip, tiles
def _slot(net, op):
    return next(s for s, o in enumerate(net.conv_ops) if o is op)


def test_f32_k_chunk_walks_three_chunks_or_falls_back(rt):
    """g (Cin = 384): chunk-major with 128 channels per chunk (three chunks) differs from tap-major within the bar only and both pass;
    256 does not divide 384, so the launch falls back to tap-major, bit for bit.  a and c (Cin = 96 <= one chunk) never chunk."""
    canvas = W.CANVASES[0]
    p, ops, w, x = _case("f32", canvas)
    net = _net(rt, "f32", canvas)
    out = {}
    for ck in (0, 128, 256):
        net.set_k_chunk(ck)
        out[ck] = [t.clone() for t in _run(rt, net, "f32", x)]
        torch.cuda.synchronize()
        _check_launches("f32", p, ops, w, _dev(p, x, out[ck]), f"f32 k_chunk {ck}", only=("g", "h1", "h2"))
    gi = 3 + [o.dst for o in p.conv_ops() if o.dst not in p.outputs].index(ops["g"].dst)
    for i, (a, b, c) in enumerate(zip(out[0], out[128], out[256])):
        assert torch.equal(a, c), "k_chunk 256 does not divide Cin = 384: the tap-major launch"
        if i != gi and i not in (1, 2):     # only g, and the heads behind it, see another summation order
            assert torch.equal(a, b)
    g0, g128 = out[0][gi].cpu().numpy(), out[128][gi].cpu().numpy()
    assert not np.array_equal(g0, g128), "three chunks of 128 channels sum in another order than tap-major"
    assert float(np.abs(g0 - g128).max()) <= f32_conv_bar(g0)


_big = {}


def _big_case(rt):
    """The program at 32 images of 8 x 8 in an fp32 plan, every launch checked against the oracle once."""
    if not _big:
        p, ops, w, x = _case("f32", BIG_CANVAS, BIG_B)
        net = _net(rt, "f32", BIG_CANVAS, BIG_B)
        base = [t.clone() for t in _run(rt, net, "f32", x)]
        torch.cuda.synchronize()
        worst, _ = _check_launches("f32", p, ops, w, _dev(p, x, base), f"f32 {BIG_B} x {BIG_CANVAS[0]}x{BIG_CANVAS[1]}")
        print(f"odd widths f32 {BIG_B} x {BIG_CANVAS[0]}x{BIG_CANVAS[1]} summary: worst {worst:.3f} of the bar")
        _big.update(net=net, base=base, p=p, ops=ops, x=x)
    return _big


def test_f32_xcd_orders_are_bit_equal_at_three_and_six_n_tiles(rt):
    """32 x 8 x 8: M = 2048, so a and c (3 N tiles of 64) and g (6) have tilesM * tilesN >= 64 and choose_xcd_gn meets tile counts that
    no power of two divides but 2 (g: a 4 x 2 grid of XCDs) or none (a, c: the contiguous order)."""
    c = _big_case(rt)
    net = c["net"]
    try:
        for border in (0, 1):
            net.set_border_skip(border)
            res = {}
            for xcd in (0, 1):
                net.set_xcd_mode(xcd)
                res[xcd] = [t.clone() for t in _run(rt, net, "f32", c["x"])]
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(res[0], res[1])), border
            assert all(torch.equal(a, b) for a, b in zip(res[0], c["base"])), border
    finally:
        net.set_xcd_mode(1)
        net.set_border_skip(-1)


def test_f32_border_skip_is_bit_equal_at_three_and_six_n_tiles(rt):
    """32 x 8 x 8: a, c and g take the batch-minor launch (y3_net_get_border_skip) with 3 and 6 N tiles; on and off give the same bits."""
    c = _big_case(rt)
    net, ops = c["net"], c["ops"]
    try:
        res = {}
        for mode in (0, 1):
            net.set_border_skip(mode)
            for k in ("a", "c", "g"):
                assert net.border_skip(_slot(net, ops[k]), BIG_B) == mode, (k, mode)
            for k in ("b", "d", "e", "f", "h0", "h1", "h2"):      # 1x1, stride-2-of-another-geometry or two sources
                assert net.border_skip(_slot(net, ops[k]), BIG_B) == (mode if ops[k].size == 3 else 0), (k, mode)
            res[mode] = [t.clone() for t in _run(rt, net, "f32", c["x"])]
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
        assert all(torch.equal(a, b) for a, b in zip(res[0], c["base"]))
    finally:
        net.set_border_skip(-1)


F32_GENERIC = [t for t in range(len(_lib.TILES)) if t not in _lib.RETIRED_TILES and t != 33]


@pytest.mark.parametrize("tile", F32_GENERIC, ids=[f"f32-t{t}" for t in F32_GENERIC])
def test_f32_every_generic_tile_that_fits_g_and_b(rt, tile):
    """g (Cout = 384: every N width divides it, 3, 6 or 12 N tiles) and b (Cout = 96: the 32-wide tile alone), forced, at the fp32 bar."""
    canvas = W.CANVASES[0]
    p, ops, w, x = _case("f32", canvas)
    bn = _lib.TILES[tile][1]
    want = [k for k in ("g", "b") if ops[k].cout % bn == 0]
    assert "g" in want and (("b" in want) == (bn == 32))
    forced = []

    def setup(net):
        for k in ("g", "b"):
            try:
                net.set_tile(_slot(net, ops[k]), tile)
            except rt.Y3Error as e:
                if "tile does not" not in str(e):
                    raise
                continue
            forced.append(k)

    net = _net(rt, "f32", canvas, setup=setup)
    assert forced == want
    out = _run(rt, net, "f32", x)
    torch.cuda.synchronize()
    worst, _ = _check_launches("f32", p, ops, w, _dev(p, x, out), f"f32 forced tile {tile}", only=forced)
    print(f"odd widths f32 forced tile {tile} on {forced}: worst {worst:.3f} of the bar")


# ---------------------------------------------------------------------------------------------- 3. split-K on g
SPLITS = [("f32", 3), ("f32", 5), ("bf16", 2), ("bf16", 3), ("f16", 2), ("f16", 3), ("i8", 3)]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode,S", SPLITS, ids=[f"{m}-S{s}" for m, s in SPLITS])
def test_split_k_on_g(rt, mode, S, B):
    """g (K = 3456: 108 K tiles of 32, 54 of 64, 27 of 128) cut into S slices, one and two images, against the unsplit launch of the same
    plan mode on the same input tensor f: bit-equal in int8 (integer sums), within the mode's per-launch bar otherwise -- and the split
    launch itself under the oracle's bar."""
    canvas = W.CANVASES[0]
    p, ops, w, x = _case(mode, canvas, B)
    sfx = {"f32": "", "bf16": "_bf16", "f16": "_f16", "i8": "_i8"}[mode]
    base = _net(rt, mode, canvas, B)
    slot = _slot(base, ops["g"])
    want = _run(rt, base, mode, x)
    net = _net(rt, mode, canvas, B, setup=lambda n: getattr(n, "set_split_k" + sfx)(slot, S))
    assert [getattr(net, "split_k" + sfx)(s) for s in range(len(net.conv_ops))] == [S if s == slot else 1 for s in range(len(net.conv_ops))]
    got = _run(rt, net, mode, x)
    torch.cuda.synchronize()
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    gi = 3 + stored.index(ops["g"].dst)
    for i, (a, b) in enumerate(zip(want, got)):
        if mode == "i8" or i not in (gi, 1, 2):
            assert torch.equal(a, b), (i, "only g and the heads behind it may move, and nothing in int8")
    dev = _dev(p, x, got)
    what = f"{mode} split S={S} B={B}"
    if mode == "i8":
        assert _check_i8(net, p, w, _i8_scales(rt, canvas, B), B, got, dev) == 1
        return
    _check_launches(mode, p, ops, w, dev, what, only=("g", "h1", "h2"))
    g0, g1 = want[gi].cpu().numpy(), got[gi].cpu().numpy()
    if mode == "f32":
        err, bar = float(np.abs(g0 - g1).max()), f32_conv_bar(g0)
    else:
        ulp = _bf16_ulp_elem if mode == "bf16" else f16_ulp_elem
        d = np.abs(g1.astype(np.float64) - g0.astype(np.float64))
        err_bar = d / (ulp(g1, g0) + 1e-5 * float(np.abs(g0).max()))
        err, bar = float(err_bar.max()), 1.0
    print(f"odd widths {what}: split against unsplit, worst {err / bar:.3f} of the bar")
    assert err <= bar, (what, err, bar)


# ---------------------------------------------------------------------------------------------- 4. detect on 96- and 160-channel sources
SCORE_THRESHOLD = 0.005      # synthetic heads: objectness bias -4 (tests/test_class_counts_gpu.py)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_detect_equals_the_composed_pipeline_on_odd_head_sources(rt, anchors, mode):
    """Heads of 255 channels reading 96- and 160-channel tensors: heads_can_decode (Cin % 64 != 0) sends y3_net_detect to the composed
    route; it equals forward + decode + NMS + pack bit for bit, twice, and image 0 alone equals image 0 of the batch."""
    nc, B, S = 80, 3, 64
    p = W.detect_program(nc)
    w, x = W.inputs(p, (S, S), B)
    x = _cuda(np.abs(x) % 1.0)
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, S, DTYPES[mode])
    grids = net.forward(x)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, nc)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, SCORE_THRESHOLD)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    assert int(nv.min()) > 0 and bool(torch.isfinite(bb).all())
    for _ in range(2):
        fb, fc, fs = net.forward_decode(x, anchors)
        packed, nv2 = net.detect(x, anchors, 100, 0.5, SCORE_THRESHOLD)
        torch.cuda.synchronize()
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss), (mode, "forward_decode")
        assert torch.equal(nv2, nv) and torch.equal(packed, want), (mode, "detect")
    p0, n0 = net.detect(x[0:1].contiguous(), anchors, 100, 0.5, SCORE_THRESHOLD)
    torch.cuda.synchronize()
    assert torch.equal(n0, nv[0:1]) and torch.equal(p0, want[0:1]), (mode, "detect of image 0 alone")


# ---------------------------------------------------------------------------------------------- 5. nets the 16-bit modes cannot run
@pytest.mark.parametrize("name", list(W.unrunnable_programs()))
def test_unrunnable_nets_are_refused_by_plan_and_run_in_the_fp32_modes(rt, name):
    canvas, B = W.CANVASES[0], W.BATCH
    p, slot, (cin, c0, cout) = W.unrunnable_programs()[name]
    p, ops, w, x = _case("f32", canvas, B, name)
    net = rt.Net(p)
    net.load_weights(w)
    scales = net.calibrate_i8(_cuda(x))     # an fp32 plan of the same object; the int8 plan below then has its scales
    assert quant.first_i8_conv(p) == len(p.conv_ops()) - 3 > slot
    shape = re.escape(f"conv {slot} (Cin {cin}, c0 {c0}, Cout {cout}) has no ")
    for mode, text in (("bf16", "bf16 tile"), ("f16", "fp16 tile"), ("i8", "fp16 tile (it lies before the int8 cut")):
        with pytest.raises(rt.Y3Error, match=shape + re.escape(text)):
            net.plan(B, canvas, DTYPES[mode])
        # the refusal left no plan: nothing to read, and the next plan starts from nothing
        assert net.i8_first_conv() == -1
        with pytest.raises(rt.Y3Error):
            net.read_tensor(p.conv_ops()[slot].dst, B)
    torch.cuda.synchronize()
    for mode in ("f32", "f32x3", "f32x2"):
        net.keep_activations(True)
        net.plan(B, canvas, DTYPES[mode])
        out = _run(rt, net, mode, x)
        torch.cuda.synchronize()
        worst, _ = _check_launches(mode, p, ops, w, _dev(p, x, out), f"{name} {mode}")
        print(f"odd widths {name} {mode} summary: worst {worst:.3f} of the bar")
    assert scales and all(s > 0 for t, s in enumerate(scales) if any(o.dst == t for o in p.conv_ops()))
