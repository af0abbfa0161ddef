"""Conv launches on tensors between 2 GiB and the 4 GiB guard of y3_net_plan_hw (tests/high_offset_cases.py; the arithmetic of the table is
checked in tests/test_high_offsets_host.py): the launches the per-tile suites prove at low addresses, at addresses whose bit 31 is set.
A kernel that is wrong there is wrong silently -- a buffer load past num_records returns zero -- so every case

  1. forces a tile on EVERY conv (the setter refuses a tile that does not fit) and sees every conv launch (profile_convs),
  2. holds the checked images -- image 0, the image across offset 2^31 of every high tensor, the last image -- of every launch to the
     oracle on the launch's OWN device operands, at the bars of the per-tile suites: 2e-5 |ref|max for fp32, f32x3, f32x2 and the fp32
     grids, one ulp (+ 1e-5 |ref|max) per stored bf16 / fp16 element with the suites' caps on the differing share, np.array_equal
     against yolo_v3_tf2_amd/quant.py for int8,
  3. and finds them bit-identical (torch.equal) to the same image run alone through a batch-1 plan with the same forced tiles.

The inputs are made on the device from a seeded generator, the checked images overwritten with known host arrays; of a multi-GB tensor
only the checked images ever leave the device (read_tensor's whole-batch copy on the device is counted in the case's memory budget).
conv_first runs as the Cin = 3 launch of a plan that keeps its activations, in each of the five formats it stores.  For int8 the setter
is the bf16 family's and an int8 form that is not built would fall back to the heuristic silently: tests/test_high_offsets_host.py holds
every forced tile to y3_tile_built and the fit rule of its own family.  Also here: the guard itself, and why no fused stem runs above
2 GiB -- the plan is refused before a stem destination can get there."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import high_offset_cases as hc  # noqa: E402
from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16  # noqa: E402
from tests.helpers import check_f32_conv, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import quant  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_images(case, n):
    """The known images: standard normal, exact in the format the plan takes its input in."""
    from oracle import oracle as O
    p, _ = case.program()
    x = np.random.default_rng(hc.SEED).standard_normal((n, *case.canvas, p.tensors[p.input_tensor].channels)).astype(np.float32)
    return O.round_bf16(x) if case.mode == "bf16" else round_f16(x) if case.mode in ("f16", "i8") else x


def _device_input(rt, case, imgs, host):
    """[B,H,W,C] of the plan's input format, random from a seeded device generator, images `imgs` replaced by `host`."""
    p, _ = case.program()
    B, (H, W), C = case.batch, case.canvas, p.tensors[p.input_tensor].channels
    gen = torch.Generator(device="cuda").manual_seed(hc.SEED)
    if case.mode not in ("f32x3", "f32x2") or C == 3:       # the three-channel image of conv_first is fp32 in every mode
        dt = torch.float32 if C == 3 else {"bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.float16}.get(case.mode, torch.float32)
        x = torch.randn((B, H, W, C), generator=gen, device="cuda", dtype=dt)
        x[torch.tensor(imgs, device="cuda")] = _cuda(host).to(dt)
        return x
    split, npl, dt = (rt.split3_planes, 3, torch.bfloat16) if case.mode == "f32x3" else (rt.split2_planes, 2, torch.float16)
    out = torch.empty((B, H, W, npl, C), device="cuda", dtype=dt)
    step = 4096      # the planes of a slab at a time: the fp32 values of the whole batch are never held
    for s in range(0, B, step):
        xs = torch.randn((min(step, B - s), H, W, C), generator=gen, device="cuda")
        for k, i in enumerate(imgs):
            if s <= i < s + xs.shape[0]:
                xs[i - s] = _cuda(host[k])
        out[s:s + xs.shape[0]] = split(xs)
    return out


def _check_launches(case, p, ops, w, scales, tensor, stored_fmt):
    """Every launch of the program on the checked images, from its own device operands (tensor(id) -> host array of those images)."""
    from oracle import oracle as O
    mode = case.mode
    for name, o in ops.items():
        got = tensor(o.dst)
        what = f"{case.name} conv {name}"
        if mode == "i8":
            exp = quant.conv_i8(o, w, tensor, scales, quant.writes_f32(p, o))
            assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
            assert np.array_equal(got, exp), (what, int((got != exp).sum()), got.size, np.argwhere((got != exp).reshape(got.shape[0], -1).any(1)).ravel())
            assert np.abs(got.astype(np.float32)).max() > 0, what
            continue
        mfma = o.cin != 3        # conv_first: fp32 arithmetic on fp32 weights in every mode, the result rounded to the plan's format
        if mode == "f16":
            with f16_emulation():
                ref = oracle_launch(O, o, w, tensor, acc64=True, bf16_weights=mfma)
        else:
            ref = oracle_launch(O, o, w, tensor, acc64=True, bf16_weights=(mode == "bf16" and mfma))
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        assert np.abs(ref).max() > 0.1, what      # not a comparison of two empty buffers
        if mode in ("bf16", "f16") and o.dst in stored_fmt:
            exp = O.round_bf16(ref) if mode == "bf16" else round_f16(ref)
            ulp = hc.bf16_ulp_elem(got, exp) if mode == "bf16" else f16_ulp_elem(got, exp)
            diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
            bar = ulp + 1e-5 * float(np.abs(exp).max())
            per_image = (diff / bar).reshape(diff.shape[0], -1).max(1)
            frac = float((diff > 0).mean())
            print(f"high-offsets {what}: worst {per_image.max():.3f} of the bar (per checked image {np.round(per_image, 3).tolist()}), {frac:.2e} differ")
            assert (diff <= bar).all(), (what, per_image.tolist())
            assert frac <= hc.DIFFER_CAP[mode], (what, frac)
        else:
            per_image = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
            err, bar = check_f32_conv(got, ref, (what, per_image.tolist()))
            print(f"high-offsets {what}: worst {err / bar:.3f} of the bar")


@pytest.mark.parametrize("case", hc.CASES, ids=[c.name for c in hc.CASES])
def test_launches_above_2_gib(rt, case):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    t0 = time.perf_counter()
    m = hc.MODES[case.mode]
    p, ops = case.program()
    w = synthetic_weights(p, seed=hc.SEED)
    B, canvas, imgs = case.batch, case.canvas, hc.checked_images(case)
    host = _host_images(case, len(imgs))
    scales = None
    if case.mode == "i8":       # calibrated on the known images; the random ones clip where they exceed them, as real activations do
        cal = rt.Net(p)
        cal.load_weights(w)
        scales = cal.calibrate_i8(_cuda(host))
        del cal
    net = rt.Net(p)
    net.load_weights(w)
    if scales is not None:
        net.set_act_scales(scales)
    for slot, tile in hc.forcing(case).items():          # 1. a tile that does not fit is refused here
        if tile != hc.FIRST:                             #    (the Cin = 3 conv takes none: with its activations kept the plan runs it as conv_first)
            getattr(net, m["setter"])(slot, tile)
    net.keep_activations(True)
    if case.border_skip:
        net.set_border_skip(1)
    net.plan(B, canvas, m["dtype"])
    net.set_lanes(case.lanes)
    if case.mode == "i8":
        assert net.i8_first_conv() == 0
    if case.border_skip:
        assert all(net.border_skip(slot, B) == case.lanes for slot, o in enumerate(net.conv_ops) if o.size == 3 and o.src1 < 0)
    torch.cuda.synchronize()
    t_plan = time.perf_counter()
    x = _device_input(rt, case, imgs, host)
    grids = net.forward(x)
    torch.cuda.synchronize()
    t_fwd = time.perf_counter()

    # the checked images of every tensor, sliced on the device
    idx = torch.tensor(imgs, device="cuda")
    staged = hc.staged_outputs(p) if case.mode != "f32" else set()
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    read = net.read_tensor_i8 if case.mode == "i8" else net.read_tensor
    big = {t: g.index_select(0, idx).reshape(len(imgs), g.shape[1], g.shape[2], -1) for t, g in zip(p.outputs, grids)}
    for t in stored + ([p.input_tensor] if case.mode == "i8" else []):
        full = read(t, B)
        big[t] = full.index_select(0, idx)
        del full
    del grids
    ms = net.profile_convs(x)                             # 1. every conv is a launch of its own, on the tile forced above
    assert (ms > 0).all(), ms
    torch.cuda.synchronize()

    t_read = time.perf_counter()

    # 2. teacher-forced, per launch
    dev = {t: g.cpu().numpy() for t, g in big.items()}
    if case.mode == "i8":
        assert np.array_equal(dev[p.input_tensor], quant.quantize(host, scales[p.input_tensor])), "quantize16_to_i8"
    else:
        dev[p.input_tensor] = host
    _check_launches(case, p, ops, w, scales, dev.__getitem__, set(stored) | staged)
    t_host = time.perf_counter()

    # 3. the same images alone, at low addresses, through the same instantiations
    if case.batch_independent:
        net.plan(1, canvas, m["dtype"])
        for k, i in enumerate(imgs):
            g1 = net.forward(x[i:i + 1].contiguous())
            for t, g in zip(p.outputs, g1):
                assert torch.equal(g.reshape(big[t][k:k + 1].shape), big[t][k:k + 1]), (case.name, "image", i, "output", t)
            for t in stored:
                assert torch.equal(read(t, 1), big[t][k:k + 1]), (case.name, "image", i, "tensor", t)
        torch.cuda.synchronize()
    high = {t: hc.tensor_bytes(case, t, nb) for t, (_, nb) in hc.high_tensors(case).items()}
    t_one = time.perf_counter()
    del net, x, big
    torch.cuda.empty_cache()
    t1 = time.perf_counter()
    print(f"high-offsets {case.name}: batch {B}, lanes {case.lanes}, images {imgs}, {len(high)} high tensors of {min(high.values())} .. {max(high.values())} bytes, "
          f"plan {hc.total_bytes(case) / 2 ** 30:.1f} GiB, wall {t1 - t0:.1f} s (weights, calibration, plan {t_plan - t0:.1f}; input, forward "
          f"{t_fwd - t_plan:.1f}; slices, profile {t_read - t_fwd:.1f}; oracle {t_host - t_read:.1f}; batch-1 plan {t_one - t_host:.1f}; free {t1 - t_one:.1f})")


# ---------------------------------------------------------------------------------------------- the guard
def test_plan_refuses_a_tensor_at_the_guard(rt):
    """A plan whose largest tensor reaches 0xFFFFFFF0 bytes is refused before anything is allocated, and the net is left without a plan."""
    case = hc.CASE_BY_NAME["f32-near-guard"]
    p, ops = case.program()
    net = rt.Net(p)
    net.plan(2, case.canvas)
    assert net.flops_per_image() > 0
    per = hc.image_bytes(case, p.input_tensor)
    assert case.batch * per < hc.GUARD <= (case.batch + 1) * per
    with pytest.raises(rt.Y3Error, match="32-bit buffer offsets"):
        net.plan(case.batch + 1, case.canvas)
    assert net.flops_per_image() == 0.0
    x = torch.zeros((1, *case.canvas, 64), device="cuda")
    # the library has no plan and says so; Net knows it as well (include/y3.h, the table at y3_net_plan_hw: outcome (b)) ...
    import ctypes
    grids = (ctypes.c_void_p * 3)()
    assert net.lib.y3_net_forward(net._h, x.data_ptr(), 1, grids, None) == -4 and b"call y3_net_plan first" in net.lib.y3_last_error()
    assert net.lib.y3_net_get_plan(net._h, None, None, None, None) == 0 and (net.max_batch, net.canvas) == (0, (0, 0))
    # ... so its forward plans by itself and gets as far as the weights this net never had
    with pytest.raises(rt.Y3Error, match="has no weights"):
        net.forward(x)
    assert (net.max_batch, net.canvas) == (1, tuple(case.canvas))
    net.plan(2, case.canvas)                               # the net itself is unharmed
    assert net.flops_per_image() > 0


@pytest.mark.parametrize("family", sorted(hc.STEM_FAMILIES))
def test_plan_refuses_a_fused_stem_before_its_destination_passes_2_gib(rt, family):
    """Why no case runs conv_stem_f32 or conv_stem16 above 2 GiB (tests/test_high_offsets_host.py has the arithmetic): at the first batch
    whose stem destination -- conv1's output -- would pass 2^31 bytes, conv0's own tensor, twice as large, is at the guard, and the plan is
    refused for it although the fused kernel would never store it."""
    from tests.f16_stem_cases import stem_program
    from yolo_v3_tf2_amd import _lib
    p = stem_program()
    c0, c1 = p.conv_ops()[0], p.conv_ops()[1]
    eb = hc.STEM_FAMILIES[family]
    dtype = {"conv_stem_f32": _lib.Y3_DTYPE_F32, "conv_stem16_bf16": _lib.Y3_DTYPE_BF16, "conv_stem16_f16": _lib.Y3_DTYPE_F16}[family]
    B = hc.HIGH // (16 * 16 * 64 * eb) + 1                 # 32 x 32, the smallest canvas the stem takes: conv1's output one image past 2^31 bytes
    assert B * 16 * 16 * 64 * eb > hc.HIGH and B * 32 * 32 * 32 * eb >= hc.GUARD
    net = rt.Net(p)
    if family == "conv_stem16_f16":
        net.set_stem_fusion_f16(2)
    else:
        net.set_stem_fusion(2)
    with pytest.raises(rt.Y3Error, match=f"tensor {c0.dst} is .*32-bit buffer offsets"):
        net.plan(B, 32, dtype)
    assert net.flops_per_image() == 0.0 and c1.src0 == c0.dst


def test_plan_counts_an_fp32_grid_at_four_bytes(rt):
    """A bf16 plan whose stored tensors stay under the guard but whose full-resolution fp32 grid -- addressed by the launch that stores it
    with 4-byte elements -- does not: refused like any other tensor."""
    from yolo_v3_tf2_amd import _lib
    p, ops = hc.body_program(64, 128, 64, 64, 128, heads="full")
    H, W = hc.CANVAS
    B = -(-hc.GUARD // (H * W * 128 * 4))
    assert B * H * W * 128 * 2 < hc.HIGH + (1 << 20)       # the widest stored tensor: half the grid
    net = rt.Net(p)
    with pytest.raises(rt.Y3Error, match="32-bit buffer offsets"):
        net.plan(B, hc.CANVAS, _lib.Y3_DTYPE_BF16)
    assert net.flops_per_image() == 0.0
    net.plan(B - 1, hc.CANVAS, _lib.Y3_DTYPE_BF16)
    assert net.flops_per_image() > 0
