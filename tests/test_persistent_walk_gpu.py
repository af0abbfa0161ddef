"""The seven persistent kernels on walks of THREE tiles per workgroup, on the GPU (cases, geometry and references:
tests/persistent_cases.py; their basis: tests/test_persistent_walk_host.py).  The shapes of the other kernel-level tests give these kernels
one tile per workgroup, two at 416 x 416; here every launch has workgroups with three tiles and workgroups with two, and a workgroup's
successive tiles lie at different positions of different images.

Per case, one plan for all B images on one lane, every conv that is not the persistent launch on a forced tile:
  (a) forward on all B images == the concatenation of forwards on chunks so small that every workgroup has at most one tile; bit for bit,
      every output and every probed tensor (the kernels promise an element's bits do not depend on its image, the batch or the lane);
  (b) the wrap images of the big batch against the CPU reference of those images alone, under the bars the kernels' own tests use;
  (c) weight-resident convs: the big batch on tile 32 / 33 == the big batch on the generic tile of the same MFMA shape, bit for bit;
  (d) two forwards of the big batch are bit-equal;
  (e) per kernel family, a captured graph's replay == the eager forward.
Reading a failure of (a): the message names the walk indices of the differing pixels (persistent_cases.locate maps element -> tile ->
workgroup -> walk index); with keep_activations / read_tensor the weight-resident cases compare the persistent launches' own outputs."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import persistent_cases as P  # noqa: E402
from tests.helpers import f32_conv_bar, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

DT = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16}
# tiles tried in turn for a conv that is not the persistent launch (the first one its setter accepts): fp32; 16-bit with BK = 64; with BK = 32
OTHER_TILES = {"f32": (11, 10, 9, 8, 6), "k64": (11, 10, 12, 3, 4, 8), "k32": (6, 5, 22)}


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    _lib.require_gpu()  # fail loudly, never fall back
    return runtime


def _n_cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _device_input(case, x):
    xd = torch.from_numpy(np.array(x, order="C")).cuda()      # a copy: the cached input is read-only
    if case.family == "res16":
        xd = xd.to(torch.bfloat16 if case.fmt == "bf16" else torch.float16)
    return xd


def _build(rt, case, resident=True, keep=None):
    """The planned net of a case: the persistent kernel engaged (resident=False: the generic tile in the weight-resident convs' place),
    every other MFMA conv on a forced tile, no early chunk, no split-K, one lane."""
    p, w, _ = P.inputs(case)
    net = rt.Net(p)
    net.load_weights(w)
    res = case.family in ("res16", "res32")
    set_tile = net.set_tile if case.fmt == "f32" else net.set_tile_bf16
    in_stem = {"tiny": (0, 1), "stem": (0, 1, 2) if case.fmt == "f32" else (0, 1)}.get(case.family, ())
    forced = {}
    for slot, o in enumerate(net.conv_ops):
        if slot in in_stem or o.cin == 3:
            continue
        if res and o.size == 3:
            forced[slot] = P.RESIDENT_TILE[case.family] if resident else P.GENERIC_TILE[case.family](o.cin)
            set_tile(slot, forced[slot])
            continue
        for t in OTHER_TILES["f32" if case.fmt == "f32" else "k64" if o.cin % 64 == 0 else "k32"]:
            try:
                set_tile(slot, t)
            except rt.Y3Error:
                continue
            forced[slot] = t
            break
        assert slot in forced, (case.name, slot, "no tile of the list fits this conv")
    if case.family == "tiny":
        net.set_tiny_stem_fusion(True)
    if case.family == "stem" and case.fmt == "f16":
        net.set_stem_fusion_f16(2)
    net.set_early_chunk(0, 0)
    net.keep_activations(res if keep is None else keep)
    net.plan(case.B, case.canvas if case.canvas[0] != case.canvas[1] else case.canvas[0], DT[case.fmt])
    net.set_lanes(1)
    return net, forced


def _forward(net, xd, probes):
    """Outputs, then the probed stored tensors, of one forward; clones."""
    outs = [g.clone() for g in net.forward(xd)]
    return outs + [net.read_tensor(t, xd.shape[0]).clone() for t in probes]


@pytest.fixture(scope="module")
def big(request, rt):
    """One case's planned net and the result of its forward on all B images; built once per case (pytest groups the tests by it)."""
    case = request.param
    g = P.geometry(case, _n_cus())
    p, w, x = P.inputs(case)
    net, forced = _build(rt, case)
    xd = _device_input(case, x)
    probes = P.probes(case, p)
    one = xd[:1].contiguous()
    if case.family == "tiny":
        assert net.tiny_stem_fused == 1
    elif case.family == "stem":
        ms = net.profile_convs(one)
        assert ms[0] == 0.0 and ms[1] > 0.0, "the fused stem did not engage"
        assert (ms[2] == 0.0) == (case.fmt == "f32"), "the 1x1 third layer of the fp32 case runs inside the stem kernel, and only there"
    full = _forward(net, xd, probes)
    torch.cuda.synchronize()
    return SimpleNamespace(case=case, g=g, p=p, w=w, x=x, xd=xd, net=net, forced=forced, probes=probes, full=full)


def _all(cases):
    return pytest.mark.parametrize("big", cases, indirect=True, ids=[c.name for c in cases])


def _where(s, a, b):
    """Which pixels of two tensors differ, in the persistent launch's terms."""
    diff = a != b
    if not bool(diff.any()):
        return "equal"
    m = diff.reshape(diff.shape[0], diff.shape[1], diff.shape[2], -1).any(dim=3).cpu().numpy()
    walks = P.walk_index_map(s.case, s.g)
    text = f"{int(diff.sum())} elements in {int(m.sum())} pixels of images {sorted(set(np.nonzero(m)[0].tolist()))[:12]}"
    if m.shape == walks.shape:
        text += f"; walk index -> differing pixels {dict((int(k), int((m & (walks == k)).sum())) for k in np.unique(walks))}"
        b0, y0, x0 = (int(v[0]) for v in np.nonzero(m))
        text += f"; first at image {b0} pixel ({y0}, {x0}): (tile, workgroup, walk index) {P.locate(s.case, s.g, b0, y0, x0)}"
    return text


# ---------------------------------------------------------------------------------------------- the cases on this device
@_all(P.CASES)
def test_case_has_walks_of_three_and_of_two_on_this_device(big):
    print(P.describe(big.case, big.g))
    P.check_conditions(big.case, big.g)


# ---------------------------------------------------------------------------------------------- (a) walk invariance
@_all(P.CASES)
def test_big_batch_equals_its_one_tile_chunks_bit_for_bit(big):
    s, g = big, big.g
    print(P.describe(s.case, g))
    parts = []
    for i in range(0, s.case.B, g.chunk):
        xs = s.xd[i:i + g.chunk]
        assert xs.shape[0] * g.tiles_per_image <= g.stride, "a chunk gives no workgroup a second tile"
        parts.append(_forward(s.net, xs, s.probes))
    torch.cuda.synchronize()
    names = [f"output {k}" for k in range(len(s.p.outputs))] + [f"tensor {t}" for t in s.probes]
    for k, (name, full) in enumerate(zip(names, s.full)):
        cat = torch.cat([part[k] for part in parts])
        assert cat.shape == full.shape and bool(torch.isfinite(full).all())
        assert torch.equal(cat, full), (s.case.name, name, _where(s, full, cat))


# ---------------------------------------------------------------------------------------------- (b) the wrap images against the CPU reference
def _wrap_reference(s):
    return P.wrap_reference(s.case) if s.g.wrap == P.geometry(s.case).wrap else P.reference(s.case, s.g.wrap)


def _np(t, wrap):
    return np.ascontiguousarray(t[wrap].cpu().numpy())


def _b_tiny(s, ref):
    from tests import tiny_stem_cases as T
    a, b = _np(s.full[0], s.g.wrap), _np(s.full[1], s.g.wrap)
    assert np.array_equal(a, b) and not a[..., 32:].any(), "the identity heads agree and carry zeros behind channel 31"
    got = np.ascontiguousarray(a[..., :32])
    if s.case.fmt == "f32":
        err, bar = float(np.abs(got - ref["f64"]).max()), f32_conv_bar(ref["f64"])
        print(f"{s.case.name} wrap images: {err:.3e} = {err / bar:.4f} of the bar {bar:.3e}")
        assert got.shape == ref["f64"].shape and err <= bar, (err, bar)
        return
    fmt = s.case.fmt
    differ, beyond, worst = T.compare(fmt, got, ref[fmt])
    print(f"{s.case.name} wrap images: differ {differ:.4e} = {differ / P.TINY_CAPS[fmt][0]:.3f} of its cap, beyond one ulp {beyond:.4e} = "
          f"{beyond / P.TINY_CAPS[fmt][1]:.3f} of its cap, worst {worst:.3f} of the per-element bound")
    assert got.shape == ref[fmt].shape
    assert differ <= P.TINY_CAPS[fmt][0] and beyond <= P.TINY_CAPS[fmt][1], (differ, beyond)
    assert worst <= 1.0, worst


def _b_res16_bf16(s, ref):
    """The assertions of tests/test_gpu_parity.py::test_bf16_weight_resident_3x3_matches_oracle_and_generic_tiles."""
    from tests.tiny_stem_cases import bf16_ulp_elem
    outs_ref, kept = ref
    n = len(s.p.outputs)
    for k, (t, dev) in enumerate(zip(s.probes, s.full[n:])):
        g = _np(dev, s.g.wrap)
        d = np.abs(g - kept[t])
        slack = (1e-5 if k == 0 else 2.0 ** -8) * float(np.abs(kept[t]).max())
        bound = bf16_ulp_elem(g, kept[t]) + slack
        frac = float((d > 0).mean())
        print(f"{s.case.name} wrap images, 3x3 conv {k}: worst {float((d / bound).max()):.3f} of ulp + slack, {frac:.3e} of the elements differ "
              f"(cap {0.002 if k == 0 else 0.05})")
        assert (d <= bound).all(), (t, float(d.max()))
        assert frac <= (0.002 if k == 0 else 0.05), (t, frac)
    for r, dev in zip(outs_ref, s.full[:n]):
        g = _np(dev, s.g.wrap).reshape(r.shape)
        err, bar = float(np.abs(g - r).max()), 4e-3 * max(1.0, float(np.abs(r).max()))
        print(f"{s.case.name} wrap images, head: {err / bar:.4f} of the bar")
        assert err <= bar, (err, bar)


def _b_res16_f16(s, ref):
    """The assertions of tests/test_f16_gpu.py::test_f16_weight_resident_3x3_matches_oracle_and_generic_tiles: every 3x3 launch against the fp16
    oracle on its own device inputs."""
    from oracle import oracle as O
    from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16
    assert ref is None
    n = len(s.p.outputs)
    dev = {t: _np(g, s.g.wrap) for t, g in zip(s.probes, s.full[n:])}
    dev[s.p.input_tensor] = np.ascontiguousarray(s.x[s.g.wrap])
    n3 = 0
    for o in s.p.conv_ops():
        if o.size != 3:
            continue
        with f16_emulation():
            r = oracle_launch(O, o, s.w, dev.__getitem__, acc64=True, bf16_weights=True)
        got = dev[o.dst]
        assert np.array_equal(round_f16(got), got)
        exp = round_f16(r)
        diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
        bar = f16_ulp_elem(got, exp) + 1e-5 * float(np.abs(exp).max())
        frac = float((diff > 0).mean())
        print(f"{s.case.name} wrap images, conv {o.conv_index}: worst {float((diff / bar).max()):.3f} of the bar, {frac:.2e} of the elements differ (cap 1e-2)")
        assert (diff <= bar).all(), (o.conv_index, float((diff / bar).max()))
        assert frac <= 1e-2, (o.conv_index, frac)
        n3 += 1
    assert n3 == 3


def _b_f32_outputs(s, ref):
    """2e-5 * max(1, |ref|max) on every output: the bar of the fp32 weight-resident test and of the fp32 fused-stem test."""
    for k, (r, dev) in enumerate(zip(ref, s.full[:len(s.p.outputs)])):
        g = _np(dev, s.g.wrap).reshape(r.shape)
        err, bar = float(np.abs(g - r).max()), 2e-5 * max(1.0, float(np.abs(r).max()))
        print(f"{s.case.name} wrap images, output {k}: {err:.3e} = {err / bar:.4f} of the bar")
        assert err <= bar, (k, err, bar)


def _b_stem_bf16(s, ref):
    """The bars of tests/test_gpu_parity.py::test_fused_stem_bf16_conv0_error_bounded_through_identity_heads, fused against the oracle."""
    from tests.tiny_stem_cases import bf16_ulp_elem
    a = _np(s.full[0], s.g.wrap).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    d = np.abs(a - ref)
    ulp = bf16_ulp_elem(a, ref)
    frac, beyond = float((d > 0).mean()), float((d > ulp + 1e-5 * scale).mean())
    print(f"{s.case.name} wrap images: {frac:.3e} of the elements differ (cap 0.05), {beyond:.3e} by more than their own ulp (cap 0.01), worst "
          f"{float((d / (ulp + 2.0 ** -8 * scale)).max()):.3f} of ulp + 2^-8 of the scale")
    assert (d <= ulp + 2.0 ** -8 * scale).all(), float(d.max())
    assert frac <= 0.05 and beyond <= 0.01, (frac, beyond)


def _b_stem_f16(s, ref):
    """The comparison and caps of tests/test_f16_stem_gpu.py, fused against the oracle (the reference alone stays within half of those caps
    on these images: tests/test_persistent_walk_host.py)."""
    from tests import f16_stem_cases as F
    from tests.f16_oracle import round_f16
    from tests.test_f16_stem_host import STEM_BEYOND_CAP, STEM_DIFFER_CAP
    r = ref["oracle"]
    a = _np(s.full[0], s.g.wrap).reshape(r.shape)
    assert np.isfinite(a).all() and np.array_equal(round_f16(a), a)
    frac, beyond, worst = F.compare(a, r, float(np.abs(r).max()))
    print(f"{s.case.name} wrap images: {frac:.3e} of the elements differ = {frac / STEM_DIFFER_CAP:.3f} of the cap, {beyond:.3e} by more than their "
          f"own ulp = {beyond / STEM_BEYOND_CAP:.3f} of the cap, worst {worst:.3f} of ulp + 2^-11 of the scale")
    assert worst <= 1.0, worst
    assert frac <= STEM_DIFFER_CAP and beyond <= STEM_BEYOND_CAP, (frac, beyond)


@_all(P.CASES)
def test_wrap_images_of_the_big_batch_against_the_cpu_reference(big):
    s = big
    print(P.describe(s.case, s.g))
    ref = _wrap_reference(s)
    key = (s.case.family, s.case.fmt)
    check = {("tiny", "f32"): _b_tiny, ("tiny", "bf16"): _b_tiny, ("tiny", "f16"): _b_tiny, ("res16", "bf16"): _b_res16_bf16,
             ("res16", "f16"): _b_res16_f16, ("res32", "f32"): _b_f32_outputs, ("stem", "f32"): _b_f32_outputs, ("stem", "bf16"): _b_stem_bf16,
             ("stem", "f16"): _b_stem_f16}[key]
    check(s, ref)
    if s.case.family == "stem" and s.case.fmt != "f32":      # the three identity heads hand over the same stored tensor
        assert torch.equal(s.full[0], s.full[1]) and torch.equal(s.full[0], s.full[2])


# ---------------------------------------------------------------------------------------------- (c) resident == generic on the walk of three
@_all(P.RES_CASES)
def test_weight_resident_big_batch_equals_the_generic_tile_bit_for_bit(big, rt):
    s = big
    print(P.describe(s.case, s.g))
    net, forced = _build(rt, s.case, resident=False)
    resident = {k for k, v in s.forced.items() if v == P.RESIDENT_TILE[s.case.family]}
    assert len(resident) == (6 if s.case.family == "res32" else 3) and all(forced[k] == P.GENERIC_TILE[s.case.family](s.case.shape[0]) for k in resident)
    assert all(forced[k] == v for k, v in s.forced.items() if k not in resident), "every other conv runs the tile it ran beside the resident one"
    generic = _forward(net, s.xd, s.probes)
    torch.cuda.synchronize()
    assert len(generic) == len(s.full)
    for k, (a, b) in enumerate(zip(s.full, generic)):
        assert torch.equal(a, b), (s.case.name, k, _where(s, a, b))


# ---------------------------------------------------------------------------------------------- (d) determinism
@_all(P.CASES)
def test_two_forwards_of_the_big_batch_are_bit_equal(big):
    s = big
    print(P.describe(s.case, s.g))
    again = _forward(s.net, s.xd, s.probes)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(s.full, again)):
        assert torch.equal(a, b), (s.case.name, k, _where(s, a, b))


# ---------------------------------------------------------------------------------------------- (e) graph capture and replay
@_all(P.GRAPH_CASES)
def test_graph_replay_of_the_big_batch_equals_the_eager_forward(big, rt):
    """The pattern of tests/test_tiny_stem_gpu.py::test_forward_invariants_with_the_switch_on, on a net of its own without kept activations."""
    s = big
    print(P.describe(s.case, s.g))
    net, _ = _build(rt, s.case, keep=False)
    eager = [g.clone() for g in net.forward(s.xd)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.forward(s.xd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net.forward(s.xd)
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(eager, out)):
        assert torch.equal(a, b), (s.case.name, k, _where(s, a, b))
