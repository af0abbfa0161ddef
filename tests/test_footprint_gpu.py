"""What each launch writes and where (tests/footprint_cases.py; the basis is checked on the CPU by tests/test_footprint_host.py).  The
parity suites hold values to the oracle; here nothing is compared with a reference but the device with itself, bit for bit, and with
poison: no tolerance anywhere.

1. Lane regions: a chain at 5 x 5 pixels, whose stored tensors have per-image sizes that are no multiple of 256 bytes, on three and four
   lanes against one lane.  A race: two lanes that share bytes corrupt a forward only when their kernels overlap in time, so this test
   may pass on a rule that lets regions overlap.  The proof is the sweep of tests/test_footprint_host.py.
2. Caller-owned outputs between poisoned guards (footprint_cases.guarded): y3_net_forward of YOLOv3 in all six modes, at other class
   counts, of YOLOv3-tiny and of raw-feature programs; y3_net_forward_decode; y3_net_detect and y3_net_detect_grids; the stand-alone
   max-pool, decode, class-score, candidate and pack ops.
3. Arena tensors beyond the call's batch: after five images, a forward of three leaves images 3 and 4 of every stored tensor alone."""
import ctypes as C_

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import footprint_cases as F  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402
from yolo_v3_tf2_amd._args import _anchors, _dev, _fptr  # noqa: E402

TORCH_DTYPE = {"float32": torch.float32, "int32": torch.int32, "int64": torch.int64, "bfloat16": torch.bfloat16, "float16": torch.float16}


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


_nets = {}


@pytest.fixture(scope="module", autouse=True)
def _release_nets():
    yield
    _nets.clear()


def _net(rt, key):
    """One Net per program with its weights loaded, shared by the module's tests; every test plans it for itself."""
    if key not in _nets:
        net = rt.Net(F.program(key))
        net.load_weights(F.weights(key))
        _nets[key] = net
    return _nets[key]


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def _feed(rt, mode, x):
    """The input in the form a plan of `mode` takes (a 3-channel image is fp32 in every mode)."""
    t = _cuda(x)
    if x.shape[-1] == 3 or mode == "f32":
        return t
    if mode == "f32x3":
        return rt.split3_planes(t)
    if mode == "f32x2":
        return rt.split2_planes(t)
    return t.to(torch.bfloat16 if mode == "bf16" else torch.float16)


def _plan(net, mode, canvas, max_batch, x=None, keep=False, tiny_stem=None):
    """Plan a shared net: one lane, the switches a test may have left set put back.  x: the fp32 batch an int8 plan is calibrated on."""
    if mode == "i8":
        net.calibrate_i8(x)
    if net.program.nclasses > 0:
        net.nms_per_class = False
        net.multi_label = False
    net.set_tiny_stem_fusion(bool(tiny_stem))
    net.keep_activations(keep)
    net.plan(max_batch, canvas, F.MODES[mode])
    net.set_lanes(1)


def _check(g, ref, what, written=True):
    """One guarded output after the call and a synchronize: guards intact; no poison left in the body; the body is the unguarded call's."""
    assert F.guards_intact(g), f"{what}: written outside the tensor"
    if written:
        assert F.poison_words(g.tensor) == 0, f"{what}: {F.poison_words(g.tensor)} words of the tensor were never written"
    assert F.same_bits(g.tensor, ref), f"{what}: differs from the same call into an ordinary tensor"


def _ids(cases):
    return [c.name for c in cases]


def test_the_guard_helpers_see_what_they_must(rt):
    """One byte written in front of or behind the tensor (inside the allocation the test owns) breaks guards_intact; an element never
    stored, or one image of a grid, shows in poison_words; a tensor whose byte count is no multiple of 4 has its odd tail bytes looked at."""
    for shape, dtype in (((3, 3, 3, 3, 85), torch.float32), ((3, 189), torch.int64), ((3,), torch.int32), ((1, 3, 3, 5), torch.bfloat16)):
        g = F.guarded(shape, dtype)
        itemsize = g.tensor.element_size()
        assert g.lo >= F.guard_bytes(shape, itemsize) and g.buf.numel() - g.hi >= F.guard_bytes(shape, itemsize)
        assert g.hi - g.lo == g.tensor.numel() * itemsize and g.tensor.data_ptr() == g.buf.data_ptr() + g.lo
        assert F.guards_intact(g)
        if itemsize >= 4:
            assert F.poison_words(g.tensor) == g.tensor.numel() * itemsize // 4
        g.tensor.zero_()
        assert F.guards_intact(g) and (itemsize < 4 or F.poison_words(g.tensor) == 0)
        for at in (0, g.lo - 1, g.hi, g.hi + 1, g.hi + 5, g.buf.numel() - 1):
            keep = int(g.buf[at])
            g.buf[at] = keep ^ 1
            assert not F.guards_intact(g), (shape, at)
            g.buf[at] = keep
            assert F.guards_intact(g)
    g = F.guarded((4, 3, 3, 3, 85), torch.float32)
    g.tensor[:3].zero_()
    assert F.poison_words(g.tensor[:3]) == 0 and F.poison_words(g.tensor[3:]) == g.tensor[3:].numel()
    g.tensor[3, 2, 2, 2, 84] = 1.0
    assert F.poison_words(g.tensor[3:]) == g.tensor[3:].numel() - 1
    assert not F.same_bits(g.tensor[:1], g.tensor[3:]) and F.same_bits(g.tensor[:1], g.tensor[1:2])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 1. lane regions
@pytest.mark.parametrize("B", F.LANE_CHAIN_BATCHES)
@pytest.mark.parametrize("mode", ("f32", "bf16", "i8"))
def test_three_and_four_lanes_equal_one_lane_at_unaligned_regions(rt, mode, B):
    """Outputs and every stored tensor of lanes 3 and 4 equal those of one lane bit for bit, two forwards each, at batch B and then B - 1
    on the same plan.  This is a race and may pass on a rule whose regions overlap; tests/test_footprint_host.py::test_lane_regions_sweep
    is the proof."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = F.lane_chain_program()[mode]
    x = np.random.default_rng(F.IMAGE_SEED).standard_normal((B, F.LANE_CHAIN_CANVAS, F.LANE_CHAIN_CANVAS, 64)).astype(np.float32)
    net = rt.Net(p)
    net.load_weights(synthetic_weights(p, seed=F.SEED))
    xf = _cuda(x).to(torch.float16).float() if mode == "i8" else _cuda(x)      # fp16-exact values for the plan that is fed fp16
    _plan(net, mode, F.LANE_CHAIN_CANVAS, B, x=xf, keep=True)
    xd = xf.to(torch.float16) if mode == "i8" else _feed(rt, mode, x)
    stored = sorted(F.stored_image_bytes(p, mode, F.LANE_CHAIN_CANVAS))
    as_i8 = []
    if mode == "i8":
        cut = net.i8_first_conv()
        convs = p.conv_ops()
        behind = {o.dst for o in convs[cut:]}
        crossing = {t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind and t != p.input_tensor}
        as_i8 = sorted((behind - set(p.outputs)) | crossing)
        assert as_i8

    def run(batch):
        outs = [g.clone() for g in net.forward(xd[:batch].contiguous())]
        outs += [net.read_tensor(t, batch) for t in stored] + [net.read_tensor_i8(t, batch) for t in as_i8]
        torch.cuda.synchronize()
        return outs

    for batch in (B, B - 1):
        net.set_lanes(1)
        one = run(batch)
        assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) > 0 for t in one)
        for lanes in (3, 4):
            net.set_lanes(lanes)
            for rep in range(2):
                got = run(batch)
                bad = [i for i, (a, b) in enumerate(zip(one, got)) if not F.same_bits(a, b)]
                assert not bad, (mode, B, batch, lanes, rep, bad)
    # what y3_net_read_tensor refuses: a batch no plan has, and a batch other than the one the lanes wrote into regions that do not follow
    # one another (3200-byte images on four lanes)
    n = C_.c_size_t()
    for bad_batch in (0, -1, B + 1):
        assert net.lib.y3_net_read_tensor(net._h, stored[0], bad_batch, None, C_.byref(n), None) == _lib.Y3_ERR_INVALID
        if as_i8:
            assert net.lib.y3_net_read_tensor_i8(net._h, as_i8[0], bad_batch, None, C_.byref(n), None) == _lib.Y3_ERR_INVALID
    with pytest.raises(rt.Y3Error, match="can be read back at that batch only"):
        net.read_tensor(stored[0], B)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. guarded outputs of the network
FORWARD = [c for c in F.CASES if c.call == "y3_net_forward"]


@pytest.mark.parametrize("case", FORWARD, ids=_ids(FORWARD))
def test_forward_writes_all_of_its_grids_and_nothing_else(rt, case):
    """y3_net_forward into grids allocated for max_batch images between guards: the images of the call are written completely and equal
    the ordinary call's, the images behind the call's batch keep their poison, and so do both guards."""
    net, opts = _net(rt, case.net), dict(case.opts)
    x = F.images(case.net, case.canvas, case.max_batch)
    _plan(net, case.mode, case.canvas, case.max_batch, x=_cuda(x), tiny_stem=opts.get("tiny_stem"))
    if "tiny_stem" in opts:
        assert net.tiny_stem_fused == opts["tiny_stem"]
    xd = _feed(rt, case.mode, x)
    for lanes in case.lanes:
        net.set_lanes(lanes)
        for batch in case.batches:
            xb = xd[:batch].contiguous()
            ref = [g.clone() for g in net.forward(xb)]
            gs = [F.guarded(s, torch.float32) for s in F.grid_shapes(case, case.max_batch)]
            net.forward(xb, out=[g.tensor[:batch] for g in gs])
            torch.cuda.synchronize()
            for k, (g, r) in enumerate(zip(gs, ref)):
                what = f"{case.name} lanes {lanes} batch {batch} grid {k}"
                assert F.guards_intact(g), f"{what}: written outside the tensor"
                assert F.poison_words(g.tensor[:batch]) == 0, f"{what}: not all of the grid was written"
                assert F.same_bits(g.tensor[:batch], r), f"{what}: differs from the same call into an ordinary tensor"
                rest = g.tensor[batch:]
                assert F.poison_words(rest) == rest.numel(), f"{what}: images behind the call's batch were written"


DECODE = [c for c in F.CASES if c.call == "y3_net_forward_decode"]


@pytest.mark.parametrize("case", DECODE, ids=_ids(DECODE))
def test_forward_decode_writes_boxes_classes_scores_and_nothing_else(rt, case):
    net = _net(rt, case.net)
    x = F.images(case.net, case.canvas, case.max_batch)
    _plan(net, case.mode, case.canvas, case.max_batch, x=_cuda(x))
    a = F.anchors(case.net)
    ah = _anchors(a, reshape=True, scales=net.heads)
    for lanes in case.lanes:
        net.set_lanes(lanes)
        for batch in case.batches:
            xb = _cuda(x[:batch])
            ref = [t.clone() for t in net.forward_decode(xb, a)]
            gs = [F.guarded(s, TORCH_DTYPE[d]) for _, s, d in F.guarded_outputs(case)]
            _lib.check(net.lib.y3_net_forward_decode(net._h, _dev(xb), batch, _fptr(ah), *[_dev(g.tensor) for g in gs], _lib.stream_ptr()),
                     "y3_net_forward_decode")
            torch.cuda.synchronize()
            for (what, _, _), g, r in zip(F.guarded_outputs(case), gs, ref):
                _check(g, r, f"{case.name} lanes {lanes} {what}")


DETECT = [c for c in F.CASES if c.call in ("y3_net_detect", "y3_net_detect_grids")]


def _detect(net, call, xb, ah, packed, nv, grids):
    head = (net._h, _dev(xb), xb.shape[0], _fptr(ah), F.MAX_BOXES, F.IOU, F.SCORE)
    if call == "y3_net_detect":
        return net.lib.y3_net_detect(*head, _dev(packed), _dev(nv), _lib.stream_ptr())
    ptrs = (C_.c_void_p * len(grids))(*[g.data_ptr() for g in grids])
    return net.lib.y3_net_detect_grids(*head, ptrs, _dev(packed), _dev(nv), _lib.stream_ptr())


@pytest.mark.parametrize("case", DETECT, ids=_ids(DETECT))
def test_detect_writes_its_rows_counts_and_grids_and_nothing_else(rt, case):
    """packed: guards and equality with the unguarded call (its rows behind num_valid are zeros the call stores); num_valid and the
    three grids of y3_net_detect_grids: no poison left as well."""
    net, opts = _net(rt, case.net), dict(case.opts)
    x = F.images(case.net, case.canvas, case.max_batch)
    _plan(net, case.mode, case.canvas, case.max_batch, x=_cuda(x))
    ah = _anchors(F.anchors(case.net), reshape=True, scales=net.heads)
    (batch,) = case.batches
    xb = _cuda(x[:batch])
    try:
        net.nms_per_class = bool(opts["per_class"])
        net.multi_label = bool(opts.get("multi_label"))
        outs = F.guarded_outputs(case)
        ref = [torch.empty(s, dtype=TORCH_DTYPE[d], device="cuda") for _, s, d in outs]
        _lib.check(_detect(net, case.call, xb, ah, ref[0], ref[1], ref[2:]), case.call)
        torch.cuda.synchronize()
        gs = [F.guarded(s, TORCH_DTYPE[d]) for _, s, d in outs]
        _lib.check(_detect(net, case.call, xb, ah, gs[0].tensor, gs[1].tensor, [g.tensor for g in gs[2:]]), case.call)
        torch.cuda.synchronize()
    finally:
        net.nms_per_class = False
        net.multi_label = False
    for (what, _, _), g, r in zip(outs, gs, ref):
        _check(g, r, f"{case.name} {what}", written=what != "packed")
    assert int(ref[1].sum()) > 0, "no detection at all: the rows compared are all padding"


# ---------------------------------------------------------------------------------------------- 2. guarded outputs of stand-alone ops
@pytest.mark.parametrize("dtype", F.POOL_DTYPES)
@pytest.mark.parametrize("shape,stride", F.POOL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_maxpool_writes_its_output_and_nothing_else(rt, shape, stride, dtype):
    from tests.tiny_cases import pool_data
    from yolo_v3_tf2_amd import ops
    x = _cuda(pool_data(shape, "normal")).to(TORCH_DTYPE[dtype])
    ref = ops.maxpool2x2(x, stride)
    g = F.guarded((shape[0], shape[1] // stride, shape[2] // stride, shape[3]), TORCH_DTYPE[dtype])
    ops.maxpool2x2(x, stride, out=g.tensor)
    torch.cuda.synchronize()
    _check(g, ref, f"maxpool {shape} stride {stride} {dtype}")


@pytest.mark.parametrize("nc", F.DECODE_NC)
def test_decode_family_writes_its_outputs_and_nothing_else(rt, nc):
    """_decode_scores(out=), decode_candidates(out=, ws=), and through their C entries y3_class_scores and y3_pack_detections, whose
    wrappers allocate their outputs."""
    from yolo_v3_tf2_amd import ops
    grids = [_cuda(g) for g in F.decode_grids(nc)]
    a = F.anchors("yolov3_nc80").reshape(3, 3, 2)
    B, N = F.DECODE_BATCH, sum(3 * g * g for g in F.DECODE_GRIDS)
    shapes = (((B, N, 4), torch.float32), ((B, N), torch.int64), ((B, N), torch.float32))
    ref = ops._decode_scores(grids, a, nc)
    gs = [F.guarded(s, d) for s, d in shapes]
    ops._decode_scores(grids, a, nc, out=tuple(g.tensor for g in gs))
    torch.cuda.synchronize()
    for what, g, r in zip(("boxes", "cls", "scores"), gs, ref):
        _check(g, r, f"decode_scores nc {nc} {what}")
    boxes, cls, scores = ref

    K, thr = 40, 0.3
    cshapes = (((B, K, 4), torch.float32), ((B, K), torch.int64), ((B, K), torch.float32), ((B, K), torch.int32), ((B,), torch.int32))
    cref = ops.decode_candidates(grids, a, nc, thr, K)
    cg = [F.guarded(s, d) for s, d in cshapes]
    need = ops.decode_candidates_workspace_bytes([(g, g) for g in F.DECODE_GRIDS], B, nc)
    ws = F.guarded((need,), torch.uint8)
    ops.decode_candidates(grids, a, nc, thr, K, out=tuple(g.tensor for g in cg), ws=ws.tensor)
    torch.cuda.synchronize()
    assert F.guards_intact(ws), "decode_candidates: written outside its workspace"
    for what, g, r in zip(("cand_boxes", "cand_cls", "cand_scores", "cand_src", "totals"), cg, cref):
        _check(g, r, f"decode_candidates nc {nc} {what}")
    assert int(cref[4].min()) > 0, "no candidate at all: the rows compared are all padding"

    _, conf, probs = ops.yolo_decode(grids, a, nc)
    sref = ops.class_scores(conf, probs)
    sg = [F.guarded((B, N), torch.int64), F.guarded((B, N), torch.float32)]
    lib = _lib.load()
    _lib.check(lib.y3_class_scores(_dev(conf), _dev(probs), B, N, nc, _dev(sg[0].tensor), _dev(sg[1].tensor), _lib.stream_ptr()), "y3_class_scores")
    torch.cuda.synchronize()
    for what, g, r in zip(("cls", "scores"), sg, sref):
        _check(g, r, f"class_scores nc {nc} {what}")

    M = 20
    sel, nv = ops.nms_padded(boxes, scores, M, 0.5, 0.3)
    pref = ops.pack_detections(boxes, cls, scores, sel, nv)
    pg = F.guarded((B, M, 7), torch.int32)
    _lib.check(lib.y3_pack_detections(_dev(boxes), _dev(cls), _dev(scores), _dev(sel), _dev(nv), B, N, M, _dev(pg.tensor), _lib.stream_ptr()),
             "y3_pack_detections")
    torch.cuda.synchronize()
    _check(pg, pref, f"pack_detections nc {nc}")


# ---------------------------------------------------------------------------------------------- 3. arena tensors beyond the call's batch
def _readable(rt, net, tensors, batch, i8=False):
    """{tensor: its read-back} of those of `tensors` the plan holds (a tensor inside the fused tiny stem, or not held as int8, is not)."""
    out = {}
    for t in tensors:
        try:
            out[t] = (net.read_tensor_i8 if i8 else net.read_tensor)(t, batch).clone()
        except rt.Y3Error as e:
            assert "fused tiny stem" in str(e) or "not held as int8" in str(e), e
    return out


def _five_then_three(rt, net, mode, x1, x2, tensors, what):
    """Forward five images X1, snapshot every stored tensor at 5, forward three other images X2, read again at 5: images 3 and 4 equal the
    snapshot bit for bit (and images 0..2 changed).  The three images' grids equal the first three of a five-image forward of
    cat(X2, X1[3:]): batch independence of the bits, as tests/test_gpu_parity.py::test_full_size_batch_properties asserts it."""
    B, b = F.BEYOND_MAX_BATCH, F.BEYOND_BATCH
    net.forward(x1)
    snap = _readable(rt, net, tensors, B)
    snap8 = _readable(rt, net, tensors, B, i8=True) if mode == "i8" else {}
    assert snap and (mode != "i8" or snap8), what
    g3 = [g.clone() for g in net.forward(x2)]
    again = _readable(rt, net, tensors, B)
    again8 = _readable(rt, net, tensors, B, i8=True) if mode == "i8" else {}
    torch.cuda.synchronize()
    for before, after, kind in ((snap, again, "fp32 read"), (snap8, again8, "int8 read")):
        assert sorted(before) == sorted(after)
        if not before:      # the int8 reads of a plan that is not int8
            continue
        for t in before:
            assert F.same_bits(before[t][b:], after[t][b:]), f"{what}: a forward of {b} images wrote into images {b}.. of tensor {t} ({kind})"
        assert any(not F.same_bits(before[t][:b], after[t][:b]) for t in before), f"{what}: the second forward wrote nothing ({kind})"
    g5 = net.forward(torch.cat([x2, x1[b:]]).contiguous())
    torch.cuda.synchronize()
    for k, (a, c) in enumerate(zip(g3, g5)):
        assert F.same_bits(a, c[:b]), f"{what}: grid {k} of {b} images differs from the first {b} of {B}"


@pytest.mark.parametrize("key,mode", F.BEYOND_NETS, ids=[f"{k}_{m}" for k, m in F.BEYOND_NETS])
def test_a_smaller_batch_leaves_the_arena_images_behind_it_alone(rt, key, mode):
    from yolo_v3_tf2_amd.graph import AuxOp
    net = _net(rt, key)
    x = F.images(key, 96, F.BEYOND_MAX_BATCH + F.BEYOND_BATCH)
    # a 16-bit plan of YOLOv3-tiny exists with the fused stem only; the three tensors inside that launch are never stored
    _plan(net, mode, 96, F.BEYOND_MAX_BATCH, x=_cuda(x[:F.BEYOND_MAX_BATCH]), keep=True, tiny_stem=key.startswith("tiny") and mode != "f32")
    p = net.program
    tensors = sorted({o.dst for o in p.conv_ops() if o.dst not in p.outputs} | {o.dst for o in p.ops if isinstance(o, AuxOp)})
    _five_then_three(rt, net, mode, _cuda(x[:F.BEYOND_MAX_BATCH]), _cuda(x[F.BEYOND_MAX_BATCH:]), tensors, f"{key} {mode}")


@pytest.mark.parametrize("family,mode", F.BEYOND_STEMS, ids=[f"{f}_{m}" for f, m in F.BEYOND_STEMS])
def test_a_smaller_batch_leaves_the_fused_stems_destination_alone(rt, family, mode):
    """The fused stems step aside under keep_activations (YOLOv3's) or keep their inner tensors to themselves (tiny's): the programs of
    tests/persistent_cases.py on a plan without keep, whose stem destination stays alive to the last op."""
    from tests import persistent_cases as P
    from tests.tiny_stem_cases import stem_program
    kind = {"tiny": _lib.Y3_PERSISTENT_TINY_STEM, "stem": _lib.Y3_PERSISTENT_STEM_F32 if mode == "f32" else _lib.Y3_PERSISTENT_STEM_16}[family]
    B = F.BEYOND_MAX_BATCH + F.BEYOND_BATCH
    case = P.Case(f"footprint_{family}_{mode}", family, mode, kind, (64, 96), B, 4 if family == "tiny" else 2, (4, 8) if family == "tiny" else (8, 16), 1, None)
    p, w, x = P.inputs(case)
    net = rt.Net(p)
    net.load_weights(w)
    if family == "stem" and mode == "f16":
        net.set_stem_fusion_f16(2)
    _plan(net, mode, case.canvas, F.BEYOND_MAX_BATCH, tiny_stem=family == "tiny")
    xd = _cuda(x)
    if family == "tiny":
        assert net.tiny_stem_fused == 1
        dst = stem_program()[1]
    else:
        ms = net.profile_convs(xd[:1].contiguous())
        assert ms[0] == 0.0 and ms[1] > 0.0, "the fused stem did not engage"
        dst = p.conv_ops()[1].dst
    _five_then_three(rt, net, mode, xd[:F.BEYOND_MAX_BATCH].contiguous(), xd[F.BEYOND_MAX_BATCH:].contiguous(), [dst], case.name)
