"""Rectangular network input on the GPU: a net planned for an H x W canvas (y3_net_plan_hw) through every layer -- the decode of
gh x gw grids, the conv stack against the oracle, the fused routes against the composed ones, the input stage and the
unletterbox kernel against their host restatements, detect_stream / evaluate_stream -- and the square plan made through the
pair, bit for bit against the square plan made through the int.  Sizes are the smallest at which a row / column mix-up
cannot hide: gh != gw in both orientations, odd grids (3, 5) on one side."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _net(rt, program, weights, B, size, dtype=None, lanes=None, stem=None):
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, size, dtype)
    if lanes is not None:
        net.set_lanes(lanes)
    if stem is not None:
        net.set_stem_fusion(stem)
    return net


# ---------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("gs,B,nc", [(((2, 3), (4, 6), (8, 12)), 3, 7), (((3, 2), (6, 4), (12, 8)), 2, 80)])
def test_decode_rect_grids_match_the_host_restatement(rt, anchors, gs, B, nc):
    """yolo_decode / yolo_decode_scores on gh x gw grids against core/yolo_decode_layer.yolo_decode_hw_host within 2e-6 x
    scale (the bar of test_decode_matches_oracle: device expf against a host exp); shapes and order exact; decode_scores ==
    decode followed by class_scores, bit for bit."""
    from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
    rng = np.random.default_rng(21)
    grids = [rng.normal(0, 1.5, (B, gh, gw, 3, 5 + nc)).astype(np.float32) for gh, gw in gs]
    hb, hc, hp = yolo_decode_hw_host(grids, anchors, nc)
    dev = [_cuda(g) for g in grids]
    gb, gc, gp = rt.yolo_decode(dev, anchors, nc)
    sb, scls, ssc = rt.yolo_decode_scores(dev, anchors, nc)
    torch.cuda.synchronize()
    N = 3 * sum(gh * gw for gh, gw in gs)
    assert tuple(gb.shape) == hb.shape == (B, N, 4) and tuple(gc.shape) == hc.shape and tuple(gp.shape) == hp.shape
    scale = max(1.0, float(np.abs(hb).max()))
    print(gs, float(np.abs(gb.cpu().numpy() - hb).max()) / scale, float(np.abs(gc.cpu().numpy() - hc).max()),
          float(np.abs(gp.cpu().numpy() - hp).max()))
    assert np.abs(gb.cpu().numpy() - hb).max() <= 2e-6 * scale
    assert np.abs(gc.cpu().numpy() - hc).max() <= 2e-6 and np.abs(gp.cpu().numpy() - hp).max() <= 2e-6
    # a row / column mix-up moves a centre by at least 1 / max(gh, gw) of the canvas: far outside the bound above
    cls2, s2 = rt.class_scores(gc, gp)
    assert torch.equal(sb, gb) and torch.equal(scls, cls2) and torch.equal(ssc, s2)


def test_decode_square_pairs_are_the_square_call(rt, anchors):
    """(g, g) grids through y3_yolo_decode_hw / _scores_hw == y3_yolo_decode / _scores.  Both run the one shared body, so this
    catches a wrapper mistake only (a wrong {g, g} expansion, a swapped pointer); that square results are what they always
    were is guarded by the existing oracle parity suite (tests/test_gpu_parity.py::test_decode_matches_oracle and the
    network / detect tests), which runs through the generalised code."""
    import ctypes as C
    from yolo_v3_tf2_amd import _lib
    rng = np.random.default_rng(22)
    gs, B, nc = (2, 4, 8), 3, 7
    grids = [_cuda(rng.normal(0, 1.5, (B, g, g, 3, 5 + nc)).astype(np.float32)) for g in gs]
    nb, nconf, nprobs = rt.yolo_decode(grids, anchors, nc)
    sb, scls, ssc = rt.yolo_decode_scores(grids, anchors, nc)
    N = 3 * sum(g * g for g in gs)
    lib = _lib.load()
    ptrs = (C.c_void_p * 3)(*[g.data_ptr() for g in grids])
    sizes = (C.c_int32 * 3)(*gs)
    a = np.ascontiguousarray(anchors, np.float32)
    ap = a.ctypes.data_as(C.POINTER(C.c_float))
    ob, oconf, oprobs = torch.empty((B, N, 4), device="cuda"), torch.empty((B, N, 1), device="cuda"), torch.empty((B, N, nc), device="cuda")
    _lib.check(lib.y3_yolo_decode(ptrs, sizes, B, nc, ap, C.c_void_p(ob.data_ptr()), C.c_void_p(oconf.data_ptr()),
                                  C.c_void_p(oprobs.data_ptr()), _lib.stream_ptr()))
    ob2, ocls = torch.empty((B, N, 4), device="cuda"), torch.empty((B, N), dtype=torch.int64, device="cuda")
    osc = torch.empty((B, N), device="cuda")
    _lib.check(lib.y3_yolo_decode_scores(ptrs, sizes, B, nc, ap, C.c_void_p(ob2.data_ptr()), C.c_void_p(ocls.data_ptr()),
                                         C.c_void_p(osc.data_ptr()), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(nb, ob) and torch.equal(nconf, oconf) and torch.equal(nprobs, oprobs)
    assert torch.equal(sb, ob2) and torch.equal(scls, ocls) and torch.equal(ssc, osc)


# --------------------------------------------------------------------------------------------------------------- network
@pytest.fixture(scope="module")
def oracle_grids(program, weights):
    """oracle.forward (shape-generic) once per canvas; shared and left unchanged."""
    from oracle import oracle as O
    out = {}
    for (H, W), B in (((64, 96), 2), ((96, 64), 2), ((96, 160), 1)):
        x = np.random.default_rng(1234 + H).random((B, H, W, 3), dtype=np.float32)
        out[(H, W)] = (x, O.forward(program, weights, x))
    return out


@pytest.mark.parametrize("canvas", [(64, 96), (96, 64), (96, 160)])
def test_rect_network_grids_match_oracle(rt, program, weights, oracle_grids, canvas):
    """The full 75-conv forward on an H x W canvas, fp32, within 1e-4 absolute of the oracle (the bar of
    test_network_grids_match_oracle), fused stem on (the default) and off; the two forms within the bound
    test_fused_stem_matches_oracle_and_the_two_launch_form uses; the fused stem really ran on the rectangular plan."""
    x, ref = oracle_grids[canvas]
    B, (H, W) = x.shape[0], canvas
    xd = _cuda(x)
    outs = {}
    for fused in (1, 0):
        net = _net(rt, program, weights, B, canvas, stem=fused)
        assert net.grid_sizes() == [(H // 32, W // 32), (H // 16, W // 16), (H // 8, W // 8)]
        got = net.forward(xd)
        ms = net.profile_convs(xd)
        assert (ms[0] == 0.0) == bool(fused) and (ms[2] == 0.0) == bool(fused), "stem fusion did not follow the switch"
        for r, g, (gh, gw) in zip(ref, got, net.grid_sizes()):
            assert tuple(g.shape) == (B, gh, gw, 3, 85) == r.shape
            err = float(np.abs(g.cpu().numpy() - r).max())
            print(canvas, "fused" if fused else "unfused", err)
            assert err <= 1e-4
        outs[fused] = [g.clone() for g in got]
        assert abs(net.flops_per_image() - program.flops_per_image(canvas)) <= 1e-6 * program.flops_per_image(canvas)
    for a, b in zip(outs[1], outs[0]):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))


def test_rect_network_bf16_holds_the_free_running_bar(rt, program, weights, oracle_grids):
    """bf16 plan at (64, 96): relative norm against oracle.forward(bf16=True) below 1.5e-2, the bar tests/test_gpu_parity.py
    uses for the free-running bf16 network."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd import _lib
    x, _ = oracle_grids[(64, 96)]
    ref = O.forward(program, weights, x, bf16=True)
    net = _net(rt, program, weights, 2, (64, 96), _lib.Y3_DTYPE_BF16)
    got = net.forward(_cuda(x))
    rel = max(float(np.linalg.norm(g.cpu().numpy() - r) / np.linalg.norm(r)) for g, r in zip(got, ref))
    print("bf16 rel", rel)
    assert rel < 1.5e-2


def test_plan_hw_refuses_bad_sides_by_name(rt, program, weights):
    net = rt.Net(program)
    for bad in ((64, 100), (72, 96), (0, 96)):
        with pytest.raises(rt.Y3Error, match="y3_net_plan"):
            net.plan(1, bad)
    with pytest.raises(rt.Y3Error, match="64 x 100 .* not divisible by"):
        net.plan(1, (64, 100))


# ---------------------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("lanes", [1, 2])
def test_rect_routes_are_bit_identical(rt, program, weights, anchors, mode, lanes):
    """(64, 96), B = 3: net.detect == forward -> yolo_decode_scores -> nms_padded -> pack_detections; forward_decode (the head
    convs decoding their own tiles) == the composed route; oracle.nms_padded on the device's own boxes and scores gives the
    same indices and counts."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd import _lib
    canvas, B = (64, 96), 3
    a = rt.rect_anchors(anchors, 96, canvas)
    x = _cuda(np.random.default_rng(31).random((B, *canvas, 3), dtype=np.float32))
    net = _net(rt, program, weights, B, canvas, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[mode], lanes=lanes)
    grids = net.forward(x)
    bb, cc, ss = rt.yolo_decode_scores(grids, a, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    fb, fc, fs = net.forward_decode(x, a)
    assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
    for _ in range(2):     # the second call reuses the scratch
        packed, nv2 = net.detect(x, a, 100, 0.5, 0.05)
        torch.cuda.synchronize()
        assert torch.equal(nv2, nv) and torch.equal(packed, want) and int(nv.sum()) > 0
    rs, rn = O.nms_padded(bb.cpu().numpy(), ss.cpu().numpy(), 100, 0.5, 0.05)
    assert np.array_equal(rs, sel.cpu().numpy()) and np.array_equal(rn, nv.cpu().numpy())


def test_square_plan_through_the_pair_is_the_square_plan(rt, program, weights, anchors):
    """plan(b, (96, 96)) against plan(b, 96): grids, detect output and preprocess_batch output bit-identical; grid_sizes gives
    pairs for the pair and what it always gave for the int."""
    B = 3
    rng = np.random.default_rng(41)
    x = _cuda(rng.random((B, 96, 96, 3), dtype=np.float32))
    n_int, n_pair = _net(rt, program, weights, B, 96), _net(rt, program, weights, B, (96, 96))
    assert n_int.grid_sizes() == [3, 6, 12] and n_pair.grid_sizes() == [(3, 3), (6, 6), (12, 12)]
    assert n_int.flops_per_image() == n_pair.flops_per_image()
    for a, b in zip(n_int.forward(x), n_pair.forward(x)):
        assert torch.equal(a, b)
    (pa, na), (pb, nb) = n_int.detect(x, anchors, 100, 0.5, 0.05), n_pair.detect(x, anchors, 100, 0.5, 0.05)
    assert torch.equal(pa, pb) and torch.equal(na, nb) and int(na.sum()) > 0
    assert n_pair.max_batch == B and n_pair.canvas == (96, 96)       # a square batch did not re-plan the pair plan
    # an automatic re-plan (a larger batch) keeps the form of the caller's plan: pairs stay pairs, ints stay ints
    x5 = _cuda(rng.random((B + 2, 96, 96, 3), dtype=np.float32))
    for u, v in zip(n_int.forward(x5), n_pair.forward(x5)):
        assert torch.equal(u, v)
    assert n_pair.max_batch == B + 2 and n_pair.grid_sizes() == [(3, 3), (6, 6), (12, 12)] and n_int.grid_sizes() == [3, 6, 12]
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((100, 37, 3), (37, 100, 4), (1, 1, 3), (96, 96, 3))]
    blob, descs = rt.pack_images(imgs, 1, letterbox=[True, False, True, False])
    assert np.array_equal(rt.letterbox_geometries(descs, 96), rt.letterbox_geometries(descs, (96, 96)))
    import ctypes as C
    from yolo_v3_tf2_amd import _lib
    blob_dev = _cuda(blob)
    new = rt.preprocess_batch(blob_dev, descs, torch.full((4, 96, 96, 3), 7.0, device="cuda"))
    old = torch.full((4, 96, 96, 3), 7.0, device="cuda")
    d = np.ascontiguousarray(descs)
    _lib.check(_lib.load().y3_preprocess_batch(C.c_void_p(blob_dev.data_ptr()), blob_dev.numel(), d.ctypes.data_as(C.POINTER(_lib.ImageDesc)),
                                               len(d), C.c_void_p(old.data_ptr()), 0, 96, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(new, old)


# ----------------------------------------------------------------------------------------------------------- input stage
RAGGED = [(1, 1, 3), (100, 37, 3), (37, 100, 3), (48, 64, 4), (64, 96, 3), (96, 64, 3), (200, 11, 3), (23, 61, 4)]


def _host_reference(img, mode, canvas, letterbox):
    from yolo_v3_tf2_amd.core.utils import resize_bilinear, resize_image
    resize = resize_image if letterbox else resize_bilinear
    rgb = img[..., :3]
    if mode == 0:
        return resize(rgb, *canvas)
    if mode == 1:
        return resize(rgb.astype(np.float32) * np.float32(1.0 / 255.0), *canvas)
    return resize(rgb.astype(np.float32), *canvas) / np.float32(255)


@pytest.mark.parametrize("canvas", [(64, 96), (96, 64)])
def test_rect_preprocess_is_bit_exact(rt, canvas):
    """preprocess_batch onto an H x W canvas over ragged frames (1x1, 100x37, 37x100, four channels, the canvas itself and its
    transpose), all three modes, with and without the letterbox flag, into slots that held 1.0: == the NumPy restatement ==
    preprocess_image per image; the slot after the last keeps its 1.0."""
    rng = np.random.default_rng(51)
    images, modes, flags = [], [], []
    for mode in (1, 0, 2):
        for i, shape in enumerate(RAGGED):
            for lb in (False, True):
                images.append(rng.random(shape, dtype=np.float32) if mode == 0 else rng.integers(0, 256, shape, dtype=np.uint8))
                modes.append(mode)
                flags.append(lb)
    n = len(images)
    blob, descs = rt.pack_images(images, modes, letterbox=flags)
    batch = torch.full((n + 1, *canvas, 3), 1.0, device="cuda")
    rt.preprocess_batch(_cuda(blob), descs, batch)
    single = torch.full((n + 1, *canvas, 3), 1.0, device="cuda")
    for slot, (img, mode, lb) in enumerate(zip(images, modes, flags)):
        rt.preprocess_image(_cuda(img), single, slot, divide_after=(mode == 2), letterbox=lb)
    torch.cuda.synchronize()
    assert torch.equal(batch, single) and bool((batch[n] == 1.0).all())
    got = batch.cpu().numpy()
    for slot, (img, mode, lb) in enumerate(zip(images, modes, flags)):
        assert np.array_equal(got[slot], _host_reference(img, mode, canvas, lb)), (slot, img.shape, mode, lb)
    geoms = rt.letterbox_geometries(descs, canvas)
    lb_rows = geoms[np.array(flags)]
    assert (lb_rows[:, 0] < canvas[0]).any() and (lb_rows[:, 1] < canvas[1]).any(), "bars on both axes are in the set"


@pytest.mark.parametrize("canvas", [(64, 96), (96, 64)])
def test_rect_unletterbox_is_bit_exact(rt, canvas):
    """unletterbox_detections on an H x W canvas == x' = (x * W - left) / sw, y' = (y * H - top) / sh in fp32, each operation
    rounded on its own; rows behind num_valid, the other words and a whole-canvas image are not touched."""
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry, unletterbox_boxes
    rng = np.random.default_rng(61)
    shapes = [(100, 37), (37, 100), (1, 1), canvas, (480, 640), (640, 480)]
    geoms = np.stack([letterbox_geometry(h, w, *canvas) for h, w in shapes])
    geoms[3] = (canvas[0], canvas[1], 0, 0)
    B, M = len(shapes), 20
    rows = rng.integers(0, 2 ** 31 - 1, (B, M, 7)).astype(np.int32)
    rows[..., :4] = rng.random((B, M, 4), dtype=np.float32).view(np.int32)
    nv = np.array([20, 7, 0, 20, 13, 1], np.int32)
    packed = _cuda(rows)
    rt.unletterbox_detections(packed, _cuda(nv), geoms, canvas)
    got = packed.cpu().numpy()
    want = rows.copy()
    for b in range(B):
        want[b, :nv[b], :4] = unletterbox_boxes(rows[b, :nv[b], :4].view(np.float32), geoms[b], canvas).view(np.int32)
    assert np.array_equal(got, want)
    assert np.array_equal(got[3], rows[3]) and not np.array_equal(got[0, :20, :4], rows[0, :20, :4])
    with pytest.raises(rt.Y3Error, match="does not lie inside"):
        rt.unletterbox_detections(packed, _cuda(nv), geoms, canvas[::-1])      # the geometries of the other orientation do not fit


def _stream_frames(seed, counts=(4, 4, 3)):
    rng = np.random.default_rng(seed)
    shapes = [(48, 64, 3), (100, 37, 3), (37, 100, 4), (64, 96, 3), (90, 160, 3), (1, 1, 3), (120, 90, 3), (33, 200, 3)]
    out, k = [], 0
    for n in counts:
        out.append([rng.integers(0, 256, shapes[(k + i) % len(shapes)], dtype=np.uint8) for i in range(n)])
        k += n
    return out


def _serial_detect(rt, net, frames, a, canvas, thr, letterbox):
    batch = torch.zeros((len(frames), *canvas, 3), device="cuda")
    for slot, img in enumerate(frames):
        rt.preprocess_image(_cuda(img), batch, slot, letterbox=letterbox)
    packed, nv = net.detect(batch, a, 100, 0.5, thr)
    if letterbox:
        _, descs = rt.pack_images(frames, 1, letterbox=True)
        rt.unletterbox_detections(packed, nv, rt.letterbox_geometries(descs, canvas), canvas)
    return packed.cpu().numpy(), nv.cpu().numpy()


@pytest.mark.parametrize("letterbox", [True, False])
def test_rect_detect_stream_equals_the_serial_route_and_a_captured_batch(rt, program, weights, anchors, letterbox):
    """detect_stream on a (64, 96) plan over batches of 4, 4 and 3 ragged frames == per-image preprocess + detect
    (+ unletterbox) batch by batch, bit for bit; and one batch of it captured into a HIP graph (preprocess_batch, detect,
    unletterbox) and replayed gives the same rows."""
    canvas = (64, 96)
    a = rt.rect_anchors(anchors, 96, canvas)
    net = _net(rt, program, weights, 4, canvas)
    batches = _stream_frames(71)
    want = [_serial_detect(rt, net, b, a, canvas, 0.05, letterbox) for b in batches]
    got = list(net.detect_stream(batches, a, 100, 0.5, 0.05, letterbox=letterbox))
    assert len(got) == len(want) and net.canvas == canvas and net.max_batch == 4
    for (gp, gn), (wp, wn) in zip(got, want):
        assert np.array_equal(gn, wn) and np.array_equal(gp, wp)
    assert sum(int(n.sum()) for _, n in got) > 0
    if not letterbox:
        return
    frames = batches[0]
    blob, descs = rt.pack_images(frames, 1, letterbox=True)
    geoms, blob_dev = rt.letterbox_geometries(descs, canvas), _cuda(blob)
    batch = torch.zeros((4, *canvas, 3), device="cuda")

    def step():
        rt.preprocess_batch(blob_dev, descs, batch)
        packed, nv = net.detect(batch, a, 100, 0.5, 0.05)
        rt.unletterbox_detections(packed, nv, geoms, canvas)
        return packed, nv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = step()
    gp.zero_()
    gn.zero_()
    batch.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(gp.cpu().numpy(), want[0][0]) and np.array_equal(gn.cpu().numpy(), want[0][1])


def test_rect_evaluate_stream_equals_sweep_counters(rt, program, weights, anchors):
    """evaluate_stream(letterbox=True) on a (64, 96) plan == sweep_counters fed the same stream's detections (the rows
    detect_stream yields at the lowest threshold) and the same ground truth; loss=True on the non-square plan is refused."""
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    canvas, thresholds = (64, 96), [0.05, 0.1, 0.15, 0.3]
    a = rt.rect_anchors(anchors, 96, canvas)
    net = _net(rt, program, weights, 4, canvas)
    batches = _stream_frames(81)
    dets = list(net.detect_stream(batches, a, 100, 0.5, min(thresholds), letterbox=True))
    rng = np.random.default_rng(82)
    gts = []
    for packed, nv in dets:
        gt = []
        for b in range(len(packed)):
            rows = np.arange(0, int(nv[b]), 4)[:6]
            boxes = packed[b, rows, :4].copy().view(np.float32)
            classes = packed[b, rows, 5].copy()
            classes[1::3] = (classes[1::3] + 1) % 80
            c, s = rng.uniform(0.2, 0.8, (2, 2)), rng.uniform(0.1, 0.3, (2, 2))
            boxes = np.concatenate([boxes, np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)])
            gt.append((boxes, np.concatenate([classes, rng.integers(0, 80, 2).astype(np.int32)]).astype(np.int32)))
        gts.append(gt)
    want = np.zeros((len(thresholds), 5 * 80 + 2), np.int64)
    for (packed, nv), gt in zip(dets, gts):
        want += sweep_counters(packed, nv, *rt.pack_ground_truth(gt), 80, 0.5, thresholds)
    got = net.evaluate_stream(batches, gts, a, 100, 0.5, thresholds, 80, letterbox=True)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert want[0, 2 * 80:3 * 80].sum() > 0 and want[0, 3 * 80:4 * 80].sum() > 0 and want[0, -1] == 11      # tp, fp, examples
    with pytest.raises(ValueError):
        net.evaluate_stream(batches, gts, a, 100, 0.5, thresholds, 80, loss=True)
