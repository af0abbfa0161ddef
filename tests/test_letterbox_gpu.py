"""Letterboxed input on the GPU: the letterbox form of resize_kernel / preprocess_batch_kernel against each other and against
core/utils.resize_image (bit for bit), unletterbox_kernel against core/utils.unletterbox_boxes (bit for bit),
Net.detect_stream(letterbox=True) against the serial composition, and graph capture.  No tolerances anywhere: the kernels
perform the host restatement's fp32 operations in the same order, so every comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (h, w, S) -> (sh, sw, top, left): the geometry table of tests/test_letterbox_host.py
GEOMETRY_CASES = [
    ((50, 100, 64), (32, 64, 16, 0)), ((90, 30, 60), (60, 20, 0, 20)), ((5, 128, 64), (2, 64, 31, 0)),
    ((63, 128, 64), (32, 64, 16, 0)), ((1, 200, 64), (1, 64, 31, 0)), ((33, 64, 64), (33, 64, 15, 0)),
    ((23, 1, 64), (64, 3, 0, 30)), ((1080, 1920, 416), (234, 416, 91, 0)), ((128, 128, 64), (64, 64, 0, 0)),
]
# (H, W, C): the sources of that table, then a four-channel frame, a narrow one, an upscale, the identity at S = 64, one pixel
SHAPES = [(h, w, 3) for (h, w, _), _ in GEOMETRY_CASES] + [(667, 812, 4), (100, 37, 3), (10, 20, 3), (64, 64, 3), (1, 1, 4)]


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _image(rng, shape, mode):
    return rng.random(shape, dtype=np.float32) if mode == 0 else rng.integers(0, 256, shape, dtype=np.uint8)


def _mixed_images(seed):
    """Every shape in every mode (0: float32, 1: uint8 * 1/255 first, 2: uint8, / 255 last); the letterbox flag on every
    second image of the list, so that each shape meets the flag in some mode and one launch mixes both forms."""
    rng = np.random.default_rng(seed)
    images, modes = [], []
    for mode in (1, 0, 2):
        for shape in SHAPES:
            images.append(_image(rng, shape, mode))
            modes.append(mode)
        if mode != 2:      # an odd count per mode: an even one would give a shape the same flag in all three
            images.append(_image(rng, (37, 61, 3), mode))
            modes.append(mode)
    flags = [i % 2 == 1 for i in range(len(images))]
    return images, modes, flags


def _host_reference(img, mode, S, letterbox):
    """tests/test_input_stage_gpu.py::_host_reference with resize_image in the place of resize_bilinear where flagged"""
    from yolo_v3_tf2_amd.core.utils import resize_bilinear, resize_image
    resize = resize_image if letterbox else resize_bilinear
    rgb = img[..., :3]
    if mode == 0:
        return resize(rgb, S, S)
    if mode == 1:
        return resize(rgb.astype(np.float32) * np.float32(1.0 / 255.0), S, S)
    return resize(rgb.astype(np.float32), S, S) / np.float32(255)


def _per_image(rt, images, modes, flags, S, fill=0.0):
    """The serial route: one upload and one y3_preprocess_image per image."""
    batch = torch.full((len(images), S, S, 3), fill, device="cuda")
    for slot, (img, mode, lb) in enumerate(zip(images, modes, flags)):
        rt.preprocess_image(_cuda(img), batch, slot, divide_after=(mode == 2), letterbox=lb)
    return batch


@pytest.mark.parametrize("S", [64, 96, 51])
def test_letterbox_kernels_are_bit_exact(rt, S):
    """One preprocess_batch over 44 unlike images, every second one letterboxed, into slots that held 1.0 everywhere ==
    preprocess_image(letterbox=...) per image == resize_image / resize_bilinear on the host; the neighbouring slots keep
    their 1.0, so the padding was written (as zeros) and nothing beyond the slots was.  S = 51 has S*S % 4 != 0 and takes the
    scalar-store path; at 64 and 96 a thread's four pixels straddle the pad edge wherever left or left + sw is no multiple
    of four."""
    images, modes, flags = _mixed_images(S)
    seen = {}
    for img, mode, lb in zip(images, modes, flags):
        seen.setdefault(img.shape, set()).add(lb)
    assert all(v == {False, True} for v in seen.values()), "every shape must meet both forms"
    blob, descs = rt.pack_images(images, modes, letterbox=flags)
    first, n = 2, len(images)
    batch = torch.full((first + n + 1, S, S, 3), 1.0, device="cuda")
    rt.preprocess_batch(_cuda(blob), descs, batch, first_slot=first)
    want = _per_image(rt, images, modes, flags, S, fill=1.0).cpu().numpy()
    got = batch.cpu().numpy()
    assert (got[:first] == 1.0).all() and (got[first + n:] == 1.0).all(), "slots outside [first_slot, first_slot + n) were written"
    geoms = rt.letterbox_geometries(descs, S)
    padded = 0
    for i, (img, mode, lb) in enumerate(zip(images, modes, flags)):
        assert np.array_equal(got[first + i], want[i]), (i, img.shape, mode, lb, float(np.abs(got[first + i] - want[i]).max()))
        ref = _host_reference(img, mode, S, lb)
        assert np.array_equal(got[first + i], ref), (i, img.shape, mode, lb, geoms[i].tolist(), float(np.abs(got[first + i] - ref).max()))
        sh, sw, top, left = geoms[i].tolist()
        outside = np.ones((S, S), bool)
        outside[top:top + sh, left:left + sw] = False
        assert not got[first + i][outside].any(), (i, "padding is not zero")
        padded += int(outside.any())
    assert padded >= n // 3, "most flagged images must really have padding"


@pytest.mark.parametrize("S", [64, 51])
def test_square_sources_do_not_see_the_flag(rt, S):
    """A square source fills the canvas: with the flag it is bit-equal to the same source without it, in every mode."""
    rng = np.random.default_rng(5)
    shapes = [(128, 128, 3), (64, 64, 3), (1, 1, 4), (37, 37, 4), (200, 200, 3)]
    images = [_image(rng, s, m) for m in (1, 0, 2) for s in shapes]
    modes = [m for m in (1, 0, 2) for _ in shapes]
    blob, d_flag = rt.pack_images(images, modes, letterbox=True)
    _, d_plain = rt.pack_images(images, modes)
    assert (rt.letterbox_geometries(d_flag, S) == np.array([S, S, 0, 0])).all()
    blob_dev = _cuda(blob)
    a = torch.full((len(images), S, S, 3), 1.0, device="cuda")
    b = torch.full((len(images), S, S, 3), 1.0, device="cuda")
    rt.preprocess_batch(blob_dev, d_flag, a)
    rt.preprocess_batch(blob_dev, d_plain, b)
    assert torch.equal(a, b)
    assert torch.equal(a, _per_image(rt, images, modes, [True] * len(images), S))


def test_unaligned_batch_base_with_flagged_images(rt):
    """A batch whose base is not 16-byte aligned cannot take the vector stores; the values are the same."""
    S = 64
    images, modes, flags = _mixed_images(3)
    blob, descs = rt.pack_images(images, modes, letterbox=flags)
    n = len(images) * S * S * 3
    flat = torch.full((n + 4,), 1.0, device="cuda")
    batch = flat[1:1 + n].view(len(images), S, S, 3)
    assert batch.data_ptr() % 16 == 4 and batch.is_contiguous()
    rt.preprocess_batch(_cuda(blob), descs, batch)
    aligned = torch.full((len(images), S, S, 3), 1.0, device="cuda")
    assert aligned.data_ptr() % 16 == 0
    rt.preprocess_batch(_cuda(blob), descs, aligned)
    assert torch.equal(batch, aligned)
    assert torch.equal(batch, _per_image(rt, images, modes, flags, S))
    assert flat[0] == 1 and (flat[-3:] == 1).all()


def test_more_flagged_images_than_one_launch_holds(rt):
    """70 letterboxed tiny images: two launches inside one call == the same images issued as chunks of 50 == per image."""
    S = 64
    rng = np.random.default_rng(70)
    images = [rng.integers(0, 256, (int(rng.integers(1, 41)), int(rng.integers(1, 41)), int(rng.integers(3, 5))), dtype=np.uint8)
              for _ in range(70)]
    modes = [int(m) for m in rng.integers(1, 3, len(images))]
    blob, descs = rt.pack_images(images, modes, letterbox=True)
    blob_dev = _cuda(blob)
    one = torch.full((len(images) + 1, S, S, 3), 1.0, device="cuda")
    rt.preprocess_batch(blob_dev, descs, one, first_slot=1)
    chunks = torch.full_like(one, 1.0)
    for i0 in range(0, len(images), 50):
        rt.preprocess_batch(blob_dev, descs[i0:i0 + 50], chunks, first_slot=1 + i0)
    assert torch.equal(one, chunks)
    assert (one[0] == 1).all() and torch.equal(one[1:], _per_image(rt, images, modes, [True] * len(images), S))
    # the image behind the launch boundary got its own geometry, not image 0's
    g = rt.letterbox_geometries(descs, S)
    assert not np.array_equal(g[64], g[0])
    sh, sw, top, left = g[64].tolist()
    slot = one[65].cpu().numpy()
    outside = np.ones((S, S), bool)
    outside[top:top + sh, left:left + sw] = False
    assert outside.any() and not slot[outside].any() and slot[~outside].any()


def _packed_rows(rng, batch, M, nv):
    """Hand-made rows as y3_pack_detections leaves them: boxes (some outside [0,1]: nothing clips), score, class, index;
    rows >= num_valid zero."""
    packed = np.zeros((batch, M, 7), np.int32)
    boxes = (rng.random((batch, M, 4), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    packed[..., :4] = boxes.view(np.int32)
    packed[..., 4] = rng.random((batch, M), dtype=np.float32).view(np.int32)
    packed[..., 5] = rng.integers(0, 80, (batch, M))
    packed[..., 6] = rng.integers(0, 10647, (batch, M))
    for b in range(batch):
        packed[b, nv[b]:] = 0
    return packed


def test_unletterbox_detections_alone(rt):
    """70 images (two launches) x 5 hand-made rows, num_valid from {0, 1, 3, 5}, the geometries of the host test's table (one
    call per image size they belong to) plus whole-canvas images at S = 416, on a view of a buffer with one more image on
    either side: bit-equal to unletterbox_boxes on the valid rows; score, class and index words, rows >= num_valid,
    whole-canvas images and the images around the view are what they were."""
    from yolo_v3_tf2_amd.core.utils import unletterbox_boxes
    B, M = 70, 5
    rng = np.random.default_rng(17)
    by_size = {}
    for (_, _, S), g in GEOMETRY_CASES:
        by_size.setdefault(S, []).append(g)
    by_size[416].append((416, 416, 0, 0))
    assert sorted(by_size) == [60, 64, 416]
    for S, table in sorted(by_size.items()):
        geoms = np.array([table[int(i)] for i in rng.integers(0, len(table), B)], np.int32)
        if S == 416:
            geoms[[0, 63, 64, 69]] = (416, 416, 0, 0)
            geoms[[1, 65]] = (234, 416, 91, 0)
        nv = rng.choice(np.array([0, 1, 3, 5], np.int32), B).astype(np.int32)
        nv[:4], nv[64:68] = [0, 1, 3, 5], [5, 3, 1, 0]
        before = _packed_rows(rng, B + 2, M, np.concatenate([[5], nv, [5]]))
        buf = _cuda(before)
        view = buf[1:B + 1]
        out = rt.unletterbox_detections(view, _cuda(nv), geoms, S)
        assert out.data_ptr() == view.data_ptr()
        got = buf.cpu().numpy()
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[-1], before[-1]), "rows outside the view were written"
        got, src = got[1:-1], before[1:-1]
        assert np.array_equal(got[..., 4:], src[..., 4:]), "score, class and index words changed"
        moved = 0
        for b in range(B):
            n = int(nv[b])
            assert not got[b, n:].any(), (S, b, "rows >= num_valid must stay zero")
            want = unletterbox_boxes(src[b, :n, :4].copy().view(np.float32), geoms[b], S)
            assert np.array_equal(got[b, :n, :4], want.view(np.int32)), (S, b, geoms[b].tolist(), n)
            if tuple(geoms[b]) == (S, S, 0, 0):
                assert np.array_equal(got[b], src[b]), (S, b, "a whole-canvas image must not be touched")
            elif n:
                moved += int(not np.array_equal(got[b, :n, :4], src[b, :n, :4]))
        assert moved >= 10, (S, moved)


def test_unletterbox_device_call_refuses_bad_arguments(rt):
    packed = torch.zeros((2, 5, 7), dtype=torch.int32, device="cuda")
    nv = torch.zeros((2,), dtype=torch.int32, device="cuda")
    g = np.array([[32, 64, 16, 0], [64, 64, 0, 0]], np.int32)
    for args in ((packed.cpu(), nv, g, 64), (packed, nv[:1], g, 64), (packed, nv, g[:1], 64), (packed.float(), nv, g, 64),
                 (packed, nv, np.array([[32, 64, 16, 0], [64, 64, 1, 0]], np.int32), 64)):
        with pytest.raises(rt.Y3Error):
            rt.unletterbox_detections(*args)


# Net.detect_stream(letterbox=True) at S = 160; the score threshold and what the CPU oracle counts at it: see the test's docstring
STREAM_S, STREAM_THRESHOLD = 160, 0.05
STREAM_SHAPES = [(480, 640, 3), (100, 37, 3), (300, 400, 4), (160, 160, 3)]


def stream_batches():
    """Batches of 4, 4 and 3 uint8 frames over the four shapes (the second batch in another order)."""
    rng = np.random.default_rng(160)
    order = [[0, 1, 2, 3], [3, 2, 1, 0], [0, 1, 2]]
    return [[rng.integers(0, 256, STREAM_SHAPES[k], dtype=np.uint8) for k in ks] for ks in order]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_detect_stream_letterbox_equals_the_serial_composition(rt, program, weights, anchors, mode):
    """detect_stream(letterbox=True) over batches of 4, 4 and 3 frames == preprocess_image(letterbox=True) per slot ->
    Net.detect -> unletterbox_detections on the same net, in submission order; detect_stream(letterbox=False) == the serial
    route it was equal to before the flag existed.
    Score threshold 0.05, the one tests/test_input_stage_gpu.py uses; no other value had to be tried.  On the CPU the oracle
    (oracle.forward / yolo_decode / yolo_nms over core/utils.resize_image of stream_batches(), synthetic weights seed 4321,
    100 boxes, IoU 0.5) counts at it
      fp32        num_valid [[95, 44, 93, 100], [100, 89, 48, 92], [92, 43, 97]]   (best score per batch 0.266, 0.258, 0.189)
      bf16=True   num_valid [[94, 44, 95, 100], [100, 91, 47, 91], [96, 44, 97]]
    so every image of every batch has valid rows to move, and most have zero rows behind them that must stay zero."""
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry, unletterbox_boxes
    S, T = STREAM_S, STREAM_THRESHOLD
    batches = stream_batches()
    assert [len(b) for b in batches] == [4, 4, 3]
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[mode])
    want, want_plain, canvas = [], [], []
    for b in batches:
        geoms = np.stack([letterbox_geometry(im.shape[0], im.shape[1], S, S) for im in b])
        packed, nv = net.detect(_per_image(rt, b, [1] * len(b), [True] * len(b), S), anchors, 100, 0.5, T)
        canvas.append(packed.cpu().numpy())
        rt.unletterbox_detections(packed, nv, geoms, S)
        want.append((packed.cpu().numpy(), nv.cpu().numpy(), geoms))
        packed, nv = net.detect(_per_image(rt, b, [1] * len(b), [False] * len(b), S), anchors, 100, 0.5, T)
        want_plain.append((packed.cpu().numpy(), nv.cpu().numpy()))
    print("num_valid per batch:", [w[1].tolist() for w in want])
    got = list(net.detect_stream(batches, anchors, 100, 0.5, T, mode=1, depth=2, letterbox=True))
    assert len(got) == len(batches)
    for i, ((gp, gn), (wp, wn, geoms)) in enumerate(zip(got, want)):
        assert isinstance(gp, np.ndarray) and gp.shape == (len(batches[i]), 100, 7) and gn.shape == (len(batches[i]),)
        assert (wn > 0).any(), (i, "no valid row in this batch: the coordinate path is not exercised")
        assert np.array_equal(gn, wn), (i, gn, wn)
        assert np.array_equal(gp, wp), i
        # ... and the serial composition itself moved the boxes as the host restatement does
        for k in range(len(batches[i])):
            n = int(wn[k])
            moved = unletterbox_boxes(canvas[i][k, :n, :4].copy().view(np.float32), geoms[k], S)
            assert np.array_equal(wp[k, :n, :4], moved.view(np.int32)), (i, k)
        padded = [k for k in range(len(batches[i])) if tuple(geoms[k]) != (S, S, 0, 0) and wn[k] > 0]
        assert padded and all(not np.array_equal(wp[k], canvas[i][k]) for k in padded), i
    assert not np.array_equal(want[0][0], want[1][0]), "the batches must differ for the order to mean anything"
    plain = list(net.detect_stream(batches, anchors, 100, 0.5, T, mode=1, depth=2))
    again = list(net.detect_stream(batches, anchors, 100, 0.5, T, mode=1, depth=2, letterbox=False))
    for i, (p, a, (wp, wn)) in enumerate(zip(plain, again, want_plain)):
        assert np.array_equal(p[1], wn) and np.array_equal(p[0], wp), i
        assert np.array_equal(a[1], wn) and np.array_equal(a[0], wp), i


def test_staged_batch_carries_the_geometry(rt):
    S = 64
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(50, 100, 3), (90, 30, 4), (64, 64, 3)]]
    stage = rt.InputStage(S, 3, rt.packed_nbytes(frames), depth=2)
    h = stage.submit(frames, 1, letterbox=[True, False, True])
    assert h.geometry.dtype == np.int32 and h.geometry.tolist() == [[32, 64, 16, 0], [64, 64, 0, 0], [64, 64, 0, 0]]
    torch.cuda.current_stream().wait_event(h.ready)
    got = h.batch.clone()
    stage.release(h)
    h2 = stage.submit(frames, 1)
    assert h2.geometry.tolist() == [[64, 64, 0, 0]] * 3
    stage.release(h2)
    torch.cuda.synchronize()
    assert torch.equal(got, _per_image(rt, frames, [1] * 3, [True, False, True], S))


def test_letterbox_detect_and_unletterbox_in_one_graph(rt, program, weights, anchors):
    """preprocess_batch (flagged) + Net.detect + unletterbox_detections captured into one graph; each replay, after new pixel
    values of the same shapes were copied into the device blob, equals the eager result.  (Descriptors and geometries are
    frozen into the graph.)"""
    S, shapes = 160, [(480, 640, 3), (100, 37, 4), (200, 150, 3)]
    rng = np.random.default_rng(9)

    def frames():
        return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]

    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(len(shapes), S)
    blob, descs = rt.pack_images(frames(), 1, letterbox=True)
    geoms = rt.letterbox_geometries(descs, S)
    assert geoms.tolist() == [[120, 160, 20, 0], [160, 59, 0, 50], [160, 120, 0, 20]]
    blob_dev = _cuda(blob)
    batch = torch.zeros((len(shapes), S, S, 3), device="cuda")

    def step():
        rt.preprocess_batch(blob_dev, descs, batch)
        packed, nv = net.detect(batch, anchors, 100, 0.5, 0.05)
        return rt.unletterbox_detections(packed, nv, geoms, S), nv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = step()
    seen = []
    for _ in range(2):
        new = frames()
        blob2, descs2 = rt.pack_images(new, 1, letterbox=True)
        assert np.array_equal(descs2, descs)
        ep, en = net.detect(_per_image(rt, new, [1] * len(new), [True] * len(new), S), anchors, 100, 0.5, 0.05)
        on_canvas = ep.clone()
        rt.unletterbox_detections(ep, en, geoms, S)
        assert (en > 0).any() and not torch.equal(ep, on_canvas)
        blob_dev.copy_(torch.from_numpy(blob2))
        gp.zero_()
        gn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gn, en) and torch.equal(gp, ep)
        seen.append(ep.clone())
    assert not torch.equal(seen[0], seen[1]), "the two replays must see different pixels"
