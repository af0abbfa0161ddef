"""Batched input stage on the GPU: preprocess_batch_kernel against the per-image kernel and the NumPy restatement (bit for
bit), the InputStage ring, Net.detect_stream against the serial route, and graph capture.  No tolerances anywhere: the
batched stage performs the per-image stage's fp32 operations in the same order, so every comparison is np.array_equal."""
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


# (H, W, C): the shapes of test_preprocess_matches_host_restatement and test_preprocess_divide_after_... in
# tests/test_gpu_parity.py, then a single pixel, single rows / columns, and images smaller than every S (an upscale)
SHAPES = [(667, 812, 4), (100, 37, 3), (32, 32, 3), (1080, 1920, 3), (37, 61, 3), (128, 128, 3), (500, 375, 3),
          (1, 1, 3), (1, 1, 4), (1, 50, 3), (23, 1, 4), (8, 8, 3), (20, 13, 4)]


def _mixed_images(seed):
    """Every shape in every mode (0: float32, 1: uint8 * 1/255 first, 2: uint8, / 255 last), interleaved."""
    rng = np.random.default_rng(seed)
    images, modes = [], []
    for shape in SHAPES:
        for mode in (1, 0, 2):
            images.append(rng.random(shape, dtype=np.float32) if mode == 0 else rng.integers(0, 256, shape, dtype=np.uint8))
            modes.append(mode)
    return images, modes


def _host_reference(img, mode, S):
    from yolo_v3_tf2_amd.core.utils import resize_bilinear
    rgb = img[..., :3]
    if mode == 0:
        return resize_bilinear(rgb, S, S)
    if mode == 1:
        return resize_bilinear(rgb.astype(np.float32) * np.float32(1.0 / 255.0), S, S)
    return resize_bilinear(rgb.astype(np.float32), S, S) / np.float32(255)


def _per_image(rt, images, modes, S):
    """The serial route: one upload and one y3_preprocess_image per image."""
    batch = torch.zeros((len(images), S, S, 3), device="cuda")
    for slot, (img, mode) in enumerate(zip(images, modes)):
        rt.preprocess_image(_cuda(img), batch, slot, divide_after=(mode == 2))
    return batch


@pytest.mark.parametrize("S", [64, 96, 416, 608, 51])
def test_batch_kernel_is_bit_exact(rt, S):
    """One call for 39 unlike images == y3_preprocess_image per image == the NumPy restatement of TF's kernel.  S = 51 has
    S*S % 4 != 0 and takes the scalar-store path; the others take the 16-byte stores."""
    images, modes = _mixed_images(S)
    assert len(images) >= 9
    blob, descs = rt.pack_images(images, modes)
    first, n = 2, len(images)
    batch = torch.zeros((first + n + 1, S, S, 3), device="cuda")
    rt.preprocess_batch(_cuda(blob), descs, batch, first_slot=first)
    want = _per_image(rt, images, modes, S).cpu().numpy()
    got = batch.cpu().numpy()
    assert not got[:first].any() and not got[first + n:].any(), "slots outside [first_slot, first_slot + n) were written"
    for i, (img, mode) in enumerate(zip(images, modes)):
        assert np.array_equal(got[first + i], want[i]), (i, img.shape, mode, float(np.abs(got[first + i] - want[i]).max()))
        ref = _host_reference(img, mode, S)
        assert np.array_equal(got[first + i], ref), (i, img.shape, mode, float(np.abs(got[first + i] - ref).max()))


def test_unaligned_batch_base_takes_the_scalar_path(rt):
    """A batch whose base is not 16-byte aligned cannot take the vector stores; the values are the same."""
    S = 64
    images, modes = _mixed_images(3)
    blob, descs = rt.pack_images(images, modes)
    flat = torch.zeros(len(images) * S * S * 3 + 4, device="cuda")
    batch = flat[1:1 + len(images) * S * S * 3].view(len(images), S, S, 3)
    assert batch.data_ptr() % 16 == 4 and batch.is_contiguous()
    rt.preprocess_batch(_cuda(blob), descs, batch)
    assert torch.equal(batch, _per_image(rt, images, modes, S))
    assert flat[0] == 0 and not flat[-3:].any()


def test_more_images_than_one_launch_holds(rt):
    """150 images: launches of 72, 72 and 6 inside one call == the same images issued as chunks of 50 == per image.  A 1x1x3 image and
    a four-channel image sit on either side of both launch boundaries."""
    S = 64
    rng = np.random.default_rng(150)
    images = [rng.integers(0, 256, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(3, 5))), dtype=np.uint8)
              for _ in range(150)]
    for i, shape in ((71, (1, 1, 3)), (72, (23, 39, 4)), (143, (39, 17, 4)), (144, (1, 1, 3))):
        images[i] = rng.integers(0, 256, shape, dtype=np.uint8)
    modes = [int(m) for m in rng.integers(1, 3, len(images))]
    blob, descs = rt.pack_images(images, modes)
    blob_dev = _cuda(blob)
    one = torch.zeros((len(images) + 1, S, S, 3), device="cuda")
    rt.preprocess_batch(blob_dev, descs, one, first_slot=1)
    chunks = torch.zeros_like(one)
    for i0 in range(0, len(images), 50):
        rt.preprocess_batch(blob_dev, descs[i0:i0 + 50], chunks, first_slot=1 + i0)
    assert torch.equal(one, chunks)
    assert not one[0].any() and torch.equal(one[1:], _per_image(rt, images, modes, S))


def test_device_call_refuses_bad_arguments(rt):
    S = 32
    img = np.random.default_rng(1).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    blob, descs = rt.pack_images([img, img], 1)
    batch = torch.zeros((2, S, S, 3), device="cuda")
    with pytest.raises(rt.Y3Error):
        rt.preprocess_batch(_cuda(blob), descs, batch, first_slot=1)        # the second image has no slot
    with pytest.raises(rt.Y3Error):
        rt.preprocess_batch(_cuda(blob[:-1]), descs, batch)                 # the blob is a byte short
    with pytest.raises(rt.Y3Error):
        rt.preprocess_batch(_cuda(blob), np.zeros(2, np.dtype([("offset", "<u8"), ("height", "<i4")])), batch)
    torch.cuda.synchronize()
    assert not batch.any()


def _frame_batches(seed, sizes):
    rng = np.random.default_rng(seed)
    shapes = [(480, 640, 3), (100, 37, 3), (300, 400, 4), (64, 48, 3), (720, 1280, 3)]
    return [[rng.integers(0, 256, shapes[int(rng.integers(len(shapes)))], dtype=np.uint8) for _ in range(n)] for n in sizes]


def test_ring_keeps_batches_in_flight_apart(rt):
    """InputStage(depth=2) over 7 distinct batches with no host synchronise between the submits; the consumer's stream is
    kept busy before every read, so the copy stream runs ahead of it and a slot overwritten while still in flight shows
    up as another batch's pixels.  Bit-equal to the serial per-image route or the ring is wrong."""
    S = 128
    batches = _frame_batches(21, [5, 3, 6, 6, 1, 4, 6])
    stage = rt.InputStage(S, 6, max(rt.packed_nbytes(b) for b in batches), depth=2)
    busy = torch.randn((2048, 2048), device="cuda")
    got = []
    for b in batches:
        h = stage.submit(b, 1)
        for _ in range(8):                                   # the consumer is slower than the stage
            busy = torch.mm(busy, busy).clamp_(-1, 1)
        torch.cuda.current_stream().wait_event(h.ready)
        got.append(h.batch.clone())
        stage.release(h)
    with pytest.raises(rt.Y3Error):
        stage.release(h)                                     # twice
    torch.cuda.synchronize()
    for i, (b, g) in enumerate(zip(batches, got)):
        assert g.shape[0] == len(b)
        assert torch.equal(g, _per_image(rt, b, [1] * len(b), S)), i
    # a slot that was never released is not handed out again
    h1, h2 = stage.submit(batches[0], 1), stage.submit(batches[1], 1)
    with pytest.raises(rt.Y3Error):
        stage.submit(batches[2], 1)
    stage.release(h1)
    stage.release(h2)
    with pytest.raises(rt.Y3Error):
        stage.submit(batches[0] * 2, 1)                      # more images than max_batch
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_detect_stream_equals_the_serial_route(rt, program, weights, anchors, mode):
    """detect_stream at 416^2 over batches of 4, 4 and 3 frames: packed and num_valid of every batch, the ragged last one
    included, are np.array_equal to preprocess_image per slot + Net.detect on the same net, in submission order."""
    from yolo_v3_tf2_amd import _lib
    S = 416
    batches = _frame_batches(33, [4, 4, 3])
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[mode])
    want = []
    for b in batches:
        packed, nv = net.detect(_per_image(rt, b, [1] * len(b), S), anchors, 100, 0.5, 0.05)
        want.append((packed.cpu().numpy(), nv.cpu().numpy()))
    got = list(net.detect_stream(batches, anchors, 100, 0.5, 0.05, mode=1, depth=2))
    assert len(got) == len(batches)
    print("num_valid per batch:", [w[1].tolist() for w in want])
    for i, ((gp, gn), (wp, wn)) in enumerate(zip(got, want)):
        assert isinstance(gp, np.ndarray) and gp.shape == (len(batches[i]), 100, 7) and gn.shape == (len(batches[i]),)
        assert np.array_equal(gn, wn), (i, gn, wn)
        assert np.array_equal(gp, wp), i
    assert not np.array_equal(want[0][0], want[1][0]), "the batches must differ for the order to mean anything"
    # an iterator (sizes not visible in advance) with the bounds given, and a second run on the same net
    cap = max(rt.packed_nbytes(b) for b in batches)
    again = list(net.detect_stream(iter(batches), anchors, 100, 0.5, 0.05, max_batch=4, max_blob_bytes=cap))
    assert all(np.array_equal(a[0], w[0]) and np.array_equal(a[1], w[1]) for a, w in zip(again, want))
    with pytest.raises(rt.Y3Error):
        list(net.detect_stream(iter(batches), anchors, 100, 0.5, 0.05))


def test_preprocess_batch_and_detect_in_one_graph(rt, program, weights, anchors):
    """preprocess_batch + Net.detect captured into one graph; each replay, after new pixel values of the same shapes were
    copied into the device blob, equals the eager result.  (The descriptors are frozen into the graph.)"""
    S, shapes = 160, [(480, 640, 3), (100, 37, 4), (200, 150, 3)]
    rng = np.random.default_rng(9)

    def frames():
        return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]

    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(len(shapes), S)
    blob, descs = rt.pack_images(frames(), 1)
    blob_dev = _cuda(blob)
    batch = torch.zeros((len(shapes), S, S, 3), device="cuda")

    def step():
        rt.preprocess_batch(blob_dev, descs, batch)
        return net.detect(batch, anchors, 100, 0.5, 0.05)

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
        blob2, descs2 = rt.pack_images(new, 1)
        assert np.array_equal(descs2, descs)
        ep, en = net.detect(_per_image(rt, new, [1] * len(new), S), anchors, 100, 0.5, 0.05)
        blob_dev.copy_(torch.from_numpy(blob2))
        gp.zero_()
        gn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gn, en) and torch.equal(gp, ep)
        seen.append(ep.clone())
    assert not torch.equal(seen[0], seen[1]), "the two replays must see different pixels"
