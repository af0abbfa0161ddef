"""Validation loss on the GPU: assign_targets_kernel (y3_yolo_assign_targets) bit for bit against its host restatement
core.preprocess_dataset.assign_targets, yolo_loss_kernel (y3_yolo_loss) against core.loss_func.loss_from_cells on the same logits
within tests/loss_cases.LOSS_RTOL (exact zeros stay exact), determinism across runs / batch positions / batch sizes, error
images, the network's own grids, Net.evaluate_stream(loss=True), and graph capture."""
import numpy as np
import pytest

from tests.loss_cases import (LOSS_RTOL, RECIPE_GRIDS, all_loss_cases, anchors as file_anchors, large_case, random_boxes, recipe,
                              relative_gap, unit_batch, unit_cases, unit_want)

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


def _guard(a):
    """The array on the GPU with one guard image on either side (copies of image 0: rows that would count if they were read)."""
    a = np.asarray(a)
    return _cuda(np.concatenate([a[:1], a, a[:1]]))


def _same_bits(x, y):
    """torch.equal on the words: a NaN among the inputs equals itself."""
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def _host_cells(case, a=None):
    from yolo_v3_tf2_amd.core.preprocess_dataset import assign_targets
    return assign_targets(case["gt_boxes"], case["gt_classes"], case["gt_count"], file_anchors() if a is None else a,
                          case["grid_sizes"], case["nc"])


def _host_loss(case, cells, a=None):
    from yolo_v3_tf2_amd.core.loss_func import loss_from_cells
    return loss_from_cells(case["grids"], case["gt_boxes"], case["gt_classes"], cells, file_anchors() if a is None else a, case["nc"])


def _device_cells(rt, gb, gc, cnt, a, grid_sizes, nc):
    """y3_yolo_assign_targets on views between guard images; the inputs and the guard rows of the output must come back untouched."""
    B, G = gc.shape
    bufs = [_guard(gb), _guard(gc), _guard(cnt)]
    before = [b.clone() for b in bufs]
    out = torch.full((B + 2, G), 77, dtype=torch.int32, device="cuda")
    rt.assign_targets(*[b[1:-1] for b in bufs], a, grid_sizes, nc, cells=out[1:-1])
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(bufs, before)), "the inputs were written"
    assert (out[0] == 77).all() and (out[-1] == 77).all(), "cells were written outside the batch"
    return out[1:-1].cpu().numpy()


def _device_loss(rt, case, cells, a=None):
    """y3_yolo_loss between guard images, as above -> float64 [B,3,4]."""
    a = file_anchors() if a is None else a
    B = cells.shape[0]
    bufs = [_guard(g) for g in case["grids"]] + [_guard(case["gt_boxes"]), _guard(case["gt_classes"]), _guard(cells)]
    before = [b.clone() for b in bufs]
    out = torch.full((B + 2, 3, 4), -7.0, dtype=torch.float64, device="cuda")
    v = [b[1:-1] for b in bufs]
    rt.yolo_loss(v[:3], a, case["nc"], v[3], v[4], v[5], loss=out[1:-1])
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(bufs, before)), "the inputs were written"
    assert (out[0] == -7).all() and (out[-1] == -7).all(), "the loss was written outside the batch"
    return out[1:-1].cpu().numpy()


@pytest.mark.parametrize("name,case", list(all_loss_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_cells_and_loss_equal_the_host_restatement(rt, name, case):
    """Grids (2,4,8) with 0 to 40 boxes per image and 1 / 7 / 80 classes, max_gt 40 and 1; (13,26,52) with up to 100 boxes;
    (19,38,76): the larger bitmap.  cells: np.array_equal.  loss: an entry that is exactly 0 on the host is exactly 0 on the
    device, every other one within LOSS_RTOL of the host's (same logits, same fp32 terms, other expf / logf)."""
    want_cells = _host_cells(case)
    cells = _device_cells(rt, case["gt_boxes"], case["gt_classes"], case["gt_count"], file_anchors(), case["grid_sizes"], case["nc"])
    assert cells.dtype == np.int32 and np.array_equal(cells, want_cells)
    want = _host_loss(case, want_cells)
    got = _device_loss(rt, case, cells)
    gap = relative_gap(got, want)
    print(f"{name}: device against host {gap:.3g} (bar {LOSS_RTOL:.3g}); val_loss of the batch {want.sum():.6f}")
    assert got.dtype == np.float64 and want[..., 2].all() and want[..., 0].any()
    assert gap <= LOSS_RTOL


@pytest.mark.parametrize("case", unit_cases(), ids=lambda c: c[0])
def test_cells_on_the_unit_cases(rt, case):
    name, nc, a, images, want = case
    for max_gt in (None, 5):
        gb, gc, cnt = unit_batch(images, max_gt)
        cells = _device_cells(rt, gb, gc, cnt, a, RECIPE_GRIDS, nc)
        assert np.array_equal(cells, unit_want(want, gb.shape[1])), (name, cells)
        assert np.array_equal(cells, _host_cells(dict(gt_boxes=gb, gt_classes=gc, gt_count=cnt, grid_sizes=RECIPE_GRIDS, nc=nc), a))


def _zero_case(nc, images):
    gb, gc, cnt = unit_batch(images)
    return dict(grids=[np.zeros((len(images), g, g, 3, 5 + nc), np.float32) for g in RECIPE_GRIDS], gt_boxes=gb, gt_classes=gc,
                gt_count=cnt, grid_sizes=RECIPE_GRIDS, nc=nc)


def test_known_answers(rt):
    """The device's own expf / logf on the answers that are exact: zero grids without ground truth; a box that is its anchor on a
    cell centre with zero logits (xy = wh = 0); one class (class = 0); and a zero-width box (finite wh)."""
    eps = np.float32(1e-7)
    case = _zero_case(7, [([], [])])
    got = _device_loss(rt, case, _host_cells(case))
    term = float(-np.log(np.float32(0.5) + eps))
    for s, g in enumerate(RECIPE_GRIDS):
        assert got[0, s, [0, 1, 3]].tolist() == [0, 0, 0]
        assert abs(got[0, s, 2] - 3 * g * g * term) <= 2.0**-23 * 3 * g * g * term      # one ulp of logf
    a = file_anchors().copy()
    a[1, 1] = (0.25, 0.125)
    case = _zero_case(3, [([[0.25, 0.3125, 0.5, 0.4375]], [1])])
    cells = _host_cells(case, a)
    got, want = _device_loss(rt, case, cells, a), _host_loss(case, cells, a)
    assert got[0, 1, 0] == 0 and got[0, 1, 1] == 0 and got[0, 1, 3] > 0 and relative_gap(got, want) <= LOSS_RTOL
    case = recipe(1)
    got = _device_loss(rt, case, _host_cells(case))
    assert (got[..., 3] == 0).all() and got[..., 0].any()
    case = _zero_case(3, [([[0.5, 0.4, 0.5, 0.6]], [0])])
    cells = _host_cells(case)
    got, want = _device_loss(rt, case, cells), _host_loss(case, cells)
    assert np.isfinite(got).all() and got[0, :, 1].sum() > 0 and relative_gap(got, want) <= LOSS_RTOL


def _loss_of(rt, case, rows, max_gt=None):
    """The device's loss of the images `rows` of the case, as a batch of their own."""
    G = max_gt or case["gt_classes"].shape[1]
    gb, gc, cnt = case["gt_boxes"][rows, :G], case["gt_classes"][rows, :G], case["gt_count"][rows]
    cells = rt.assign_targets(_cuda(gb), _cuda(gc), _cuda(cnt), file_anchors(), case["grid_sizes"], case["nc"])
    loss = rt.yolo_loss([_cuda(g[rows]) for g in case["grids"]], file_anchors(), case["nc"], _cuda(gb), _cuda(gc), cells)
    return cells.cpu().numpy(), loss.cpu().numpy()


def test_an_image_has_the_same_bits_wherever_it_is(rt):
    """The same call twice; each image alone; the batch reversed; and (13,26,52) against itself with an image repeated: every
    image's twelve numbers are the same bits."""
    for case in (recipe(80), recipe(7), large_case((13, 26, 52))):
        B = len(case["gt_count"])
        every = list(range(B))
        cells, whole = _loss_of(rt, case, every)
        assert np.array_equal(_loss_of(rt, case, every)[1], whole), "two runs differ"
        for i in every:
            assert np.array_equal(_loss_of(rt, case, [i])[1][0], whole[i]), f"image {i} alone differs"
        assert np.array_equal(_loss_of(rt, case, every[::-1])[1], whole[::-1]), "positions matter"
        assert np.array_equal(_loss_of(rt, case, [B - 1, 0, 0, B - 2])[1], whole[[B - 1, 0, 0, B - 2]])
        assert whole[:B - 1, :, 2].all()
    # buffers of another width: image 2 of the recipe (8 boxes) with max_gt = 8 instead of 40
    case = recipe(80)
    assert np.array_equal(_loss_of(rt, case, [2], max_gt=8)[1][0], _loss_of(rt, case, [0, 2])[1][1])


def test_error_images_get_zeros_and_leave_their_neighbours_alone(rt):
    case = recipe(7)
    clean_cells, clean = _loss_of(rt, case, list(range(5)))
    gb, gc = case["gt_boxes"].copy(), case["gt_classes"].copy()
    gc[2, 5] = 7                           # a class equal to nclasses
    gb[3, 17] = [0.75, 0.2, 1.25, 0.4]     # a centre of exactly 1.0
    bad = dict(case, gt_boxes=gb, gt_classes=gc)
    cells, loss = _loss_of(rt, bad, list(range(5)))
    assert np.array_equal(cells, _host_cells(bad))
    assert (cells[2, :8] == -3).all() and (cells[2, 8:] == -1).all() and (cells[3] == -3).all()
    assert not loss[2].any() and not loss[3].any()
    for i in (0, 1, 4):
        assert np.array_equal(cells[i], clean_cells[i]) and np.array_equal(loss[i], clean[i])
    # the loss kernel's own guard: cells that name a row while the class cannot index its logits
    gc = case["gt_classes"].copy()
    gc[2, int(np.argmax(clean_cells[2] >= 0))] = -1
    loss = rt.yolo_loss([_cuda(g) for g in case["grids"]], file_anchors(), 7, _cuda(case["gt_boxes"]), _cuda(gc),
                        _cuda(clean_cells)).cpu().numpy()
    assert not loss[2].any() and np.array_equal(loss[[0, 1, 3, 4]], clean[[0, 1, 3, 4]])


def test_bad_arguments_raise(rt):
    case = recipe(7)
    gb, gc, cnt = (_cuda(case[k]) for k in ("gt_boxes", "gt_classes", "gt_count"))
    grids = [_cuda(g) for g in case["grids"]]
    a = file_anchors()
    cells = rt.assign_targets(gb, gc, cnt, a, RECIPE_GRIDS, 7)
    assert cells.shape == (5, 40) and rt.yolo_loss(grids, a, 7, gb, gc, cells).shape == (5, 3, 4)
    for args in ((gb.cpu(), gc, cnt), (gb.double(), gc, cnt), (gb, gc.long(), cnt), (gb, gc, cnt.long()), (gb[:4], gc, cnt),
                 (gb, gc[:, :39], cnt), (gb, gc, cnt[:4]), (gb[..., :3], gc, cnt)):
        with pytest.raises(rt.Y3Error):
            rt.assign_targets(*args, a, RECIPE_GRIDS, 7)
    for kw in (dict(cells=cells.long()), dict(cells=cells[:4]), dict(cells=cells.cpu())):
        with pytest.raises(rt.Y3Error):
            rt.assign_targets(gb, gc, cnt, a, RECIPE_GRIDS, 7, **kw)
    for bad in (lambda: rt.assign_targets(gb, gc, cnt, a, (2, 4), 7), lambda: rt.assign_targets(gb, gc, cnt, a, (2, 4, 300), 7),
                lambda: rt.assign_targets(gb, gc, cnt, a, RECIPE_GRIDS, 5000), lambda: rt.assign_targets(gb, gc, cnt, a[:2], RECIPE_GRIDS, 7),
                lambda: rt.yolo_loss(grids[:2], a, 7, gb, gc, cells), lambda: rt.yolo_loss(grids, a, 6, gb, gc, cells),
                lambda: rt.yolo_loss(grids, a, 7, gb[:4], gc[:4], cells[:4]), lambda: rt.yolo_loss(grids, a, 7, gb, gc, cells.long()),
                lambda: rt.yolo_loss(grids, a, 7, gb, gc, cells[:, :39]), lambda: rt.yolo_loss(grids, a, 7, gb, gc, cells, loss=torch.zeros((5, 3, 4), device="cuda")),
                lambda: rt.yolo_loss([g.cpu() for g in grids], a, 7, gb, gc, cells)):
        with pytest.raises(rt.Y3Error):
            bad()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# the network's own grids: S = 64, the seeded synthetic weights of tests/golden/e2e_s64_seed4321.npz -> grids (2,4,8), 80 classes
def _ground_truth(seed, counts, nc=80):
    rng = np.random.default_rng(seed)
    return [(random_boxes(rng, n), rng.integers(0, nc, n).astype(np.int32)) for n in counts]


def test_loss_of_the_networks_own_grids(rt, program, weights, anchors):
    """Net.forward, then the two calls, against loss_from_cells on the grids read back from the device: the new kernels apart
    from the rounding of the convs."""
    import os
    from tests.loss_cases import ROOT
    images = np.load(os.path.join(ROOT, "tests", "golden", "e2e_s64_seed4321.npz"))["images"]
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(2, 64)
    grids = net.forward(_cuda(images))
    assert [g.shape[1] for g in grids] == [2, 4, 8]
    gb, gc, cnt = rt.pack_ground_truth(_ground_truth(64, (12, 5)))
    cells = rt.assign_targets(_cuda(gb), _cuda(gc), _cuda(cnt), anchors, net.grid_sizes(), 80)
    loss = rt.yolo_loss(grids, anchors, 80, _cuda(gb), _cuda(gc), cells).cpu().numpy()
    case = dict(grids=[g.cpu().numpy() for g in grids], gt_boxes=gb, gt_classes=gc, gt_count=cnt, grid_sizes=(2, 4, 8), nc=80)
    want_cells = _host_cells(case, anchors)
    assert np.array_equal(cells.cpu().numpy(), want_cells) and (want_cells >= 0).sum() >= 10
    want = _host_loss(case, want_cells, anchors)
    gap = relative_gap(loss, want)
    print(f"network grids: device against host {gap:.3g} (bar {LOSS_RTOL:.3g}); per image {want.sum(axis=(1, 2))}")
    assert want.all() and gap <= LOSS_RTOL


def _frames(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def test_evaluate_stream_with_loss(rt, program, weights, anchors):
    """Two batches at S = 64, the second ragged, one error image: the counters are those of loss=False, `sum` has the bits of
    forward + assign_targets + yolo_loss composed by hand per batch with the same torch reductions, images / errors are right."""
    S, thresholds = 64, [0.05, 0.1, 0.2]
    batches = [_frames(1, [(64, 64), (50, 70), (90, 64)]), _frames(2, [(64, 80), (33, 47)])]
    gts = [_ground_truth(3, (4, 0, 9)), _ground_truth(4, (6, 2))]
    gts[1][1][1][0] = 80      # a class equal to nclasses: an error image
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(3, S)
    plain = net.evaluate_stream(batches, gts, anchors, 100, 0.5, thresholds, 80)
    counters, loss = net.evaluate_stream(batches, gts, anchors, 100, 0.5, thresholds, 80, loss=True)
    assert np.array_equal(counters, plain) and plain[:, 401].tolist() == [4] * 3 and plain[:, 400].tolist() == [1] * 3
    assert plain[0, :80].sum() > 0, "predictions at the lowest threshold"
    assert sorted(loss) == ["errors", "images", "sum"] and (loss["images"], loss["errors"]) == (4, 1)
    assert loss["sum"].dtype == np.float64 and loss["sum"].shape == (3, 4) and (loss["sum"] > 0).all()
    total = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    per_image = []
    for frames, gt in zip(batches, gts):
        batch = torch.zeros((len(frames), S, S, 3), device="cuda")
        for slot, img in enumerate(frames):
            rt.preprocess_image(_cuda(img), batch, slot)
        grids = net.forward(batch)
        gb, gc, cnt = (_cuda(a) for a in rt.pack_ground_truth(gt, 9))
        cells = rt.assign_targets(gb, gc, cnt, anchors, net.grid_sizes(), 80)
        out = rt.yolo_loss(grids, anchors, 80, gb, gc, cells)
        total += out.sum(dim=0)
        per_image.append(out.cpu().numpy())
    assert np.array_equal(loss["sum"], total.cpu().numpy())
    assert not per_image[1][1].any() and all(p.any() for p in per_image[0]) and per_image[1][0].any()
    # the pair form and the one-class form carry the same loss
    pair, loss2 = net.evaluate_stream(batches, gts, anchors, 100, 0.5, thresholds, 80, one_class="both", loss=True, depth=3)
    assert np.array_equal(pair[0], plain) and np.array_equal(loss2["sum"], loss["sum"]) and loss2["images"] == 4
    # nothing to do: zeros
    empty, loss0 = net.evaluate_stream([], [], anchors, 100, 0.5, thresholds, 80, loss=True)
    assert not empty.any() and not loss0["sum"].any() and (loss0["images"], loss0["errors"]) == (0, 0)


def test_evaluate_stream_refuses_loss_with_letterbox(rt, program, weights, anchors):
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(2, 64)
    batches, gts = [_frames(5, [(64, 64), (40, 64)])], [_ground_truth(6, (2, 3))]
    with pytest.raises(rt.Y3Error, match="letterbox"):
        net.evaluate_stream(batches, gts, anchors, 100, 0.5, [0.1], 80, letterbox=True, loss=True)
    with pytest.raises(rt.Y3Error, match="nclasses"):
        net.evaluate_stream(batches, gts, anchors, 100, 0.5, [0.1], 7, loss=True)
    torch.cuda.synchronize()


def test_both_calls_in_one_graph(rt):
    """y3_yolo_assign_targets + y3_yolo_loss captured on one stream and replayed after the buffers took other values: the bits
    of the eager result."""
    a, b = recipe(80), dict(recipe(80))
    rng = np.random.default_rng(9)
    b["grids"] = [g + rng.normal(0, 0.5, g.shape).astype(np.float32) for g in a["grids"]]
    b["gt_boxes"] = a["gt_boxes"][::-1].copy()
    b["gt_classes"], b["gt_count"] = a["gt_classes"][::-1].copy(), a["gt_count"][::-1].copy()
    anc = file_anchors()
    bufs = {k: _cuda(a[k]) for k in ("gt_boxes", "gt_classes", "gt_count")}
    grids = [_cuda(g) for g in a["grids"]]
    cells = torch.full((5, 40), 77, dtype=torch.int32, device="cuda")
    loss = torch.full((5, 3, 4), -7.0, dtype=torch.float64, device="cuda")

    def step(cells_out, loss_out):
        rt.assign_targets(bufs["gt_boxes"], bufs["gt_classes"], bufs["gt_count"], anc, RECIPE_GRIDS, 80, cells=cells_out)
        return rt.yolo_loss(grids, anc, 80, bufs["gt_boxes"], bufs["gt_classes"], cells_out, loss=loss_out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(torch.empty_like(cells), torch.empty_like(loss))     # warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(cells, loss)
    results = []
    for case in (a, b):
        for k in bufs:
            bufs[k].copy_(_cuda(case[k]))
        for dst, src in zip(grids, case["grids"]):
            dst.copy_(_cuda(src))
        cells.fill_(77)
        loss.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        eager_cells = torch.empty_like(cells)
        eager = step(eager_cells, torch.empty_like(loss))
        assert torch.equal(cells, eager_cells) and torch.equal(loss, eager)
        assert np.array_equal(cells.cpu().numpy(), _host_cells(case))
        results.append(loss.cpu().numpy())
    assert not np.array_equal(results[0], results[1][::-1]), "the two replays must see different logits"


def test_driver_prints_val_loss_from_the_same_pass(rt, weights, tmp_path, capsys):
    """evaluate(on_device=True, loss=True) on the four-image TFRecord set of tests/test_evaluate_gpu.py: the results of the call
    without loss, plus the sums of Net.evaluate_stream, reported in the wording of the reference's eager loop."""
    from tests.test_evaluate_gpu import _same_results, _write_set
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core.loss_func import summarize_loss
    cfg = _write_set(tmp_path / "even", [2, 2, 2, 2], 21)
    plain = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights, on_device=True)
    capsys.readouterr()
    results, loss = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights, on_device=True, loss=True)
    out = capsys.readouterr().out
    _same_results(results, plain)
    assert (loss["images"], loss["errors"]) == (4, 0) and loss["sum"].shape == (3, 4) and (loss["sum"][:, 2] > 0).all()
    val_loss, per_grid, per_source = summarize_loss(loss["sum"], 4)
    assert np.isfinite(val_loss) and val_loss > 0 and abs(per_grid.sum() - val_loss) <= 1e-12 * val_loss
    assert f"val_loss:{val_loss}" in out and "perGrid[" in out and "perSource[xy,wh,obj,class]:" in out
    with pytest.raises(ValueError):
        ev.evaluate(cfg, [0.05], weights=weights, loss=True)
