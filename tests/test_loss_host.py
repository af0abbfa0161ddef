"""Validation loss, host tier (no GPU): the NumPy restatements of the reference's label assignment (core/preprocess_dataset.py)
and loss (core/loss_func.py) -- hand-made assignment cases, known answers that pin the restated Keras operators, the dense
form against the sparse form, the basis of the bar the device is held to -- and the argument checks of the two C entry points."""
import ctypes as C

import numpy as np
import pytest

from tests.loss_cases import (LOSS_RTOL, RECIPE_GRIDS, all_loss_cases, anchors, collisions, recipe, relative_gap, unit_batch,
                              unit_cases, unit_want)

EPS = np.float32(1e-7)


def _assign(case, a=None):
    from yolo_v3_tf2_amd.core.preprocess_dataset import assign_targets
    return assign_targets(case["gt_boxes"], case["gt_classes"], case["gt_count"], anchors() if a is None else a, case["grid_sizes"],
                          case["nc"])


def _loss(case, cells, dtype=np.float32):
    from yolo_v3_tf2_amd.core.loss_func import loss_from_cells
    return loss_from_cells(case["grids"], case["gt_boxes"], case["gt_classes"], cells, anchors(), case["nc"], dtype=dtype)


@pytest.mark.parametrize("case", unit_cases(), ids=lambda c: c[0])
def test_assignment_unit_cases(case):
    from yolo_v3_tf2_amd.core.preprocess_dataset import assign_targets
    name, nc, a, images, want = case
    gb, gc, cnt = unit_batch(images)
    cells = assign_targets(gb, gc, cnt, a, RECIPE_GRIDS, nc)
    assert cells.dtype == np.int32 and np.array_equal(cells, unit_want(want, gb.shape[1])), (name, cells)
    # wider buffers change nothing but the padding
    gb, gc, cnt = unit_batch(images, max_gt=5)
    assert np.array_equal(assign_targets(gb, gc, cnt, a, RECIPE_GRIDS, nc), unit_want(want, 5))


@pytest.mark.parametrize("nc", [1, 7, 80])
def test_the_recipe_sees_what_it_is_meant_to_see(nc):
    """recipe() itself asserts the nine (scale, anchor) pairs and the collisions; here: the counts, and every live row is accounted for."""
    case = recipe(nc)
    cells = _assign(case)
    print(nc, "collisions:", collisions(cells))
    assert case["gt_count"].tolist() == [1, 3, 8, 40, 0]
    live = np.arange(40)[None] < case["gt_count"][:, None]
    assert (cells[~live] == -1).all() and ((cells[live] >= 0) | (cells[live] == -2)).all() and cells.max() < 252
    kept = cells[cells >= 0]
    for b in range(5):
        row = cells[b][cells[b] >= 0]
        assert len(set(row.tolist())) == len(row), "two rows of one image kept the same cell"
    assert len(kept) + collisions(cells) == 52


def _zero_case(nc, images, a=None, grid_sizes=RECIPE_GRIDS):
    gb, gc, cnt = unit_batch(images)
    return dict(grids=[np.zeros((len(images), g, g, 3, 5 + nc), np.float32) for g in grid_sizes], gt_boxes=gb, gt_classes=gc,
                gt_count=cnt, grid_sizes=grid_sizes, nc=nc)


def test_known_answer_zero_grids_without_ground_truth():
    case = _zero_case(7, [([], [])])
    loss = _loss(case, _assign(case))
    term = -np.log(np.float32(0.5) + EPS)
    assert term.dtype == np.float32
    for s, g in enumerate(RECIPE_GRIDS):
        assert loss[0, s].tolist() == [0.0, 0.0, 3 * g * g * float(term), 0.0]


def test_known_answer_equal_class_logits_give_log_nc():
    for nc in (7, 80):
        case = _zero_case(nc, [([[0.2, 0.3, 0.5, 0.7]], [nc - 1])])
        for t in case["grids"]:
            t[..., 5:] = 1.25
        cells = _assign(case)
        loss = _loss(case, cells)
        s = [k for k in range(3) if loss[0, k, 3] != 0]
        assert len(s) == 1 and abs(loss[0, s[0], 3] - np.log(nc)) <= 4 * 2.0**-24 * np.log(nc)


def test_known_answer_one_class_has_no_class_loss():
    case = recipe(1)
    loss = _loss(case, _assign(case))
    assert (loss[..., 3] == 0).all() and (loss[:4, :, 2] > 0).all() and loss[..., 0].sum() > 0


def test_known_answer_a_box_that_is_its_anchor_on_a_cell_centre():
    """Anchor (0.25, 0.125) of the 4 x 4 grid, centre (0.375, 0.375) = the centre of cell (1,1), all in binary fractions, zero
    logits: tx = ty = 0.5 = sigmoid(0), log(tw / aw) = 0 = t[2]."""
    a = anchors().copy()
    a[1, 1] = (0.25, 0.125)
    from yolo_v3_tf2_amd.core.loss_func import loss_from_cells
    case = _zero_case(3, [([[0.25, 0.3125, 0.5, 0.4375]], [1])])
    cells = _assign(case, a)
    assert cells.tolist() == [[12 + (1 * 4 + 1) * 3 + 1]]
    loss = loss_from_cells(case["grids"], case["gt_boxes"], case["gt_classes"], cells, a, 3)
    assert loss[0, 1, 0] == 0 and loss[0, 1, 1] == 0 and loss[0, 1, 3] > 0
    term, hit = -np.log(np.float32(0.5) + EPS), -np.log(np.float32(0.5) + EPS)
    assert loss[0, 1, 2] == 47 * float(term) + float(hit)


def test_known_answer_a_zero_width_box_has_a_finite_wh_term():
    """log(0 / aw) = -inf is replaced by 0: the width part of the term is t[2]^2 = 0, the height part is log(th / ah)^2."""
    case = _zero_case(3, [([[0.5, 0.4, 0.5, 0.6]], [0])])
    cells = _assign(case)
    loss = _loss(case, cells)
    n = int(cells[0, 0])
    assert n >= 0
    s = int(np.searchsorted([0, 12, 60, 252], n, side="right")) - 1
    ah = anchors()[s, (n - [0, 12, 60][s]) % 3, 1]
    want = np.float32(2) * np.square(np.log(np.float32(0.6) - np.float32(0.4)) - np.log(ah) + np.float32(0))
    assert np.isfinite(loss).all() and loss[0, s, 1] > 0 and abs(loss[0, s, 1] - want) <= 1e-5 * want


@pytest.mark.parametrize("nc", [1, 7, 80])
def test_dense_form_equals_sparse_form(nc):
    """_arrange_in_grid + get_loss_func (the reference's shapes and names) == assign_targets + loss_from_cells: the same fp32 terms,
    only the order of the fp64 sums differs."""
    from yolo_v3_tf2_amd.core.loss_func import get_loss_func
    from yolo_v3_tf2_amd.core.preprocess_dataset import PreprocessDataset
    case = recipe(nc)
    B, G = case["gt_classes"].shape
    live = np.arange(G)[None] < case["gt_count"][:, None]
    y = np.concatenate([case["gt_boxes"], live[..., None], case["gt_classes"][..., None]], -1).astype(np.float32)
    sparse = _loss(case, _assign(case)).sum(axis=0)
    a = anchors()
    for s, g in enumerate(RECIPE_GRIDS):
        y_true = PreprocessDataset()._arrange_in_grid(y, a, s, [B, g, g, 3, 6], G)
        assert y_true.shape == (B, g, g, 3, 6) and y_true[..., 4].sum() > 0
        dense = get_loss_func(a[s], nc)(y_true, case["grids"][s])
        assert dense.shape == (4,) and dense.dtype == np.float64
        assert np.abs(dense - sparse[s]).max() <= 1e-12 * np.abs(sparse[s]).max(), (s, dense, sparse[s])
        assert get_loss_func(a[s], nc, eager_mode=False)(y_true, case["grids"][s]) == dense.sum()


def test_dense_form_raises_where_the_reference_scatter_raises():
    from yolo_v3_tf2_amd.core.preprocess_dataset import PreprocessDataset
    y = np.array([[[0.75, 0.2, 1.25, 0.4, 1, 0]]], np.float32)
    with pytest.raises(IndexError):
        for s, g in enumerate(RECIPE_GRIDS):
            PreprocessDataset()._arrange_in_grid(y, anchors(), s, [1, g, g, 3, 6], 1)


def test_error_images_are_left_out_of_the_loss():
    case = dict(recipe(7))
    gc = case["gt_classes"].copy()
    gc[2, 5] = 7
    bad = dict(case, gt_classes=gc)
    cells = _assign(bad)
    assert (cells[2, :8] == -3).all() and (cells[2, 8:] == -1).all()
    loss, clean = _loss(bad, cells), _loss(case, _assign(case))
    assert not loss[2].any() and np.array_equal(np.delete(loss, 2, 0), np.delete(clean, 2, 0))


def test_float32_rounding_stays_under_a_quarter_of_the_bar():
    """The bar's basis: over every case the GPU test compares on, the float32 restatement is within LOSS_RTOL / 4 of the float64 one."""
    worst = 0.0
    for name, case in all_loss_cases():
        cells = _assign(case)
        gap = relative_gap(_loss(case, cells), _loss(case, cells, np.float64))
        print(f"{name}: fp32 against fp64 {gap:.3g}")
        worst = max(worst, gap)
    print(f"largest {worst:.3g}, bar {LOSS_RTOL:.3g}")
    assert 0 < worst <= LOSS_RTOL / 4
    assert worst >= LOSS_RTOL / 8, "the bar has drifted away from the gap it was derived from"


def test_summarize_loss():
    from yolo_v3_tf2_amd.core.loss_func import summarize_loss
    total = np.arange(12, dtype=np.float64).reshape(3, 4)
    val_loss, per_grid, per_source = summarize_loss(total, 4)
    assert val_loss == 66 / 4 and per_grid.tolist() == [6 / 4, 22 / 4, 38 / 4] and per_source.tolist() == [12 / 4, 15 / 4, 18 / 4, 21 / 4]


# ---------------------------------------------------------------------------------------------------------------------------
# a pointer that is never dereferenced: every check fails on the host before any HIP call
_FAKE = 0x10000


def _call(lib, entry, **kw):
    gs = (C.c_int32 * 3)(*kw.pop("grid_sizes", (13, 26, 52)))
    an = (C.c_float * 18)(*([0.1] * 18))
    grids = kw.pop("grids", (_FAKE, _FAKE, _FAKE))
    grids = None if grids is None else (C.c_void_p * 3)(*grids)
    a = dict(gt_boxes=_FAKE, gt_classes=_FAKE, gt_count=_FAKE, batch=2, max_gt=10, nclasses=80, gs=gs, anchors=an, cells=_FAKE,
             grids=grids, loss=_FAKE)
    a.update(kw)
    if entry == "y3_yolo_assign_targets":
        return lib.y3_yolo_assign_targets(a["gt_boxes"], a["gt_classes"], a["gt_count"], a["batch"], a["max_gt"], a["nclasses"], a["gs"],
                                          a["anchors"], a["cells"], None)
    return lib.y3_yolo_loss(a["grids"], a["gs"], a["batch"], a["nclasses"], a["anchors"], a["gt_boxes"], a["gt_classes"], a["cells"],
                            a["max_gt"], a["loss"], None)


_BAD_BOTH = [dict(gt_boxes=None), dict(gt_classes=None), dict(cells=None), dict(gs=None), dict(anchors=None), dict(batch=0),
             dict(max_gt=0), dict(max_gt=1025), dict(nclasses=0), dict(nclasses=4097), dict(grid_sizes=(13, 0, 52)),
             dict(grid_sizes=(13, 26, 257)), dict(gt_boxes=_FAKE + 2)]
_ids = lambda d: "%s=%s" % next(iter(d.items()))


@pytest.mark.parametrize("bad", _BAD_BOTH + [dict(gt_count=None)], ids=_ids)
def test_assign_targets_refuses_bad_arguments_on_the_host(bad):
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert _call(lib, "y3_yolo_assign_targets", **dict(bad)) == _lib.Y3_ERR_INVALID
    msg = lib.y3_last_error()
    assert b"y3_yolo_assign_targets" in msg and len(msg) > len(b"y3_yolo_assign_targets: "), msg


@pytest.mark.parametrize("bad", _BAD_BOTH + [dict(loss=None), dict(loss=_FAKE + 4), dict(grids=None), dict(grids=(_FAKE, 0, _FAKE))],
                         ids=_ids)
def test_yolo_loss_refuses_bad_arguments_on_the_host(bad):
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert _call(lib, "y3_yolo_loss", **dict(bad)) == _lib.Y3_ERR_INVALID
    msg = lib.y3_last_error()
    assert b"y3_yolo_loss" in msg and len(msg) > len(b"y3_yolo_loss: "), msg


def test_no_cpu_fallback():
    import torch
    from yolo_v3_tf2_amd import runtime
    case = recipe(7)
    gb, gc, cnt = (torch.from_numpy(case[k]) for k in ("gt_boxes", "gt_classes", "gt_count"))
    with pytest.raises(runtime.Y3Error):
        runtime.assign_targets(gb, gc, cnt, anchors(), RECIPE_GRIDS, 7)
    with pytest.raises(runtime.Y3Error):
        runtime.yolo_loss([torch.from_numpy(g) for g in case["grids"]], anchors(), 7, gb, gc, torch.zeros((5, 40), dtype=torch.int32))
