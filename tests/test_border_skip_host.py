"""Border skip of the fp32 3x3 convs, host side (no GPU): the position table y3_border_order builds -- a permutation of the grid, every
mask9 equal to a brute-force count of the taps that read inside the image, stably sorted by mask class (the number of live taps, then
mask9) -- and a NumPy restatement of the share
of K tiles the sorted, batch-minor order removes for 32 images per lane and 64-row workgroup tiles."""
import ctypes as C

import numpy as np
import pytest

from yolo_v3_tf2_amd import _lib

# (Ho, Wo, H, W, stride): square grids 1, 2, 3, 5, 13, 26, rectangular 3x7 and 10x13, each at stride 1 (H = Ho) and stride 2 (H = 2 Ho)
GRIDS = [(1, 1), (2, 2), (3, 3), (5, 5), (13, 13), (26, 26), (3, 7), (10, 13)]
GEOMETRIES = [(ho, wo, ho * s, wo * s, s) for ho, wo in GRIDS for s in (1, 2)]


def border_order(Ho, Wo, H, W, stride, pad=1):
    out = np.zeros(Ho * Wo, np.uint32)
    _lib.load().y3_border_order(Ho, Wo, H, W, stride, pad, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out >> 20, (out >> 9) & 0x7FF, out & 0x1FF


def sort_key(mask):
    """The table's order: fewer live taps first, mask9 among masks of equal count (positions of one mask stay together)."""
    return (bin(int(mask)).count("1") << 9) | int(mask)


def brute_mask(ho, wo, H, W, stride, pad=1):
    mk = 0
    for u in range(3):
        for v in range(3):
            hi, wi = ho * stride - pad + u, wo * stride - pad + v
            if 0 <= hi < H and 0 <= wi < W:
                mk |= 1 << (u * 3 + v)
    return mk


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "%dx%d_in%dx%d_s%d" % g)
def test_table_is_a_permutation_with_brute_force_masks_stably_sorted(geo):
    Ho, Wo, H, W, stride = geo
    ho, wo, mask = border_order(Ho, Wo, H, W, stride)
    raster = ho.astype(np.int64) * Wo + wo
    assert ho.max() < Ho and wo.max() < Wo
    assert sorted(raster.tolist()) == list(range(Ho * Wo)), "not a permutation of the positions"
    want = np.array([brute_mask(int(a), int(b), H, W, stride) for a, b in zip(ho, wo)], np.uint32)
    assert np.array_equal(mask, want)
    assert (mask & 16).all(), "the centre tap reads inside the image at every position"
    keys = np.array([sort_key(m) for m in mask], np.int64)
    assert (np.diff(keys) >= 0).all(), "not sorted by (live taps, mask9)"
    same = np.diff(mask.astype(np.int64)) == 0
    assert (np.diff(raster)[same] > 0).all(), "positions of one mask left raster order: the sort is not stable"
    # the same table from a stable sort of the raster positions by their brute-force mask
    grid = [(a, b) for a in range(Ho) for b in range(Wo)]
    order = sorted(range(Ho * Wo), key=lambda i: sort_key(brute_mask(*grid[i], H, W, stride)))   # sorted() is stable
    assert raster.tolist() == order


def k_tiles_removed(g, B=32, BM=64, sort=True):
    """Share of the K tiles of a stride-1 3x3 conv on a g x g grid that a launch with batch-minor rows leaves out: rows m = j * B + b over the
    positions j in table order, workgroup tiles of BM rows, a tile walks the taps that read inside the image for at least one of its rows."""
    masks = np.array([brute_mask(a, b, g, g, 1) for a in range(g) for b in range(g)], np.int64)
    if sort:
        masks = masks[np.argsort(np.array([sort_key(m) for m in masks]), kind="stable")]
    rows = np.repeat(masks, B)                                  # mask of every GEMM row
    pad = (-len(rows)) % BM
    tiles = np.concatenate([rows, np.zeros(pad, np.int64)]).reshape(-1, BM)
    live = np.bitwise_or.reduce(tiles, axis=1)
    walked = sum(bin(int(m)).count("1") for m in live)
    return 1.0 - walked / (9.0 * len(live))


@pytest.mark.parametrize("g,floor", [(13, 0.086), (26, 0.048), (52, 0.025)])
def test_k_tiles_removed_at_the_headline_grids(g, floor):
    """The floors are the ones the change was proposed with.  Counted here: 0.08889 at 13 x 13, 0.04931 at 26 x 26 and 0.025148 at 52 x 52
    (306 of 12168 K tiles).  In plain mask9 order the corners sit between edge classes and 52 x 52 gives 304 of 12168 = 0.024984, under its
    floor; with the masks of fewer live taps first the four corners pair among themselves."""
    got = k_tiles_removed(g)
    ideal = 1.0 - ((3 * g - 2) / (3.0 * g)) ** 2
    print(f"grid {g}: K tiles removed {got:.4f} (raster positions {k_tiles_removed(g, sort=False):.4f}, every padding product {ideal:.4f})")
    assert floor <= got <= ideal + 1e-12


def test_k_tiles_removed_at_52_exact_count():
    """52 x 52, two positions per 64-row tile: 100 edge pairs and the two corner pairs each lose 3 of 9 taps."""
    assert abs(k_tiles_removed(52) - 306.0 / (9 * 1352)) < 1e-12


def test_library_table_gives_the_same_count():
    """The count above from the library's own table at 13 x 13 (the restatement sorts for itself)."""
    _, _, mask = border_order(13, 13, 13, 13, 1)
    live = np.bitwise_or.reduce(np.repeat(mask.astype(np.int64), 32)[: (13 * 13 * 32 // 64) * 64].reshape(-1, 64), axis=1)
    tail = np.repeat(mask.astype(np.int64), 32)[(13 * 13 * 32 // 64) * 64:]
    walked = sum(bin(int(m)).count("1") for m in live) + (bin(int(np.bitwise_or.reduce(tail))).count("1") if len(tail) else 0)
    n_tiles = len(live) + (1 if len(tail) else 0)
    assert abs((1.0 - walked / (9.0 * n_tiles)) - k_tiles_removed(13)) < 1e-12
