"""Persistent kernels on walks of three tiles, host side, no GPU (tests/persistent_cases.py; tests/test_persistent_walk_gpu.py runs the
cases): y3_persistent_grid pinned to the grids the launchers have always launched, the three conditions of every case at 256 compute
units with the wrap images they imply, the basis of the caps the 16-bit tiny-stem cases are held to, and the per-image independence of
the references (the reason a reference of the wrap images alone can judge a batch of 86)."""
import os
import re

import numpy as np
import pytest

from tests import persistent_cases as P
from yolo_v3_tf2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in P.CASES]


def _grid(kind, n_tiles, slices=1, n_cus=256):
    return _lib.load().y3_persistent_grid(kind, n_tiles, slices, n_cus)


def test_grid_query_is_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "y3.h")).read(), flags=re.S)
    assert "y3_persistent_grid" in _lib.SYMBOLS and re.search(r"\by3_persistent_grid\s*\(", header)
    assert hasattr(_lib.load(), "y3_persistent_grid")
    kinds = [_lib.Y3_PERSISTENT_TINY_STEM, _lib.Y3_PERSISTENT_STEM_F32, _lib.Y3_PERSISTENT_STEM_16, _lib.Y3_PERSISTENT_RES_F32,
             _lib.Y3_PERSISTENT_RES_16]
    assert kinds == [0, 1, 2, 3, 4]
    for k, name in zip(kinds, ("TINY_STEM", "STEM_F32", "STEM_16", "RES_F32", "RES_16")):
        assert re.search(r"\bY3_PERSISTENT_%s = %d\b" % (name, k), header), name


def test_grids_at_256_compute_units_are_the_launchers_own():
    """The grids the five launchers computed inline before they shared these formulas: min(tiles, 4 CUs) for the tiny stem, min(tiles, CUs)
    and min(tiles, 2 CUs) for the fp32 and 16-bit stems, min(tiles, max(1, CUs / slices)) * slices for the weight-resident convs."""
    T, S32, S16, R32, R16 = range(5)
    assert _grid(T, 150) == 150 and _grid(T, 2580) == 1024 and _grid(T, 1024) == 1024 and _grid(T, 1025) == 1024
    assert _grid(S32, 660) == 256 and _grid(S32, 255) == 255
    assert _grid(S16, 1290) == 512 and _grid(S16, 338) == 338
    for R in (R32, R16):
        assert _grid(R, 640, 1) == 256
        assert _grid(R, 324, 2) == 256
        assert _grid(R, 10, 4) == 40
        assert _grid(R, 60, 1) == 60 and _grid(R, 36, 2) == 72
        assert _grid(R, 5, 512) == 512              # more slices than compute units: one workgroup per slice
    assert _grid(T, 21632) == 1024                  # YOLOv3-tiny at 64 x 416^2: 21 tiles per workgroup
    assert _grid(T, 2580, 1, 304) == 1216 and _grid(R16, 324, 2, 304) == 304
    for bad in ((T, 0, 1, 256), (T, -3, 1, 256), (T, 100, 0, 256), (T, 100, 1, 0), (T, 100, 1, -1), (T, 100, 2, 256), (S32, 100, 2, 256),
                (S16, 100, 3, 256), (5, 100, 1, 256), (-1, 100, 1, 256), (R32, 100, -2, 256), (R16, 1 << 31, 1, 256)):
        assert _grid(*bad) <= 0, bad


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_case_conditions_and_wrap_images_at_256_compute_units(case):
    g = P.geometry(case, 256)
    print(P.describe(case, g))
    P.check_conditions(case, g)
    assert g.longest == 3 and g.shortest == 2
    # the wrap images, derived once more from the walk: the images of the last tile of the first and second round and of the first tile of
    # the second and third, each with both neighbours; the first two images and the last
    want = {0, 1, case.B - 1}
    for t in (g.stride - 1, g.stride, 2 * g.stride - 1, 2 * g.stride):
        _, wg, walk = P.locate(case, g, t // g.tiles_per_image, *_first_pixel(case, g, t))
        assert (wg, walk) == (t % g.stride, t // g.stride) and wg in (0, g.stride - 1)
        m = t // g.tiles_per_image
        want |= {m - 1, m, m + 1}
    assert g.wrap == sorted(i for i in want if 0 <= i < case.B) and 6 <= len(g.wrap) <= 9
    # they hold tiles of every walk index, and of workgroups with the long and with the short walk
    walks = P.walk_index_map(case, g)
    assert sorted(np.unique(walks[g.wrap])) == [0, 1, 2] and walks.max() == 2
    tiles = np.concatenate([np.arange(i * g.tiles_per_image, (i + 1) * g.tiles_per_image) for i in g.wrap])
    long_wg = (tiles % g.stride) < g.n_tiles % g.stride
    assert long_wg.any() and not long_wg.all()
    assert case.B * int(np.prod(_input_shape(case))) * 4 <= 16 << 20, "the largest input is 16 MB"


def _first_pixel(case, g, tile):
    r = tile % g.tiles_per_image
    return (r // g.tiles_x) * case.tile[0], (r % g.tiles_x) * case.tile[1]


def _input_shape(case):
    return case.canvas + (3 if case.shape is None else case.shape[0],)


def test_tiny_case_is_the_one_written_down():
    """96 x 160: 30 tiles per image, 2,580 tiles on 1,024 workgroups, 532 of them with three tiles; chunks of 34 images; the wrap images."""
    for name in ("tiny_f32", "tiny_bf16", "tiny_f16"):
        g = P.geometry(P.BY_NAME[name], 256)
        assert (g.tiles_y, g.tiles_x, g.n_tiles, g.grid, g.n_tiles % g.stride, g.chunk) == (6, 5, 2580, 1024, 532, 34)
        assert g.wrap == [0, 1, 33, 34, 35, 67, 68, 69, 85]
    for name, tpi, n, stride, chunk in (("res16_bf16_c32_n64_s40", 20, 640, 256, 12), ("res16_f16_c64_n128_s33", 18, 324, 128, 7),
                                        ("res16_bf16_c32_n128_s70", 54, 324, 128, 2), ("res32_n64_s41", 18, 648, 256, 14),
                                        ("res32_n128_s41", 18, 324, 128, 7), ("stem_f32", 30, 660, 256, 8), ("stem_bf16", 30, 1290, 512, 17),
                                        ("stem_f16", 30, 1290, 512, 17)):
        g = P.geometry(P.BY_NAME[name], 256)
        assert (g.tiles_per_image, g.n_tiles, g.stride, g.chunk) == (tpi, n, stride, chunk), name


def test_tiny_caps_are_twice_what_the_reference_alone_reaches():
    """On the wrap images of the tiny-stem case: the fp32-sum chain against the double-sum chain, per 16-bit format -- the fraction of pool-1
    elements that differ at all and by more than the element's own ulp + 1e-5 of the tensor's magnitude.  The case's caps are twice these
    figures (the reference alone stays within half of them, and they are no wider); no element passes the per-element bound.  The caps of
    tests/tiny_stem_cases.py would not do: the fp16 figures here are above half of them."""
    from tests import tiny_stem_cases as T
    r = P.wrap_reference(P.BY_NAME["tiny_bf16"])
    assert r["f64"].shape == (9, 24, 40, 32)
    for fmt in T.FORMATS:
        differ, beyond, worst = T.compare(fmt, r[fmt + "_s32"], r[fmt])
        print(f"tiny stem {fmt}, wrap images, fp32 sums against double sums: differ {differ:.4e}  beyond one ulp {beyond:.4e}  worst {worst:.3f} of the bound")
        assert worst <= 1.0
        for k, v in enumerate((differ, beyond)):
            assert P.TINY_CAPS[fmt][k] == 2.0 * P.TINY_MEASURED[fmt][k]
            assert v <= P.TINY_CAPS[fmt][k] / 2
            assert 0.999 * P.TINY_MEASURED[fmt][k] <= v <= P.TINY_MEASURED[fmt][k], (fmt, k, v, "the constant is the measured figure, rounded up")
    assert T.compare("f16", r["f16_s32"], r["f16"])[0] > T.CAPS["f16"][0] / 2, "else that file's caps would have served"


def test_f16_stem_reference_alone_stays_within_half_of_the_existing_caps():
    """The fp16 fused YOLOv3 stem on its wrap images: the three reference-alone comparisons of tests/test_f16_stem_host.py stay within half
    of that file's caps, so the walk case is held to those caps as they are."""
    from tests import f16_stem_cases as F
    from tests.f16_oracle import round_f16
    from tests.test_f16_stem_host import STEM_BEYOND_CAP, STEM_DIFFER_CAP
    r = P.wrap_reference(P.BY_NAME["stem_f16"])
    scale = float(np.abs(r["oracle"]).max())
    assert all(np.isfinite(a).all() and np.array_equal(round_f16(a), a) for a in r.values())
    for what, a, b in (("restated vs oracle", r["restated"], r["oracle"]), ("oracle, double vs fp32 sums", r["oracle64"], r["oracle"]),
                       ("restated vs oracle with double sums", r["restated"], r["oracle64"])):
        frac, beyond, worst = F.compare(a, b, scale)
        print(f"f16 stem wrap images, {what}: {frac:.3e} differ, {beyond:.3e} beyond their own ulp, worst {worst:.3f}")
        assert frac <= STEM_DIFFER_CAP / 2 and beyond <= STEM_BEYOND_CAP / 2 and worst <= 1.0, (what, frac, beyond, worst)


def _leaves(r):
    if isinstance(r, np.ndarray):
        return [r]
    if isinstance(r, dict):
        return [a for k in sorted(r) for a in _leaves(r[k])]
    return [a for v in r for a in _leaves(v)]


@pytest.mark.parametrize("case", [c for c in P.CASES if not (c.family == "res16" and c.fmt == "f16")], ids=lambda c: c.name)
def test_reference_of_one_image_alone_is_its_slice_of_the_subset_run(case):
    """Images are independent in every reference: the third wrap image alone (image 33 of the tiny case) gives, bit for bit, its slice of
    the reference of all wrap images.  (The fp16 weight-resident cases have no reference of their own: each launch is recomputed from the
    device's stored input.)"""
    g = P.geometry(case, 256)
    k = 2
    if case.family == "tiny":
        assert g.wrap[k] == 33
    whole, one = _leaves(P.wrap_reference(case)), _leaves(P.reference(case, [g.wrap[k]]))
    assert len(whole) == len(one) > 0
    for a, b in zip(whole, one):
        assert not a.flags.writeable and a.shape[0] == len(g.wrap) and b.shape[0] == 1
        assert np.array_equal(a[k:k + 1], b)
