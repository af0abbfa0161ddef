"""Inputs of the multi-label tests (tests/test_multilabel_host.py, tests/test_multilabel_gpu.py): the smallest head grids at which the
candidates kernel can still go wrong -- none of them the workload's own -- with random and planted logits.

Grids {2,4,8} square (N = 252) and {(2,3),(4,6),(8,12)} (N = 378: rectangular, scale boundaries off the 64-box workgroups); class
counts 1, 2, 3, 5, 80, 81 (the four lanes of a box with 0..3 leftover classes, fewer classes than lanes); batches of 1, 3 and 7 (at
7 a 64-box workgroup of the 2x2 scale, 12 boxes per image, straddles six images)."""
import numpy as np

SQUARE = ((2, 2), (4, 4), (8, 8))
RECT = ((2, 3), (4, 6), (8, 12))
GRIDS = {"square": SQUARE, "rect": RECT}
CLASS_COUNTS = (1, 2, 3, 5, 80, 81)
BATCHES = (1, 3, 7)
S_RANDOM = 0.1
BLOCK = 64          # boxes per workgroup of the decode and candidates kernels


def boxes_per_image(grid_hw):
    return sum(3 * gh * gw for gh, gw in grid_hw)


def scale_offsets(grid_hw):
    off, out = 0, []
    for gh, gw in grid_hw:
        out.append(off)
        off += 3 * gh * gw
    return out


def anchors_table():
    """The COCO anchors over 416 (datasets/coco2012/anchors.txt), smallest scale last as the heads are ordered."""
    a = np.array([[116, 90], [156, 198], [373, 326], [30, 61], [62, 45], [59, 119], [10, 13], [16, 30], [33, 23]], np.float32)
    return (a / np.float32(416)).reshape(3, 3, 2)


def random_grids(grid_hw, nc, B, seed=0):
    """Objectness ~ N(0, 2), classes ~ N(-1, 2), box fields ~ N(0, 1): at S = 0.1 some but never all pairs of an image are candidates."""
    rng = np.random.default_rng([seed, nc, B, len(grid_hw[0]) + grid_hw[0][1]])
    grids = []
    for gh, gw in grid_hw:
        g = rng.standard_normal((B, gh, gw, 3, 5 + nc)).astype(np.float32)
        g[..., 4] = (g[..., 4] * 2.0).astype(np.float32)
        g[..., 5:] = (g[..., 5:] * 2.0 - 1.0).astype(np.float32)
        grids.append(np.ascontiguousarray(g))
    return grids


def planted_grids(grid_hw, nc, B, pairs, fill=-20.0):
    """All logits `fill` (objectness and classes; box fields 0) except the pairs (b, n, c) of `pairs`: objectness of box n and
    class c of it +20.  At S = 0.1 exactly the planted pairs are candidates (sigmoid(20)^2 ~ 1, sigmoid(20) sigmoid(-20) ~ 2e-9);
    at S = -1 all pairs are."""
    offs = scale_offsets(grid_hw)
    grids = [np.zeros((B, gh, gw, 3, 5 + nc), np.float32) for gh, gw in grid_hw]
    for g in grids:
        g[..., 4:] = fill
    for b, n, c in pairs:
        s = max(i for i, o in enumerate(offs) if n >= o)
        flat = grids[s].reshape(B, -1, 5 + nc)
        flat[b, n - offs[s], 4] = 20.0
        flat[b, n - offs[s], 5 + c] = 20.0
    return grids


def boundary_pairs(grid_hw, nc, B):
    """The pairs on both sides of every boundary the kernel knows: the first and the last pair of every image, the last pair before and
    the first pair behind every scale boundary, and the same at every 64-box workgroup boundary (workgroups cover one scale across the
    batch: box g = b * per_img + r of the scale starts a workgroup when g % 64 == 0)."""
    offs, N = scale_offsets(grid_hw), boxes_per_image(grid_hw)
    pairs = set()
    for b in range(B):
        pairs |= {(b, 0, 0), (b, N - 1, nc - 1)}
        for o in offs[1:]:
            pairs |= {(b, o - 1, nc - 1), (b, o, 0)}
    for s, (gh, gw) in enumerate(grid_hw):
        per = 3 * gh * gw
        for g in range(BLOCK, B * per, BLOCK):
            for gi, c in ((g - 1, nc - 1), (g, 0)):
                pairs.add((gi // per, offs[s] + gi % per, c))
    return sorted(pairs)


def first_pairs(grid_hw, nc, b, count):
    """The first `count` pairs of image b in (n, c) order, spread: every 7th pair of the image, wrapped."""
    total = boxes_per_image(grid_hw) * nc
    step = 7 if total % 7 else 5
    ks = sorted({(i * step) % total for i in range(count)})
    assert len(ks) == count
    return [(b, k // nc, k % nc) for k in ks]


# A product tie found once by search (see test_multilabel_host.test_product_tie): conf * P_LO and conf * P_HI round to the same fp32
# although P_LO < P_HI.  Hex so that no decimal rounding stands between the file and the bits.
TIE_CONF = float.fromhex("0x1.607c18p-1")     # ~0.6884
TIE_P_LO = float.fromhex("0x1.8e416ap-2")     # ~0.3889
TIE_P_HI = float.fromhex("0x1.8e416cp-2")     # the next fp32 above it


def net_input(S=64, B=2, seed=1234):
    return np.random.default_rng(seed).random((B, S, S, 3), dtype=np.float32)
