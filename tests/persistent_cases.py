"""What tests/test_persistent_walk_host.py and tests/test_persistent_walk_gpu.py share: the cases on which a workgroup of a persistent
kernel walks THREE tiles, their geometry from y3_persistent_grid (the launchers' own formulas), the map from an output element to its tile,
workgroup and walk index, the inputs, and the CPU references of the wrap images computed once per process and left read-only.

The seven persistent kernels (a fixed grid of workgroups, tile += grid): the fused YOLOv3-tiny stem in fp32 / bf16 / fp16
(csrc/conv_tiny_stem.hip), the fused YOLOv3 stem in fp32 and in bf16 / fp16 (csrc/conv_stem.hip), the weight-resident 3x3 conv in fp32
(csrc/conv_res_f32.hip, tile id 33) and in bf16 / fp16 (csrc/conv_res_16bit.h, 16-bit tile id 32).  Each overlaps the next tile's fetch with
the current tile's arithmetic; the third tile of a walk is the first to re-enter patch buffer 0 after it was read, the first behind two
rotations of the look-ahead registers, and the first whose last iteration follows two full ones.

The cases are fixed constants sized for the 256 compute units of an MI355X.  Every case must hold three conditions on the device it runs
on (check_conditions): the longest walk is at least 3 tiles, the shortest is shorter than the longest (workgroups of one launch with
different trip counts), and the stride of a walk is no multiple of the tiles per image (a workgroup's successive tiles change their position
in the image -- border, interior, ragged edge -- as well as the image).

Wrap images: the images whose results the GPU test holds against the CPU reference -- images 0 and 1, the images that hold tiles
stride - 1, stride, 2 stride - 1 and 2 stride (where the first and second walk rounds end and the second and third begin), each with the
image before and the image after it, and the last image.  Images are independent, so the reference is computed for these alone."""
from collections import namedtuple

import numpy as np

from yolo_v3_tf2_amd import _lib

N_CUS = 256          # the compute units the cases are sized for

# family: which kernel; fmt: the plan's format; kind: Y3_PERSISTENT_*; canvas: (H, W) of the net's input; div: canvas / the persistent
# launch's output grid; tile: its (rows, columns) of output pixels (TH x TW of the kernel); slices: output-channel slices (Cout / 64 of
# the weight-resident convs, 1 otherwise); shape: (cin, cout) of the weight-resident chain, None otherwise
Case = namedtuple("Case", "name family fmt kind canvas B div tile slices shape")

_K = _lib
CASES = [
    # fused tiny stem: canvas 96 x 160, pool 1 is 24 x 40 in tiles of 4 x 8 -> 30 per image; 86 images = 2,580 tiles on 1,024 workgroups
    Case("tiny_f32", "tiny", "f32", _K.Y3_PERSISTENT_TINY_STEM, (96, 160), 86, 4, (4, 8), 1, None),
    Case("tiny_bf16", "tiny", "bf16", _K.Y3_PERSISTENT_TINY_STEM, (96, 160), 86, 4, (4, 8), 1, None),
    Case("tiny_f16", "tiny", "f16", _K.Y3_PERSISTENT_TINY_STEM, (96, 160), 86, 4, (4, 8), 1, None),
    # 16-bit weight-resident conv, tiles of 4 x 32: 40^2 -> 10 x 2 = 20 per image (ragged last column), 640 tiles on 256; 33^2 -> 9 x 2 = 18
    # (ragged row and column), 324 tiles on 128 per slice; 70^2 -> 18 x 3 = 54 (ragged row and column), 324 tiles on 128 per slice
    Case("res16_bf16_c32_n64_s40", "res16", "bf16", _K.Y3_PERSISTENT_RES_16, (40, 40), 32, 1, (4, 32), 1, (32, 64)),
    Case("res16_bf16_c64_n128_s33", "res16", "bf16", _K.Y3_PERSISTENT_RES_16, (33, 33), 18, 1, (4, 32), 2, (64, 128)),
    Case("res16_bf16_c32_n128_s70", "res16", "bf16", _K.Y3_PERSISTENT_RES_16, (70, 70), 6, 1, (4, 32), 2, (32, 128)),
    Case("res16_f16_c32_n64_s40", "res16", "f16", _K.Y3_PERSISTENT_RES_16, (40, 40), 32, 1, (4, 32), 1, (32, 64)),
    Case("res16_f16_c64_n128_s33", "res16", "f16", _K.Y3_PERSISTENT_RES_16, (33, 33), 18, 1, (4, 32), 2, (64, 128)),
    Case("res16_f16_c32_n128_s70", "res16", "f16", _K.Y3_PERSISTENT_RES_16, (70, 70), 6, 1, (4, 32), 2, (32, 128)),
    # fp32 weight-resident conv (tile id 33), tiles of 8 x 16: 41^2 -> 6 x 3 = 18 per image, ragged both ways; 648 tiles on 256, 324 on 128 per slice
    Case("res32_n64_s41", "res32", "f32", _K.Y3_PERSISTENT_RES_F32, (41, 41), 36, 1, (8, 16), 1, (32, 64)),
    Case("res32_n128_s41", "res32", "f32", _K.Y3_PERSISTENT_RES_F32, (41, 41), 18, 1, (8, 16), 2, (32, 128)),
    # fused YOLOv3 stem: canvas 96 x 160, conv1's output is 48 x 80 in tiles of 8 x 16 -> 30 per image; fp32 660 tiles on 256 (with the
    # in-stem 1x1 third layer), 16-bit 1,290 tiles on 512
    Case("stem_f32", "stem", "f32", _K.Y3_PERSISTENT_STEM_F32, (96, 160), 22, 2, (8, 16), 1, None),
    Case("stem_bf16", "stem", "bf16", _K.Y3_PERSISTENT_STEM_16, (96, 160), 43, 2, (8, 16), 1, None),
    Case("stem_f16", "stem", "f16", _K.Y3_PERSISTENT_STEM_16, (96, 160), 43, 2, (8, 16), 1, None),
]
BY_NAME = {c.name: c for c in CASES}
RES_CASES = [c for c in CASES if c.family in ("res16", "res32")]
# one case per kernel family for the graph capture
GRAPH_CASES = [BY_NAME[n] for n in ("tiny_bf16", "res16_bf16_c64_n128_s33", "res32_n128_s41", "stem_f32", "stem_f16")]
IMAGE_SEED = {"tiny": 41, "res16": 52, "res32": 61}      # the fused YOLOv3 stems take the seeds of the tests whose programs they run
GENERIC_TILE = {"res32": lambda cin: 11, "res16": lambda cin: 5 if cin == 32 else 10}      # the generic tile of the same MFMA shape and k order
RESIDENT_TILE = {"res32": 33, "res16": 32}

# grid: workgroups of the launch; stride: of a walk, in tiles (grid / slices); longest / shortest: walk lengths in tiles; chunk: images per
# call of the walk-invariance check (stride // tiles_per_image: a chunk's launch has no more tiles than workgroups per slice, so every
# workgroup has at most one); wrap: the wrap images, sorted
Geometry = namedtuple("Geometry", "tiles_y tiles_x tiles_per_image n_tiles grid stride longest shortest chunk wrap")


def geometry(case, n_cus=N_CUS):
    H, W = case.canvas
    th, tw = case.tile
    ty, tx = -(-(H // case.div) // th), -(-(W // case.div) // tw)
    tpi = ty * tx
    n = case.B * tpi
    grid = _lib.load().y3_persistent_grid(case.kind, n, case.slices, n_cus)
    assert grid > 0 and grid % case.slices == 0, (case.name, grid)
    stride = grid // case.slices
    shortest = n // stride
    longest = shortest + (n % stride != 0)
    return Geometry(ty, tx, tpi, n, grid, stride, longest, shortest, stride // tpi, wrap_images(case.B, tpi, stride))


def wrap_images(B, tiles_per_image, stride):
    w = {0, 1, B - 1}
    for t in (stride - 1, stride, 2 * stride - 1, 2 * stride):
        m = t // tiles_per_image
        w.update((m - 1, m, m + 1))
    return sorted(i for i in w if 0 <= i < B)


def check_conditions(case, g):
    """The three conditions of a case on the device whose compute units gave `g`; the chunk of the invariance check really is walk-free."""
    assert g.longest >= 3, (case.name, g)
    assert g.shortest < g.longest, (case.name, g)
    assert g.stride % g.tiles_per_image != 0, (case.name, g)
    assert g.chunk >= 1 and g.chunk * g.tiles_per_image <= g.stride, (case.name, g)


def describe(case, g):
    n_long = g.n_tiles % g.stride
    return (f"{case.name}: {case.B} images x {g.tiles_per_image} tiles = {g.n_tiles} tiles, grid {g.grid} ({case.slices} slice(s), stride {g.stride}): "
            f"{n_long} workgroups per slice walk {g.longest}, {g.stride - n_long} walk {g.shortest}; chunks of {g.chunk} images; wrap images {g.wrap}")


def locate(case, g, image, oy, ox):
    """Output pixel (oy, ox) of `image` in the persistent launch's output grid -> (tile, workgroup of its slice, walk index: 0 = the
    workgroup's first tile).  Workgroup w of a weight-resident launch is (slice w % slices, workgroup w // slices of the slice)."""
    th, tw = case.tile
    tile = image * g.tiles_per_image + (oy // th) * g.tiles_x + ox // tw
    return tile, tile % g.stride, tile // g.stride


def walk_index_map(case, g):
    """[B, rows, columns] int: the walk index of every output pixel of the persistent launch (for reading a failure: which elements sit in
    second and third tiles)."""
    H, W = case.canvas[0] // case.div, case.canvas[1] // case.div
    th, tw = case.tile
    t = (np.arange(H)[:, None] // th) * g.tiles_x + np.arange(W)[None, :] // tw
    return (np.arange(case.B)[:, None, None] * g.tiles_per_image + t[None]) // g.stride


# ---------------------------------------------------------------------------------------------- programs, weights, inputs
def _res_chain(family, cin, cout):
    if family == "res32":      # tests/test_gpu_parity.py::test_f32_weight_resident_conv_bit_identical_to_generic_tiles
        chain = [dict(filters=cout, size=3), dict(filters=32, size=1), dict(filters=cout, size=3, shortcut=-3),
                 dict(filters=32, size=1, act="linear"), dict(filters=cout, size=3, bn=False, act="linear"), dict(filters=32, size=1)]
        heads = [dict(filters=64, size=3), dict(filters=128, size=3), dict(filters=64, size=3, bn=False, act="linear")]
    else:                      # tests/test_gpu_parity.py::test_bf16_weight_resident_3x3_matches_oracle_and_generic_tiles
        chain = [dict(filters=cout, size=3), dict(filters=cin, size=1), dict(filters=cout, size=3, shortcut=-3),
                 dict(filters=cin, size=1, act="linear"), dict(filters=cout, size=3, bn=False, act="linear")]
        heads = [dict(filters=64, size=1), dict(filters=32, size=1), dict(filters=64, size=1, bn=False, act="linear")]
    return chain, heads


_inputs = {}


def inputs(case):
    """-> (program, weights, input batch fp32 -- exact in the plan's format where the net reads it as 16-bit), cached per (family, fmt, shape)."""
    fmt_key = case.fmt if case.family == "res16" else "" if case.family == "tiny" else "f32" if case.fmt == "f32" else "16"
    key = (case.family, fmt_key, case.shape, case.B, case.canvas)
    if key in _inputs:
        return _inputs[key]
    from oracle import oracle as O
    from tests.f16_oracle import round_f16
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    H, W = case.canvas
    if case.family == "tiny":
        from tests import tiny_stem_cases as T
        p, w, _, _ = T.stem_inputs("s32_b1")            # the program, SEED weights and identity heads of that file, "plain"
        x = np.random.default_rng(IMAGE_SEED["tiny"]).random((case.B, H, W, 3), dtype=np.float32)
    elif case.family in ("res16", "res32"):
        cin, cout = case.shape
        seed = IMAGE_SEED[case.family]
        p = mini_program(cin, *_res_chain(case.family, cin, cout))
        w = synthetic_weights(p, seed=seed)
        x = np.random.default_rng(seed).standard_normal((case.B, H, W, cin)).astype(np.float32)
        x = {"f32": lambda a: a, "bf16": O.round_bf16, "f16": round_f16}[case.fmt](x)
    elif case.fmt == "f32":    # tests/test_gpu_parity.py::test_fused_stem_matches_oracle_and_the_two_launch_form: the 1x1 third layer is in the stem
        p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2), dict(filters=32, size=1),
                             dict(filters=64, size=3, shortcut=-3)],
                         [dict(filters=32, size=1), dict(filters=32, size=1), dict(filters=32, size=1)])
        w = synthetic_weights(p, seed=11)
        x = np.random.default_rng(11).random((case.B, H, W, 3), dtype=np.float32)
    else:                      # tests/f16_stem_cases.py: conv0, conv1 and three identity heads, in both 16-bit formats
        from tests import f16_stem_cases as F
        p = F.stem_program()
        w = dict(synthetic_weights(p, seed=F.SEED))
        for i in (2, 3, 4):
            w[f"conv{i}.w"] = np.eye(64, dtype=np.float32).reshape(1, 1, 64, 64)
            w[f"conv{i}.bias"] = np.zeros(64, np.float32)
        x = np.random.default_rng(F.SEED).random((case.B, H, W, 3), dtype=np.float32)
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    _inputs[key] = (p, w, x)
    return _inputs[key]


def probes(case, p):
    """The stored tensors the GPU test reads back beside the net's outputs (weight-resident cases: the 3x3 outputs in bf16 and fp32, every
    stored conv output in fp16, as the existing tests of those kernels)."""
    if case.family not in ("res16", "res32"):
        return []
    if case.fmt == "f16":
        return [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    return [o.dst for o in p.conv_ops() if o.size == 3 and o.dst not in p.outputs]


# ---------------------------------------------------------------------------------------------- references of a subset of the images
def reference(case, images):
    """The CPU reference of `case` on the images `images` (a list of indices) alone, by family and format:
      tiny        {"f64", "bf16", "bf16_s32", "f16", "f16_s32"}: pool 1's tensor, the chains of tests/tiny_stem_cases.py
      res16 bf16  (outputs, {probe tensor: values}) of the bf16-emulating oracle
      res16 f16   None: that test recomputes every 3x3 launch from the device's own stored input (tests/test_f16_gpu.py)
      res32, stem f32   the outputs of the fp32 oracle
      stem bf16   head 0 of the bf16-emulating oracle = conv1's stored output
      stem f16    {"oracle", "oracle64", "restated"}: conv1's stored output, the three pipelines of tests/f16_stem_cases.py"""
    from oracle import oracle as O
    p, w, x = inputs(case)
    xs = np.ascontiguousarray(x[list(images)])
    if case.family == "tiny":
        from tests import tiny_stem_cases as T
        from tests.f16_oracle import f16_emulation, round_f16
        out = {"f64": T._chain(O, p, w, xs, True, None)}
        out["bf16"], out["bf16_s32"] = T._chain(O, p, w, xs, True, O.round_bf16), T._chain(O, p, w, xs, False, O.round_bf16)
        with f16_emulation():
            out["f16"], out["f16_s32"] = T._chain(O, p, w, xs, True, round_f16), T._chain(O, p, w, xs, False, round_f16)
        return out
    if case.family == "res16":
        return O.forward(p, w, xs, bf16=True, keep=set(probes(case, p))) if case.fmt == "bf16" else None
    if case.fmt == "f32":
        return O.forward(p, w, xs)
    if case.fmt == "bf16":
        return O.forward(p, w, xs, bf16=True)[0]
    from tests import f16_stem_cases as F
    from tests.f16_oracle import f16_emulation, round_f16
    from tests.helpers import oracle_launch
    c0, c1 = p.conv_ops()[0], p.conv_ops()[1]
    out = {}
    with f16_emulation():
        for name, acc64 in (("oracle", False), ("oracle64", True)):
            y0 = round_f16(oracle_launch(O, c0, w, {p.input_tensor: xs}.__getitem__, acc64=acc64))
            out[name] = round_f16(oracle_launch(O, c1, w, {c0.dst: y0}.__getitem__, acc64=acc64, bf16_weights=True))
        out["restated"] = round_f16(oracle_launch(O, c1, w, {c0.dst: F.conv0_restated(w, xs)}.__getitem__, acc64=False, bf16_weights=True))
    return out


def _freeze(r):
    if isinstance(r, np.ndarray):
        r.setflags(write=False)
    elif isinstance(r, dict):
        for v in r.values():
            _freeze(v)
    elif isinstance(r, (list, tuple)):
        for v in r:
            _freeze(v)
    return r


_refs = {}


def wrap_reference(case):
    """reference(case, the wrap images at 256 compute units), computed once per process, read-only.  (The wrap images of another device
    are other images: the GPU test asks reference() itself then.)"""
    if case.name not in _refs:
        _refs[case.name] = _freeze(reference(case, geometry(case).wrap))
    return _refs[case.name]


# ---------------------------------------------------------------------------------------------- the caps of the 16-bit tiny-stem cases
# tests/tiny_stem_cases.py's rule on these images: the fraction of pool-1 elements at which the device may differ from the rounded double-sum
# chain at all (differ), and by more than the element's own ulp + 1e-5 of the tensor's magnitude (beyond), is TWICE what the fp32-sum chain
# reaches against the double-sum chain on the wrap images of the case -- two pipelines that differ in nothing but the order of their sums.
# That file's CAPS cannot be used: on these images the fp16 reference alone is above half of them.  tests/test_persistent_walk_host.py
# measures the figures again and asserts the factor.  Measured (NumPy and the oracle library; images default_rng(41), 86 x 96 x 160 x 3,
# wrap images [0, 1, 33, 34, 35, 67, 68, 69, 85]), rounded up in the fourth digit:
#                  differ      beyond      worst (of the per-element bound, <= 1.0 as in that file)
#   bf16           2.641e-4    2.171e-5    0.493
#   f16            4.149e-3    2.749e-4    0.494
# (On images [0, 1, 33, 34, 35, 68, 69, 85] alone the same chains give 2.889e-4 / 2.441e-5 and 4.224e-3 / 3.011e-4.)
TINY_MEASURED = {"bf16": (2.641e-4, 2.171e-5), "f16": (4.149e-3, 2.749e-4)}
TINY_CAPS = {fmt: (2.0 * d, 2.0 * b) for fmt, (d, b) in TINY_MEASURED.items()}      # (differ, beyond)
