"""What tests/test_tiny_stem_host.py and tests/test_tiny_stem_gpu.py share: the program, weights and images of the fused tiny stem's cases
(csrc/conv_tiny_stem.hip; include/y3.h, y3_net_set_tiny_stem_fusion), the references of a case computed once per process and left
read-only, the comparison, and the caps the device is held to with the figures they come from.

The program: conv0 (3x3 / 1, 3 -> 16, BN, leaky), max-pool 2x2 / 2, conv1 (3x3 / 1, 16 -> 32, BN, leaky), max-pool 2x2 / 2, then two raw
1x1 heads 32 -> 64 without BN, linear, with the weights [I_32 | 0] and no bias: their fp32 grids are pool 1's stored values bit for bit
(channels 32 .. 63 are zero), and Cin 32 -> Cout 64 has a BK = 32 tile in both 16-bit modes.  NumPy and the oracle library only."""
import numpy as np

from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16
from yolo_v3_tf2_amd.graph import Program, _Builder, _lower
from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref

# (canvas (H, W), images).  32 x 32, one image: the 8 x 8 output is two tiles of 4 x 8, every border in them; 64 x 96, three images:
# non-square, image boundaries; 160 x 128, two images: 40 tiles per image.
CASES = {"s32_b1": ((32, 32), 1), "r64x96_b3": ((64, 96), 3), "r160x128_b2": ((160, 128), 2)}
# plain: synthetic weights, the image in [0, 1).  signs: the BN gamma of both convs of both signs and zero with shifts (beta) of order -1, so
# that whole pooling windows are negative (a maximum that starts from 0, or a pool taken before leaky, shows).  img255: the image x 255.
VARIANTS = ("plain", "signs", "img255")
VARIANT_CASE = "r64x96_b3"
GPU_CASES = [(c, "plain") for c in CASES] + [(VARIANT_CASE, v) for v in VARIANTS[1:]]
SEED = 29
FORMATS = ("bf16", "f16")

# The caps of the 16-bit device tests: the fraction of pool-1 elements at which the device may differ from the rounded double-sum chain at
# all (differ), and by more than the element's own ulp + 1e-5 of the tensor's magnitude (beyond).  Each is TWICE the largest figure that the
# fp32-sum oracle chain reaches against the double-sum chain over GPU_CASES -- two pipelines that differ in nothing but the order of their
# sums; the project's rule is that the reference alone stays within half the cap.  tests/test_tiny_stem_host.py measures the figures again
# and asserts the factor.  Measured (NumPy and the oracle library), (differ, beyond) per case and format:
#                          bf16                      f16
#   s32_b1 / plain         0         0               4.883e-4  0
#   r64x96_b3 / plain      2.170e-4  0               3.825e-3  5.425e-5
#   r160x128_b2 / plain    9.766e-5  0               3.345e-3  1.831e-4
#   r64x96_b3 / signs      2.713e-5  0               9.494e-4  0
#   r64x96_b3 / img255     4.883e-4  5.425e-5        2.848e-3  5.425e-5
#   largest                4.883e-4  5.425e-5        3.825e-3  1.831e-4
LARGEST = {"bf16": (4.883e-4, 5.426e-5), "f16": (3.825e-3, 1.832e-4)}      # the last line, rounded up in the fourth digit
CAPS = {fmt: (2.0 * d, 2.0 * b) for fmt, (d, b) in LARGEST.items()}      # (differ, beyond)
# the per-element bound no element may pass: the element's own ulp + this fraction of the tensor's magnitude
WORST = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


def stem_program(second_reader=False):
    """-> (program, pool 1's tensor id).  second_reader: one more head reads conv0's output through a pool of its own (the graph rule's
    "no": conv0's tensor has two readers)."""
    b = _Builder(0, None)
    inp = b.new_tensor(3, 1, "input")

    def conv(x, filters, size, raw=False):
        conf = {"filters": filters, "size": size, "stride": 1, "activation": "linear" if raw else "leaky"}
        if not raw:
            conf["batch_normalize"] = 1
        return b.conv(x, conf, "head" if raw else "body")

    def pool(x):
        return b.maxpool(x, {"size_xy": [2, 2], "stride_xy": [2, 2], "padding": "same"}, "body")

    c0 = conv(inp, 16, 3)
    p0 = pool(c0)
    c1 = conv(p0, 32, 3)
    p1 = pool(c1)
    outs = [conv(p1, 64, 1, raw=True), conv(p1, 64, 1, raw=True)]
    if second_reader:
        outs[1] = conv(pool(c0), 64, 3, raw=True)
    p = Program(b.tensors, b.nodes, [], inp, outs, 0)
    p.conv_nodes = [n for n in b.nodes if n.kind == "conv"]
    _lower(p)
    return p, p1


def stem_inputs(case, variant="plain"):
    """-> (program, weights at the real widths, fp32 image batch, pool 1's tensor id) of a case."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p, p1 = stem_program()
    w = dict(synthetic_weights(p, seed=SEED))
    ident = np.zeros((1, 1, 32, 64), np.float32)
    ident[0, 0, np.arange(32), np.arange(32)] = 1.0
    for i in (2, 3):
        w[f"conv{i}.w"] = ident.copy()
        w[f"conv{i}.bias"] = np.zeros(64, np.float32)
    (H, W), B = CASES[case]
    x = np.random.default_rng(SEED).random((B, H, W, 3), dtype=np.float32)
    if variant == "signs":
        rng = np.random.default_rng(SEED + 1)
        for i, n in ((0, 16), (1, 32)):
            g = w[f"conv{i}.gamma"].copy()
            g[1::3] *= -1.0                     # every third channel a negative scale,
            g[2::3] = 0.0                       # every third a zero one
            w[f"conv{i}.gamma"] = g.astype(np.float32)
            w[f"conv{i}.beta"] = (-1.0 + 0.2 * rng.standard_normal(n)).astype(np.float32)
    elif variant == "img255":
        x = (x * np.float32(255.0)).astype(np.float32)
    else:
        assert variant == "plain", variant
    return p, w, x, p1


def bf16_ulp_elem(a, b):
    """Per element: the spacing of bf16 numbers (8 significand bits) in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


ULP = {"bf16": bf16_ulp_elem, "f16": f16_ulp_elem}


def _chain(O, p, w, x, acc64, rnd):
    """pool 1's tensor from the oracle's layers and maxpool2x2_ref.  rnd None: nothing rounded, fp32 weights; else the rounding of a 16-bit
    pipeline where it stores: conv0 (fp32 weights) rounded, conv1 on rounded weights, rounded."""
    c0, c1 = p.conv_ops()[0], p.conv_ops()[1]
    w1 = dict(w)
    y = O.conv_block(x, w, c0.conv_index, 3, 1, True, True, acc64)
    if rnd:
        y = rnd(y)
        w1[f"conv{c1.conv_index}.w"] = rnd(w[f"conv{c1.conv_index}.w"])
    y = maxpool2x2_ref(y, 2)
    y = O.conv_block(y, w1, c1.conv_index, 3, 1, True, True, acc64)
    if rnd:
        y = rnd(y)
    return np.ascontiguousarray(maxpool2x2_ref(y, 2), np.float32)


_refs = {}


def references(case, variant="plain"):
    """pool 1's tensor [B, H/4, W/4, 32] of a case, read-only: "f32" / "f64" -- nothing rounded, fp32 sums / double sums; "bf16", "f16"
    -- rounded where a pipeline of that format stores, double sums (what the device is compared with); "bf16_s32", "f16_s32" -- the same
    with fp32 sums (the other pipeline of the caps' basis)."""
    key = (case, variant)
    if key not in _refs:
        from oracle import oracle as O
        p, w, x, _ = stem_inputs(case, variant)
        out = {"f32": _chain(O, p, w, x, False, None), "f64": _chain(O, p, w, x, True, None)}
        out["bf16"], out["bf16_s32"] = _chain(O, p, w, x, True, O.round_bf16), _chain(O, p, w, x, False, O.round_bf16)
        with f16_emulation():
            out["f16"], out["f16_s32"] = _chain(O, p, w, x, True, round_f16), _chain(O, p, w, x, False, round_f16)
        for a in out.values():
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def compare(fmt, a, b):
    """-> (differing fraction, fraction differing by more than the element's own ulp + 1e-5 of the magnitude of b, worst |a - b| as a
    fraction of the per-element bound ulp + WORST[fmt] of that magnitude)."""
    scale = float(np.abs(b).max())
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    ulp = ULP[fmt](a, b)
    return float((d > 0).mean()), float((d > ulp + 1e-5 * scale).mean()), float((d / (ulp + WORST[fmt] * scale)).max())
