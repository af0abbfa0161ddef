"""Data for the split-K int8 convs (low-latency int8 plans), shared by tests/test_splitk_i8_host.py (what the case is for, asserted in
NumPy alone) and tests/test_splitk_i8_gpu.py (the device against yolo_v3_tf2_amd/quant.py and against the unsplit plan, bit for bit).

wide512_case: the wide-accumulator case of tests/i8_edge_cases.py with 512 input channels, so that a 3x3 conv walks 36 K tiles of 128
and the sums of ONE slice of a split in two or three already lie beyond 2^24.  A slab that held such a sum as a float would round it, and
the rounded slices no longer add up to the conv's accumulator: slice_sums() below cuts the K walk as the kernel does, and the host test
asserts on these integers that float32 slabs would change fp32-output elements at S = 2 and at S = 3."""
import numpy as np

from tests.helpers import _Graph
from tests.i8_edge_cases import Case, F32, _head, _scales, _set, reference, round_f16
from yolo_v3_tf2_amd import quant
from yolo_v3_tf2_amd.weights import synthetic_weights

BK = 128              # channels per K tile of the int8 kernel
WIDE_SPLITS = (2, 3)
WIDE_TILE = 11


def wide512_case():
    """3x3 over 512 channels (K = 4608, 36 K tiles), 3 x 8 x 10, input bytes 118..127 at s_in = 2^-3, weights q in 100..127 of one sign
    per output channel, the sign alternating: |acc| reaches 6.4e7 < 2^31 in the interior.
      a  stored: BN, leaky, Cout 128       h  fp32 output, bias, Cout 255"""
    g = _Graph(512)
    g._keep(g.input)
    a = g.conv(g.input, 128, 3)
    h = _head(g, g.input, 3)
    p = g.program([h, _head(g, a), g.conv(a, 128, 1, act="linear", sub="head")])
    rng = np.random.default_rng(203)
    w = synthetic_weights(p, seed=203)
    s_in = F32(2.0 ** -3)
    x = (rng.integers(118, 128, (3, 8, 10, 512)) * s_in).astype(F32)
    assert np.array_equal(x, round_f16(x))
    case = Case("wide512", p, w, x, _scales(p), dict(a=a), dict(h=h))
    _set(case.scales, p.input_tensor, s_in)
    for t in (a, h):
        o = case.op(t)
        q = rng.integers(100, 128, (3, 3, 512, o.cout))
        q[1, 1, 0, :] = 127
        w[f"conv{o.conv_index}.w"] = (q * (1 - 2 * (np.arange(o.cout) % 2)) * F32(2.0 ** -12)).astype(F32)
    # a: v = acc * s_in * 2^-12 * gamma / sqrt(var + eps) + shift ~ 6.4e7 * 3e-5 = 2e3 at the most; s_out = 16 puts that at +-125
    _set(case.scales, a, 16.0)
    return case


def slice_sums(o, weights, xq, S):
    """The S partial sums of conv o (single source) as the split kernel forms them: the K walk is tap-major, k = tap * Cin + c, in tiles of
    BK channels, and slice y covers tiles [y * KT / S, (y + 1) * KT / S).  -> int64 [S, B, Ho, Wo, Cout]."""
    wq, _ = quant.quantize_weights(weights[f"conv{o.conv_index}.w"])
    kt = o.size * o.size * o.cin // BK
    flat_k = np.arange(o.size * o.size * o.cin).reshape(o.size, o.size, o.cin)      # HWI order is the walk's order
    out = []
    for y in range(S):
        lo, hi = y * kt // S * BK, (y + 1) * kt // S * BK
        mask = ((flat_k >= lo) & (flat_k < hi))[..., None]
        out.append(quant.int_conv(xq, wq * mask, o.stride))
    return np.stack(out)


_cache = {}


def get():
    """(case, xq, reference tensors): built once, shared by the tests, left unchanged."""
    if "wide512" not in _cache:
        case = wide512_case()
        _cache["wide512"] = (case,) + reference(case)
    return _cache["wide512"]
