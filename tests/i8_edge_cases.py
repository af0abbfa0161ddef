"""int8 data the random-input suites never produce, shared by tests/test_i8_edges_host.py (what each case is for, asserted from
yolo_v3_tf2_amd/quant.py alone) and tests/test_i8_edges_gpu.py (the device against quant.py, bit for bit): rounding ties, saturation,
accumulators beyond 2^24, the weight quantiser's and the BN fold's edge channels.

Every program has an fp16 input of 128 or 256 channels, so the cut is conv 0 and the input itself goes through quantize16_to_i8; every
scale is set by hand.  A case is a Case below; `stored` names the int8 tensors the case is about, `heads` the fp32 outputs."""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from tests.helpers import _Graph
from yolo_v3_tf2_amd import quant
from yolo_v3_tf2_amd.weights import synthetic_weights

F32 = np.float32
TILES = (11, 29)      # one 32x32x32 tile (64x64) and one 16x16x64 tile (64x128): both MFMA forms have epilogue loops of their own


@dataclass
class Case:
    name: str
    program: object
    weights: Dict[str, np.ndarray]
    x: np.ndarray                      # fp32 NHWC, every value exact in fp16
    scales: List[float]                # one per tensor, 0.0 where none is needed
    stored: Dict[str, int]             # role -> tensor id of a stored int8 tensor
    heads: Dict[str, int] = field(default_factory=dict)

    @property
    def B(self):
        return self.x.shape[0]

    @property
    def canvas(self) -> Tuple[int, int]:
        return self.x.shape[1], self.x.shape[2]

    def op(self, tensor):
        return conv_of(self.program, tensor)


def conv_of(p, tensor):
    """The conv launch that writes `tensor` (a shortcut's sum is written by the conv it is folded into)."""
    return next(o for o in p.conv_ops() if o.dst == tensor)


def round_f16(x):
    return np.asarray(x, F32).astype(np.float16).astype(F32)


def _scales(p):
    return [0.0] * len(p.tensors)


def _set(scales, t, v):
    scales[t] = float(F32(v))


# ---------------------------------------------------------------------------------------------- the restatement, taken apart
def epilogue_parts(o, weights, tensor_q, scales, out_f32):
    """quant.conv_i8 with its intermediate values kept: -> (acc int64, v fp32 after the shortcut, t = v * (1 / s_out) or None).
    tests/test_i8_edges_host.py holds clamp(rint(t)) (or v) to quant.conv_i8 itself, so what the host test says of acc, v and t is
    said of the restatement the device is compared with."""
    x = tensor_q(o.src0)
    if o.src0_upsample:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    if o.src1 >= 0:
        x = np.concatenate([x, tensor_q(o.src1)], axis=3)
    wq, sw = quant.quantize_weights(weights[f"conv{o.conv_index}.w"])
    acc = quant.int_conv(x, wq, o.stride)
    bn_scale, shift = quant.bn_fold(o, weights)
    sc = ((F32(scales[o.src0]) * sw).astype(F32) * bn_scale).astype(F32)
    v = (acc.astype(F32) * sc).astype(F32) + shift
    if o.leaky:
        v = np.maximum(v, F32(0.1) * v)
    if o.residual >= 0:
        v = (tensor_q(o.residual).astype(F32) * F32(scales[o.residual])).astype(F32) + v
    v = v.astype(F32)
    return acc, v, None if out_f32 else (v * (F32(1.0) / F32(scales[o.dst]))).astype(F32)


def reference(case):
    """The case through quant.py, free-running from the input's int8 copy: -> (xq, {tensor: int8 or fp32 NHWC})."""
    p = case.program
    xq = quant.quantize(case.x, case.scales[p.input_tensor])
    return xq, quant.forward_i8(p, case.weights, case.scales, {p.input_tensor: xq}, 0)


def parts(case, ref, tensor):
    """epilogue_parts of the conv that writes `tensor`, on the reference's own tensors."""
    o = case.op(tensor)
    return epilogue_parts(o, case.weights, ref.__getitem__, case.scales, quant.writes_f32(case.program, o))


def is_half(t):
    """Exactly halfway between two integers."""
    return (t - np.floor(t)) == F32(0.5)


def round_half_away(t):
    return np.clip(np.where(t >= 0, np.floor(t + F32(0.5)), np.ceil(t - F32(0.5))), -127.0, 127.0).astype(np.int8)


def _head(g, x, k=1):
    return g.conv(x, 255, k, bn=False, act="linear", sub="head")


# ---------------------------------------------------------------------------------------------- 1. ties
def ties_case():
    """Four bias convs that read the input directly, power-of-two scales throughout, so that t = (acc + n) / 2 [+ r] exactly:
      a  1x1 linear             s_w = 2^-7, s_out = 2^-10      b  3x3 linear + input     s_w = 1/2, s_out = s_in
      c  1x1 leaky              s_w = 1/2,  s_out = s_in       d  3x3 leaky + input      s_w = 1/2, s_out = s_in
    The input is k/2 * s_in, k in -6..6 (channel 0, where every conv has its +-127 weight: k in -2..2), s_in = 2^-4."""
    g = _Graph(128)
    g._keep(g.input)
    a = g.conv(g.input, 128, 1, bn=False, act="linear")
    b = g.shortcut(g.conv(g.input, 128, 3, bn=False, act="linear"), g.input)
    c = g.conv(g.input, 128, 1, bn=False)
    d = g.shortcut(g.conv(g.input, 128, 3, bn=False), g.input)
    p = g.program([_head(g, a), _head(g, b), _head(g, g.route(c, d))])
    rng = np.random.default_rng(101)
    w = synthetic_weights(p, seed=101)
    s_in = F32(2.0 ** -4)
    k = rng.integers(-6, 7, (3, 10, 12, 128))
    k[..., 0] = rng.integers(-2, 3, (3, 10, 12))
    x = (k * (s_in / 2)).astype(F32)
    assert np.array_equal(x, round_f16(x))
    case = Case("ties", p, w, x, _scales(p), dict(a=a, b=b, c=c, d=d))
    _set(case.scales, p.input_tensor, s_in)
    for role, t in case.stored.items():
        o = case.op(t)
        unit = F32(2.0 ** -7) if role == "a" else F32(0.5)                   # s_w
        kq = rng.integers(-3, 4, (o.size, o.size, o.cin, o.cout))
        if o.size == 3:
            kq *= rng.random(kq.shape) < 1.0 / 3                              # K = 1152: thinned, so that few outputs saturate
        kq[o.size // 2, o.size // 2, 0, :] = 127 * (1 - 2 * (np.arange(o.cout) % 2))
        w[f"conv{o.conv_index}.w"] = (kq * unit).astype(F32)
        sc = s_in * unit                                                      # exact: bias convs have no BN scale
        lo, hi = (0, 41) if o.leaky else (-8, 9)                              # leaky: ties only where v >= 0 (0.1f v is inexact)
        w[f"conv{o.conv_index}.bias"] = (rng.integers(lo, hi, o.cout) * sc).astype(F32)
        _set(case.scales, t, F32(2.0 ** -10) if role == "a" else s_in)
    return case


# ---------------------------------------------------------------------------------------------- 2. saturation
# scales of the stored tensors: about 1/8 of what absmax calibration gives on this input (absmax / 127 is 0.035 for the input)
SATURATION_SCALES = dict(input=0.008, a=0.0055, b=0.0085, c=0.006, d=0.006)


def saturation_case():
    """BN convs on Gaussian data under scales far too small for it:
      a  1x1 linear      b  3x3 linear + input      c  3x3 leaky + input (reads a)      d  1x1 leaky alone (reads b)"""
    g = _Graph(128)
    g._keep(g.input)
    a = g.conv(g.input, 128, 1, act="linear")
    b = g.shortcut(g.conv(g.input, 128, 3, act="linear"), g.input)
    c = g.shortcut(g.conv(a, 128, 3), g.input)
    d = g.conv(b, 256, 1)
    p = g.program([_head(g, c), _head(g, d), _head(g, a)])
    w = synthetic_weights(p, seed=102)
    for t in (b, c):      # the shortcut branches: synthetic_weights keeps them small (gamma 0.25); here they weigh as much as the shortcut
        w[f"conv{conv_of(p, t).conv_index}.gamma"] *= F32(4.0)
    x = round_f16(np.random.default_rng(102).standard_normal((2, 12, 16, 128)))
    case = Case("saturation", p, w, x, _scales(p), dict(a=a, b=b, c=c, d=d))
    _set(case.scales, p.input_tensor, SATURATION_SCALES["input"])
    for role, t in case.stored.items():
        _set(case.scales, t, SATURATION_SCALES[role])
    return case


# ---------------------------------------------------------------------------------------------- 3. wide accumulators
def wide_case():
    """3x3 over 256 channels (K = 2304), input bytes 118..127 at s_in = 2^-3, weights q in 100..127 of one sign per output channel, the
    sign alternating: |acc| reaches 3e7 in the interior, 2/3 of it on an edge, 4/9 in a corner.
      a  stored: BN, leaky, Cout 128       h  fp32 head, bias, Cout 255"""
    g = _Graph(256)
    g._keep(g.input)
    a = g.conv(g.input, 128, 3)
    h = _head(g, g.input, 3)
    p = g.program([h, _head(g, a), g.conv(a, 128, 1, act="linear", sub="head")])
    rng = np.random.default_rng(103)
    w = synthetic_weights(p, seed=103)
    s_in = F32(2.0 ** -3)
    x = (rng.integers(118, 128, (3, 8, 10, 256)) * s_in).astype(F32)
    assert np.array_equal(x, round_f16(x))
    case = Case("wide", p, w, x, _scales(p), dict(a=a), dict(h=h))
    _set(case.scales, p.input_tensor, s_in)
    for t in (a, h):
        o = case.op(t)
        q = rng.integers(100, 128, (3, 3, 256, o.cout))
        q[1, 1, 0, :] = 127
        w[f"conv{o.conv_index}.w"] = (q * (1 - 2 * (np.arange(o.cout) % 2)) * F32(2.0 ** -12)).astype(F32)
    # a: v = acc * s_in * 2^-12 * gamma / sqrt(var + eps) + shift ~ 3e7 * 3e-5 = 1e3 at the most; s_out = 8 puts that at +-125
    _set(case.scales, a, 8.0)
    return case


# ---------------------------------------------------------------------------------------------- 4. weights and BN
WEIGHT_CHANNELS = ("zero", "last_k_only", "negative_absmax", "ties", "absmax_1e-30", "absmax_1e4", "all_plus_mx", "gamma_zero", "gamma_negative")
MX = F32(127 * 2.0 ** -6)
WEIGHTS_SCALES = dict(input=0.03, a=0.02, b=0.015)


def edit_channels(w, i, bn, last):
    """Edit output channels 0..8 of conv i (WEIGHT_CHANNELS, in order) in place; `last`: one more all-zero channel, the last one."""
    W = w[f"conv{i}.w"]
    K = W[..., 0].size
    W[..., 0] = 0
    if last is not None:
        W[..., last] = 0
    W[..., 1] = 0
    W[-1, -1, -1, 1] = 0.37                                   # k = K - 1 in the packed row
    flat = W[..., 2].reshape(-1)
    flat[K // 3] = -2.0 * np.abs(flat).max()                  # the absmax is a negative element
    W[..., 2] = flat.reshape(W[..., 2].shape)
    ties = (((np.arange(K) * 37) % 254 - 127) + 0.5) * (MX / F32(127.0))       # (j + 0.5) s_w, j in -127..126
    ties[K // 2] = MX
    W[..., 3] = ties.reshape(W[..., 3].shape).astype(F32)
    W[..., 4] *= F32(1e-30) / np.abs(W[..., 4]).max()
    W[..., 5] *= F32(1e4) / np.abs(W[..., 5]).max()
    W[..., 6] = MX
    if bn:      # the two extreme channels brought back into the range of the others, so that their bytes say something
        w[f"conv{i}.gamma"][4] *= F32(1e30)
        w[f"conv{i}.mean"][4] = 0.0
        w[f"conv{i}.gamma"][5] *= F32(1e-4)
        w[f"conv{i}.gamma"][6] *= F32(0.02)
        w[f"conv{i}.gamma"][7] = 0.0
        w[f"conv{i}.gamma"][8] = -1.3


def weights_case(seed=104):
    """a  3x3 BN leaky 128 -> 128      b  1x1 BN linear 128 -> 128 (reads a)      h  1x1 bias head 128 -> 255 (reads b)
    with the channels of WEIGHT_CHANNELS edited into all three (the head: the seven weight edits, and channel 254 all zero)."""
    g = _Graph(128)
    g._keep(g.input)
    a = g.conv(g.input, 128, 3)
    b = g.conv(a, 128, 1, act="linear")
    h = _head(g, b)
    p = g.program([h, _head(g, a), g.conv(b, 128, 1, sub="head")])
    w = synthetic_weights(p, seed=seed)
    x = round_f16(np.random.default_rng(seed).standard_normal((2, 10, 12, 128)))
    case = Case("weights", p, w, x, _scales(p), dict(a=a, b=b), dict(h=h))
    for t, bn, last in ((a, True, None), (b, True, None), (h, False, 254)):
        edit_channels(w, case.op(t).conv_index, bn, last)
    _set(case.scales, p.input_tensor, WEIGHTS_SCALES["input"])
    _set(case.scales, a, WEIGHTS_SCALES["a"])
    _set(case.scales, b, WEIGHTS_SCALES["b"])
    return case


# ---------------------------------------------------------------------------------------------- 5. call order
def call_order_case():
    """The program of weights_case with two scale sets and two weight sets: (case under scales A, scales B, second weights)."""
    case = weights_case()
    scales_b = [s * 1.75 for s in case.scales]
    _set(scales_b, case.program.input_tensor, case.scales[case.program.input_tensor] * 0.6)
    second = weights_case(seed=105).weights
    return case, [float(F32(s)) for s in scales_b], second


BUILDERS = dict(ties=ties_case, saturation=saturation_case, wide=wide_case, weights=weights_case)
_cache = {}


def get(name):
    """(case, xq, reference tensors): built once, shared by the tests, left unchanged."""
    if name not in _cache:
        case = BUILDERS[name]()
        _cache[name] = (case,) + reference(case)
    return _cache[name]
