"""The fp16-emulating oracle of the fp16 tests (tests/test_f16_host.py, tests/test_f16_gpu.py, tests/test_f16_tile_matrix_gpu.py).

It is oracle.forward(..., bf16=True) -- the walker that rounds where a 16-bit pipeline stores (model_reader.bf16_stored) and holds the MFMA
convs' weights in the 16-bit format -- with the module-level oracle.oracle.round_bf16 replaced by an IEEE fp16 round trip for the duration
of a call only: the roundings stay in the same places, the format changes.  Nothing under oracle/ is edited."""
import contextlib

import numpy as np

from oracle import oracle as O


def round_f16(a):
    """fp32 -> IEEE fp16 (round to nearest even, subnormals kept, beyond 65504 -> inf) -> fp32, NumPy."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, np.float32).astype(np.float16).astype(np.float32)


@contextlib.contextmanager
def f16_emulation():
    """Inside the block every rounding of the oracle's bf16 mode is an fp16 rounding; the original is back afterwards, whatever happens."""
    original = O.round_bf16
    O.round_bf16 = round_f16
    try:
        yield O
    finally:
        O.round_bf16 = original


def forward_f16(program, weights, images, **kw):
    """oracle.forward in fp16 emulation (acc64 / keep as there)."""
    with f16_emulation():
        return O.forward(program, weights, images, bf16=True, **kw)


def f16_ulp_elem(a, b):
    """Per element: the spacing of fp16 numbers (11 significand bits) in the binade of the larger of |a|, |b|, floored at 2^-24 (the
    spacing of the fp16 subnormals)."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.maximum(np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 10), 2.0 ** -24)


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def free_running_floor(program, weights, x, keep=None):
    """The four oracle walks of the free-running comparison on input x: the fp16-emulating oracle with fp32 and with double accumulation
    (their distance is the floor: two fp16 pipelines that differ only in the order of their partial sums), the bf16-emulating oracle and
    the fp32 oracle.  -> dict(f16, f16_acc64, bf16, f32: the head grids; kept: the tensors `keep` names, of the fp16 walk;
    floor_rel / floor_max: per head)."""
    f16 = forward_f16(program, weights, x, keep=keep)
    f16, kept = f16 if keep else (f16, {})
    f16b = forward_f16(program, weights, x, acc64=True)
    out = dict(f16=f16, f16_acc64=f16b, kept=kept, bf16=O.forward(program, weights, x, bf16=True), f32=O.forward(program, weights, x))
    out["floor_rel"] = [rel_l2(a, b) for a, b in zip(f16b, f16)]
    out["floor_max"] = [float(np.abs(a - b).max()) for a, b in zip(f16b, f16)]
    return out


def launch_flip_fraction(op, weights, tensor, first_layer_fp32=True):
    """One fused launch from fp16 input tensors (tensor(id) -> fp32 NHWC holding fp16-exact values; the Cin = 3 first layer takes the fp32
    image and fp32 weights): the fraction of elements at which round_f16 of the fp32-accumulating launch differs from round_f16 of the
    double-accumulating one, and the fp32-accumulating result."""
    from tests.helpers import oracle_launch
    w16 = not (first_layer_fp32 and op.cin == 3)
    with f16_emulation():
        y32 = round_f16(oracle_launch(O, op, weights, tensor, acc64=False, bf16_weights=w16))
        y64 = round_f16(oracle_launch(O, op, weights, tensor, acc64=True, bf16_weights=w16))
    return float((y32 != y64).mean()), y32
