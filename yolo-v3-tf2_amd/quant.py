"""The int8 scheme of Y3_DTYPE_I8 plans restated in NumPy (include/y3.h, "int8 plans"; DESIGN.md section 7, "int8 plans").

The device accumulates exact i32 sums and its epilogue is a fixed sequence of fp32 operations, so this restatement reproduces every
stored byte and every head logit of the device: the GPU tests compare with np.array_equal, no tolerance.  Runs on the CPU; the exact
integer conv goes through torch.nn.functional.conv2d in float64 (|sum| <= 127 * 127 * K < 2^53: exact).

    format    symmetric int8 in [-127, 127]; one fp32 scale per activation tensor, one per output channel of a conv's weights
    weights   s_w[c] = absmax_c / 127 (1 for an all-zero channel), q = clamp(rint(w / s_w[c]))       raw weights, BN in the epilogue
    epilogue  v = (float)acc * sc[c] + sh[c];  v = max(v, 0.1f v) when leaky;  v = (float)r * s_res + v with a shortcut;
              q = clamp(rintf(v * (1.0f / s_out)));   sc[c] = (s_in * s_w[c]) * bn_scale[c];  an fp32 output stores v
    aux ops   (Net.set_pools_i8) a max-pool, an up-sample or a concat whose every source lies behind the cut selects or moves stored bytes:
              destination and sources carry one scale (scale_classes), the pool compares the bytes as signed values
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np

from .graph import AuxOp, ConvOp, Program
from .maxpool import maxpool2x2_ref
from .weights import BN_EPS

F32 = np.float32


def quantize_weights(w: np.ndarray):
    """HWIO fp32 weights -> (q int8 HWIO, s_w fp32 [Cout]): per output channel, absmax / 127, true division, round to nearest even."""
    w = np.asarray(w, F32)
    mx = np.abs(w).reshape(-1, w.shape[-1]).max(axis=0).astype(F32)
    s = np.where((mx > 0) & np.isfinite(mx), mx / F32(127.0), F32(1.0)).astype(F32)
    q = np.clip(np.rint(w / s), -127.0, 127.0).astype(np.int8)
    return q, s


def quantize(x: np.ndarray, s) -> np.ndarray:
    """fp32 values (an fp16 tensor widened) -> int8 at scale s: q = clamp(rintf(x * (1.0f / s))), one fp32 multiply."""
    inv = F32(1.0) / F32(s)
    return np.clip(np.rint(np.asarray(x, F32) * inv), -127.0, 127.0).astype(np.int8)


def dequantize(q: np.ndarray, s) -> np.ndarray:
    return q.astype(F32) * F32(s)


def first_i8_conv(p: Program) -> int:
    """c*: the first conv slot (op order) such that it and every conv after it has Cin % 128 == 0 (both parts of a concat) and
    Cout % 16 == 0 unless it writes an fp32 output itself; -1 when no conv qualifies."""
    convs = p.conv_ops()
    cut = len(convs)
    for i in range(len(convs) - 1, -1, -1):
        o = convs[i]
        ok = (o.cin != 3 and o.cin % 128 == 0 and (o.src1 < 0 or (o.c0 % 128 == 0 and (o.cin - o.c0) % 128 == 0))
              and (writes_f32(p, o) or o.cout % 16 == 0))
        if not ok:
            break
        cut = i
    return cut if cut < len(convs) else -1


def writes_f32(p: Program, o: ConvOp) -> bool:
    """Does the launch of o store the caller's fp32 grid itself?  A net output that no conv reads again and no shortcut conv writes."""
    if o.dst not in p.outputs or o.residual >= 0 or o.cin == 3:
        return False
    return not any(o.dst in (c.src0, c.src1, c.residual) for c in p.conv_ops())


def bn_fold(o: ConvOp, weights: Dict[str, np.ndarray], eps: float = BN_EPS):
    """(scale, shift) fp32 [Cout] of conv o as the library forms them: scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    i = o.conv_index
    if o.bn:
        g, b, m, v = (np.asarray(weights[f"conv{i}.{k}"], F32) for k in ("gamma", "beta", "mean", "var"))
        scale = (F32(1.0) / np.sqrt(v + F32(eps), dtype=F32)) * g
        return scale.astype(F32), (b - m * scale).astype(F32)
    return np.ones(o.cout, F32), np.asarray(weights[f"conv{i}.bias"], F32)


def int_conv(xq: np.ndarray, wq: np.ndarray, stride: int) -> np.ndarray:
    """Exact integer conv: xq int8 NHWC, wq int8 HWIO, 'same' padding of size // 2 -> int64 NHWC."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(xq.astype(np.float64))).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.ascontiguousarray(wq.astype(np.float64))).permute(3, 2, 0, 1)
    y = torch.nn.functional.conv2d(x, w, stride=stride, padding=wq.shape[0] // 2)
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).numpy()).astype(np.int64)


def conv_i8(o: ConvOp, weights: Dict[str, np.ndarray], tensor_q: Callable[[int], np.ndarray], scales, out_f32: bool,
            eps: float = BN_EPS) -> np.ndarray:
    """One int8 conv launch from its own int8 inputs (tensor_q(id) -> int8 NHWC): [upsample] [concat] conv, epilogue as above.
    scales[t]: the fp32 scale of tensor t.  -> int8 NHWC, or fp32 NHWC with out_f32."""
    x = tensor_q(o.src0)
    if o.src0_upsample:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    if o.src1 >= 0:
        assert F32(scales[o.src0]) == F32(scales[o.src1]), "the two sources of a concat conv carry one scale"
        x = np.concatenate([x, tensor_q(o.src1)], axis=3)
    wq, sw = quantize_weights(weights[f"conv{o.conv_index}.w"])
    acc = int_conv(x, wq, o.stride)
    bn_scale, shift = bn_fold(o, weights, eps)
    sc = ((F32(scales[o.src0]) * sw).astype(F32) * bn_scale).astype(F32)
    v = (acc.astype(F32) * sc).astype(F32) + shift
    if o.leaky:
        v = np.maximum(v, F32(0.1) * v)
    if o.residual >= 0:
        v = (tensor_q(o.residual).astype(F32) * F32(scales[o.residual])).astype(F32) + v
    if out_f32:
        return v.astype(F32)
    inv = F32(1.0) / F32(scales[o.dst])
    return np.clip(np.rint(v * inv), -127.0, 127.0).astype(np.int8)


def i8_aux_ops(p: Program, cut: int):
    """Which aux ops an int8 plan with Net.set_pools_i8 runs on int8 tensors (y3_net_plan's rule): a tensor is behind the cut when a conv
    from slot `cut` on or an int8 aux op writes it; walking the aux ops in op order, a max-pool, an up-sample or a concat runs in int8 when
    every source it has is behind the cut, and as in an fp16 plan when none is.  -> (the AuxOp objects that run in int8, in op order; the
    set of tensor ids behind the cut).  ValueError for what the plan refuses: a concat with one source on each side, an add behind the cut."""
    behind = {o.dst for o in p.conv_ops()[cut:]}
    chosen = []
    for o in p.ops:
        if not isinstance(o, AuxOp):
            continue
        n = sum(t in behind for t in o.inputs)
        if n == 0:
            continue
        if o.kind == "add":
            raise ValueError(f"a stand-alone add ({o.inputs} -> {o.dst}) behind the int8 cut has no int8 form")
        if n < len(o.inputs):
            raise ValueError(f"{o.kind} ({o.inputs} -> {o.dst}) has one source behind the int8 cut and one before it")
        chosen.append(o)
        behind.add(o.dst)
    return chosen, behind


def crossing_tensors(p: Program, cut: int):
    """The tensors not behind the cut that an int8 conv reads (sorted): each gets an int8 copy, quantize(x, scale)."""
    convs = p.conv_ops()
    _, behind = i8_aux_ops(p, cut)
    return sorted({t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind})


def aux_i8(o: AuxOp, tensor_q: Callable[[int], np.ndarray], scales) -> np.ndarray:
    """One int8 aux launch from its own int8 inputs: the max-pool on signed bytes, the up-sample and the concat as moves of bytes."""
    for t in o.inputs:
        assert F32(scales[t]) == F32(scales[o.dst]), "an int8 aux op's destination and sources carry one scale"
    x = tensor_q(o.inputs[0])
    assert x.dtype == np.int8
    if o.kind in ("maxpool_s2", "maxpool_s1"):
        return maxpool2x2_ref(x, 2 if o.kind == "maxpool_s2" else 1)
    if o.kind == "upsample":
        return x.repeat(2, axis=1).repeat(2, axis=2)
    if o.kind == "concat":
        return np.concatenate([x, tensor_q(o.inputs[1])], axis=3)
    raise ValueError(o.kind)


def forward_i8(p: Program, weights: Dict[str, np.ndarray], scales, boundary: Dict[int, np.ndarray], first_conv: Optional[int] = None,
               eps: float = BN_EPS):
    """The network behind the cut, free-running from the int8 boundary tensors {tensor id: int8 NHWC} (the copies of what crosses the
    cut): p.ops walked from the cut conv on, the convs and the int8 aux ops (i8_aux_ops).  -> {tensor id: int8 NHWC, or fp32 NHWC for a
    tensor a launch writes as an fp32 output} of every conv from c* on and every int8 aux op."""
    cut = first_i8_conv(p) if first_conv is None else first_conv
    assert cut >= 0, "no conv of this program qualifies for int8"
    t: Dict[int, np.ndarray] = dict(boundary)
    in_i8 = {id(o) for o in i8_aux_ops(p, cut)[0]}
    start = p.ops.index(p.conv_ops()[cut])
    for o in p.ops[start:]:
        if isinstance(o, ConvOp):
            t[o.dst] = conv_i8(o, weights, t.__getitem__, scales, writes_f32(p, o), eps)
        elif id(o) in in_i8:
            t[o.dst] = aux_i8(o, t.__getitem__, scales)
    return t


# ---- calibration -------------------------------------------------------------------------------------------------------------------
def scale_from_absmax(a: float) -> float:
    """The scale that maps |x| = a to 127 (1 for an all-zero tensor), as fp32."""
    a = F32(a)
    return float(a / F32(127.0)) if a > 0 and np.isfinite(a) else 1.0


def scale_classes(p: Program, cut: Optional[int] = None):
    """The sets of tensors that must carry one scale in an int8 plan with Net.set_pools_i8: the destination and every source of an int8
    aux op (i8_aux_ops), and the two sources of every concat conv, merged where they share a tensor.  -> a list of sorted lists, classes
    of one tensor left out, ordered by their first member."""
    cut = first_i8_conv(p) if cut is None else cut
    parent = list(range(len(p.tensors)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def tie(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for o in p.conv_ops():
        if o.src1 >= 0:
            tie(o.src0, o.src1)
    if cut >= 0:
        for o in i8_aux_ops(p, cut)[0]:
            for t in o.inputs:
                tie(t, o.dst)
    groups: Dict[int, list] = {}
    for t in range(len(p.tensors)):
        groups.setdefault(find(t), []).append(t)
    return [g for _, g in sorted(groups.items()) if len(g) > 1]


def equalize_concat(p: Program, scales, classes: Optional[bool] = None):
    """The two sources of every concat conv take the larger of their scales (repeated until nothing changes: a tensor may feed two).
    classes (None: whenever the program has int8 aux ops behind its cut, a pooled net; Net.calibrate_i8 passes its set_pools_i8 switch):
    every class of scale_classes takes the largest scale of its members instead, unset members (<= 0 or None) included once any member
    has one."""
    s = list(scales)
    cut = first_i8_conv(p)
    if classes is None:
        classes = cut >= 0 and bool(i8_aux_ops(p, cut)[0])
    if classes and cut >= 0:
        for g in scale_classes(p, cut):
            m = max((s[t] or 0.0) for t in g)
            if m > 0:
                for t in g:
                    s[t] = m
        return s
    changed = True
    while changed:
        changed = False
        for o in p.conv_ops():
            if o.src1 >= 0 and s[o.src0] != s[o.src1]:
                s[o.src0] = s[o.src1] = max(s[o.src0], s[o.src1])
                changed = True
    return s


def conv_signature(p: Program) -> str:
    """What a calibration table is tied to: the program's convs, in order."""
    import hashlib
    rows = [f"{o.size},{o.stride},{o.cin},{o.cout},{int(o.bn)},{int(o.leaky)},{o.src0},{int(o.src0_upsample)},{o.c0},{o.src1},{o.residual},{o.dst}"
            for o in p.conv_ops()]
    return hashlib.sha256(";".join(rows).encode()).hexdigest()


def save_calibration(path: str, p: Program, scales) -> None:
    """JSON: tensor id -> scale (unset entries left out), with the program's conv signature."""
    import json
    doc = {"format": "y3-i8-calibration-1", "conv_signature": conv_signature(p), "n_tensors": len(p.tensors),
           "scales": {str(t): float(F32(s)) for t, s in enumerate(scales) if s is not None and s > 0}}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def load_calibration(path: str, p: Program):
    """-> list of len(p.tensors) scales (0.0: unset).  A table made for another graph is refused (ValueError)."""
    import json
    with open(path) as f:
        doc = json.load(f)
    if doc.get("format") != "y3-i8-calibration-1":
        raise ValueError(f"{path}: not an int8 calibration file")
    if doc.get("conv_signature") != conv_signature(p) or int(doc.get("n_tensors", -1)) != len(p.tensors):
        raise ValueError(f"{path}: calibrated for another graph (conv signature differs)")
    s = [0.0] * len(p.tensors)
    for k, v in doc["scales"].items():
        s[int(k)] = float(F32(v))
    return s
