"""Shared recipes of tests/test_tiny_i8_host.py and tests/test_tiny_i8_gpu.py (int8 plans of pooled nets: Net.set_pools_i8; include/y3.h,
"Stand-alone ops in int8"): reduced pooled programs, the refused graphs, a brute-force int8 walker that shares no code with
quant.forward_i8, and the int8 test data of the pool kernel.  NumPy only; nothing here needs the HIP library or a GPU."""
import numpy as np

from tests.helpers import _Graph
from yolo_v3_tf2_amd import quant

POOL = {"size_xy": [2, 2], "padding": "same"}
# the pool kernel in int8: (shape [B,H,W,C], strides)
POOL_SHAPES = (((3, 12, 8, 16), (1, 2)),          # one 16-byte vector per pixel
               ((2, 13, 13, 512), (1,)),          # more than one workgroup
               ((2, 14, 14, 512), (2,)),          # ... at stride 2 (even extents)
               ((2, 13, 7, 48), (1,)),            # odd extents, three vectors per pixel
               ((1, 1, 1, 16), (1,)),
               ((1, 2, 2, 16), (1, 2)),
               ((1, 4, 128, 256), (1, 2)))        # a row of 1024+ vectors: the one-row-per-workgroup branch
POOL_DATA = ("random", "negative", "positions", "signs")


class _PGraph(_Graph):
    def maxpool(self, x, stride):
        return self._keep(self.b.maxpool(x, dict(POOL, stride_xy=[stride, stride]), "body"))


def reduced_pooled_program():
    """YOLOv3-tiny's part behind the cut in small, on a [B,H,W,128] fp16 input (H, W multiples of 4), so that c* = 0 and the input is the
    tensor that crosses:
      a    3x3  128 -> 256            pa = pool / 2 (a)        b  3x3  256 -> 128 (pa)        pb = pool / 1 (b)
      c    1x1  128 -> 128 (pb)       up = up-sample (c)       cat = [up, a] (384)
      h0   3x3  384 -> 256 (cat)      fp32 output              h1  1x1  128 -> 255 (up), bias, linear    fp32 output
    The up-sample has two readers and the concat a 3x3 reader, so neither folds into a conv.
    -> (program, {"pa" | "pb" | "up" | "cat": tensor id})."""
    g = _PGraph(128)
    g._keep(g.input)
    a = g.conv(g.input, 256, 3)
    pa = g.maxpool(a, 2)
    b = g.conv(pa, 128, 3)
    pb = g.maxpool(b, 1)
    c = g.conv(pb, 128, 1)
    up = g.upsample(c)
    cat = g.route(up, a)
    h0 = g.conv(cat, 256, 3, sub="head")
    h1 = g.conv(up, 255, 1, bn=False, act="linear", sub="head")
    return g.program([h0, h1]), dict(pa=pa, pb=pb, up=up, cat=cat)


def mixed_concat_program():
    """[B,H,W,64] fp16 input: c0 3x3 64 -> 128 lies before the cut (Cin = 64), c1 3x3 128 -> 128 behind it, and a stand-alone concat
    [c1, c0] feeds a 3x3 head: one source on each side of the cut."""
    g = _PGraph(64)
    g._keep(g.input)
    c0 = g.conv(g.input, 128, 3)
    c1 = g.conv(c0, 128, 3)
    cat = g.route(c1, c0)
    h0 = g.conv(cat, 256, 3, sub="head")
    h1 = g.conv(c1, 128, 1, sub="head")
    return g.program([h0, h1])


def add_behind_cut_program():
    """[B,H,W,128] fp16 input, c* = 0: t2 = conv1x1(t1 = conv3x3(x)) feeds a stand-alone add (t2 + t1) and a head, so the add does not fold."""
    g = _PGraph(128)
    g._keep(g.input)
    t1 = g.conv(g.input, 128, 3)
    t2 = g.conv(t1, 128, 1)
    add = g.shortcut(t2, t1)
    h0 = g.conv(t2, 128, 1, sub="head")
    h1 = g.conv(add, 128, 3, sub="head")
    return g.program([h0, h1])


def aux_reads_output_program():
    """[B,H,W,128] fp16 input, c* = 0: head h0 (1x1, 128 -> 128, at 1/2) is a net output AND the source of a stand-alone up-sample, whose tensor a
    3x3 head and a 1x1 head read (two readers: it does not fold)."""
    g = _PGraph(128)
    g._keep(g.input)
    t1 = g.conv(g.input, 128, 3, stride=2)
    h0 = g.conv(t1, 128, 1, sub="head")
    up = g.upsample(h0)
    h1 = g.conv(up, 128, 3, sub="head")
    h2 = g.conv(up, 128, 1, sub="head")
    return g.program([h0, h1, h2]), h0


def aux_writes_output_program():
    """[B,H,W,128] fp16 input, c* = 0: a pool's own tensor is named as a net output."""
    g = _PGraph(128)
    g._keep(g.input)
    t1 = g.conv(g.input, 128, 3)
    pool = g.maxpool(t1, 2)
    h1 = g.conv(pool, 128, 1, sub="head")
    return g.program([pool, h1]), pool


def reduced_inputs(p, batch, canvas, seed=5):
    """(weights, fp16-exact input [batch, H, W, Cin]) of a reduced program."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    cin = p.tensors[p.input_tensor].channels
    x = np.random.default_rng(seed).standard_normal((batch, canvas[0], canvas[1], cin)).astype(np.float16).astype(np.float32)
    return synthetic_weights(p, seed=seed), x


def class_scales(p, seed=5):
    """Plausible scales for every tensor, one per class of quant.scale_classes."""
    s = list(np.random.default_rng(seed).uniform(0.02, 0.08, len(p.tensors)).astype(np.float32))
    for g in quant.scale_classes(p):
        for t in g:
            s[t] = s[g[0]]
    return [float(v) for v in s]


# ---- the brute-force walker ---------------------------------------------------------------------------------------------------------
def brute_walk(p, weights, scales, boundary, cut):
    """The int8 network behind the cut, node by node over Program.nodes with plain loops over the window taps: no torch, no
    quant.conv_i8 / aux_i8 / forward_i8, no maxpool2x2_ref.  Which node runs in int8 is decided here from 'every input is an int8
    value already' -- the boundary copies stand in for their fp16 tensors, as they do for the convs on the device.
    -> {tensor id: int8 NHWC, or fp32 for a head}."""
    f32 = np.float32
    conv_nodes = sorted((n for n in p.nodes if n.kind == "conv"), key=lambda n: n.conv_index)
    first = conv_nodes[cut]
    vals = dict(boundary)
    started = False
    assert not any(t in p.outputs for n in p.nodes for t in n.inputs if n.kind != "yolo"), "a head read again inside the net is not walked here"
    for n in p.nodes:
        started = started or n is first
        if not started or n.kind == "yolo":
            continue
        if n.kind == "conv":
            x = vals[n.inputs[0]].astype(np.int64)
            i, k, s = n.conv_index, n.size, n.stride
            w = np.asarray(weights[f"conv{i}.w"], f32)
            mx = np.abs(w).reshape(-1, w.shape[-1]).max(axis=0)
            sw = np.where(mx > 0, mx / f32(127), f32(1)).astype(f32)
            wq = np.clip(np.rint(w / sw), -127, 127).astype(np.int64)
            B, H, W, _ = x.shape
            pad = k // 2
            xp = np.zeros((B, H + 2 * pad, W + 2 * pad, x.shape[3]), np.int64)
            xp[:, pad:pad + H, pad:pad + W] = x
            Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
            acc = np.zeros((B, Ho, Wo, w.shape[-1]), np.int64)
            for u in range(k):
                for v in range(k):
                    acc += xp[:, u:u + s * Ho:s, v:v + s * Wo:s] @ wq[u, v]
            if n.bn:
                g, b, m, var = (np.asarray(weights[f"conv{i}.{q}"], f32) for q in ("gamma", "beta", "mean", "var"))
                bn = (f32(1) / np.sqrt(var + f32(1e-3), dtype=f32)) * g
                shift = (b - m * bn).astype(f32)
            else:
                bn, shift = np.ones(w.shape[-1], f32), np.asarray(weights[f"conv{i}.bias"], f32)
            sc = ((f32(scales[n.inputs[0]]) * sw).astype(f32) * bn).astype(f32)
            y = (acc.astype(f32) * sc).astype(f32) + shift
            if n.leaky:
                y = np.maximum(y, f32(0.1) * y)
            if n.output not in p.outputs:      # a head stores fp32
                y = np.clip(np.rint(y * (f32(1) / f32(scales[n.output]))), -127, 127).astype(np.int8)
            vals[n.output] = y
            continue
        if not all(t in vals and vals[t].dtype == np.int8 and t not in boundary for t in n.inputs):
            continue      # an aux op before the cut
        a = vals[n.inputs[0]]
        B, H, W, C = a.shape
        if n.kind == "maxpool":
            s = n.stride
            y = np.empty((B, H // s, W // s, C), np.int8)
            for yo in range(H // s):
                for xo in range(W // s):
                    best = None
                    for yy in (yo * s, min(yo * s + 1, H - 1)):
                        for xx in (xo * s, min(xo * s + 1, W - 1)):
                            best = a[:, yy, xx] if best is None else np.where(a[:, yy, xx] > best, a[:, yy, xx], best)
                    y[:, yo, xo] = best
        elif n.kind == "upsample":
            y = np.empty((B, 2 * H, 2 * W, C), np.int8)
            for yo in range(2 * H):
                for xo in range(2 * W):
                    y[:, yo, xo] = a[:, yo // 2, xo // 2]
        elif n.kind == "concat":
            c = vals[n.inputs[1]]
            y = np.empty((B, H, W, C + c.shape[3]), np.int8)
            y[..., :C] = a
            y[..., C:] = c
        else:
            raise ValueError(n.kind)
        vals[n.output] = y
    return vals


# ---- int8 data of the pool kernel ---------------------------------------------------------------------------------------------------
def pool_data_i8(shape, kind, seed=11):
    """random: all 256 byte values; negative: every value below zero, -128 included; positions: the largest value of every stride-2
    window sits at window position (y + x + byte lane) mod 4 in raster order, so that each of the four positions wins in each byte lane;
    signs: neighbours such as -1 against 1 and -128 against 127, which an unsigned or whole-word compare orders the wrong way."""
    rng = np.random.default_rng(seed)
    B, H, W, C = shape
    if kind == "random":
        x = rng.integers(-128, 128, shape)
    elif kind == "negative":
        x = rng.integers(-128, 0, shape)
    elif kind == "positions":
        x = rng.integers(-128, 100, shape)
        yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        pos = (yy % 2) * 2 + (xx % 2)
        win = ((yy // 2) + (xx // 2) + cc) % 4
        x = np.where((pos == win)[None], rng.integers(100, 128, shape), x)
    elif kind == "signs":
        pairs = np.array([[-1, 1], [1, -1], [-128, 127], [0, -1], [-2, -1], [127, -127], [-128, -127], [1, 0]])
        yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        x = np.broadcast_to(pairs[(cc + yy // 2) % len(pairs), (xx + yy) % 2][None], shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.int8)
