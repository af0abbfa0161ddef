"""Shared recipes of tests/test_odd_widths_host.py and tests/test_odd_widths_gpu.py: conv widths outside YOLOv3's own powers of two
(96, 160, 192, 384: the widths of width-scaled and pruned variants), which y3_net_create accepts and graph.py lowers like any other.
NumPy only; nothing here needs the library or a GPU.

odd_width_program(): one program that every plan mode must run.  A 96-channel input; every conv BN unless stated; the ops are created in
the order of the table, so that the int8 cut (quant.first_i8_conv) falls at g:

      a   3x3/1  96 -> 192, leaky                           K step 32 only (Cin % 64 = 32); three 64-wide N tiles
      b   1x1    192 -> 96, leaky                            three 32-wide N tiles
      c   3x3/1  96 -> 192, linear, + a                      shortcut
      d   3x3/2  192 -> 160, leaky       (reads c)           five 32-wide N tiles
      e   1x1    192 -> 96, leaky        (reads c)
      h0  1x1    [e, b] -> 255, bias, linear       head      concat boundary c0 = 96: K step 32 on a Cin that is a multiple of 64
      f   1x1    [up(d), e] -> 384, leaky                    c0 = 160
      g   3x3/1  384 -> 384, leaky                           three K chunks of 128 channels; three 128-wide N tiles
      h1  3x3/2  384 -> 96, leaky        (reads g) head      K = 3456
      h2  1x1    384 -> 160, linear      (reads g) head

unrunnable_programs(): three small nets no 16-bit tile divides (the K step 32 tiles of the 16-bit table are 64 wide)."""
import numpy as np

from tests.helpers import _Graph

SEED = 5
BATCH = 3
CANVASES = ((12, 12), (12, 8))          # M = 432 / 108 and 288 / 72: ragged against every BM, tiles span images; Ho != Wo
NAMES = ("a", "b", "c", "d", "e", "h0", "f", "g", "h1", "h2")
STORED = ("a", "b", "c", "d", "e", "f", "g")     # written in the plan's own format
BF16_DIFFER_CAP = 2e-3                  # tests/test_tile_matrix_gpu.py
F16_DIFFER_CAP = 1e-2                   # tests/test_f16_tile_matrix_gpu.py


def odd_width_program():
    """-> (program, {name: ConvOp}), names as in the module docstring."""
    g = _Graph(96)
    a = g.conv(g.input, 192, 3)
    b = g.conv(a, 96, 1)
    c = g.shortcut(g.conv(b, 192, 3, act="linear"), a)
    d = g.conv(c, 160, 3, stride=2)
    e = g.conv(c, 96, 1)
    h0 = g.conv(g.route(e, b), 255, 1, bn=False, act="linear", sub="head")
    f = g.conv(g.route(g.upsample(d), e), 384, 1)
    gg = g.conv(f, 384, 3)
    h1 = g.conv(gg, 96, 3, stride=2, sub="head")
    h2 = g.conv(gg, 160, 1, act="linear", sub="head")
    p = g.program([h0, h1, h2])
    by_dst = {o.dst: o for o in p.conv_ops()}
    return p, {k: by_dst[t] for k, t in dict(a=a, b=b, c=c, d=d, e=e, h0=h0, f=f, g=gg, h1=h1, h2=h2).items()}


def inputs(program, canvas, batch=BATCH, seed=SEED):
    """(weights, fp32 input [batch, H, W, Cin of the program]); the first images of a larger batch are those of a smaller one."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    h, w = canvas
    cin = program.tensors[program.input_tensor].channels
    rng = np.random.default_rng(seed)
    x = np.stack([rng.standard_normal((h, w, cin)).astype(np.float32) for _ in range(batch)])
    return synthetic_weights(program, seed=seed), x


def detect_program(nclasses=80):
    """An image network whose three 1x1 detection heads of 3 * (5 + nclasses) channels read 96-, 160- and 96-channel sources
    (Cin % 64 != 0: no head decodes its own tiles, so y3_net_detect takes the composed route), of widths every mode runs:
    3 -> 32 (3x3/1), 32 -> 64 (3x3/2), 64 -> 96 (3x3/2) [head at 1/4], 96 -> 192 (3x3/2), 192 -> 160 (1x1) [head at 1/8],
    160 -> 64 (3x3/2), 64 -> 96 (1x1) [head at 1/16].  Outputs coarsest grid first."""
    from yolo_v3_tf2_amd.graph import Program, _lower
    g = _Graph(3)
    t4 = g.conv(g.conv(g.conv(g.input, 32, 3), 64, 3, stride=2), 96, 3, stride=2)
    t8 = g.conv(g.conv(t4, 192, 3, stride=2), 160, 1)
    t16 = g.conv(g.conv(t8, 64, 3, stride=2), 96, 1)
    nh = 3 * (5 + nclasses)
    heads = [g.conv(t, nh, 1, bn=False, act="linear", sub="head") for t in (t16, t8, t4)]
    p = Program(g.b.tensors, g.b.nodes, [], g.input, heads, nclasses)
    p.conv_nodes = [n for n in g.b.nodes if n.kind == "conv"]
    _lower(p)
    return p


def unrunnable_programs():
    """{name: (program, slot of the conv no 16-bit tile divides, (cin, c0 or -1, cout) of it)}.  Behind that conv each net has a
    1x1 conv to 128 channels and three 1x1 heads 128 -> 64 that every mode runs, the heads in int8 (the cut falls at the first head): the
    refusal is about the named conv alone, and in an int8 plan it concerns a conv before the cut."""
    def tail(g, t):
        t = g.conv(t, 128, 1)
        return g.program([g.conv(t, 64, 1, sub="head") for _ in range(3)])

    out = {}
    g = _Graph(96)                                       # 96 -> 96, 3x3
    out["96to96_3x3"] = (tail(g, g.conv(g.input, 96, 3)), 0, (96, -1, 96))
    g = _Graph(3)                                        # 32 -> 32, 1x1, behind a 3 -> 32 first layer
    out["32to32_1x1"] = (tail(g, g.conv(g.conv(g.input, 32, 3), 32, 1)), 1, (32, -1, 32))
    g = _Graph(96)                                       # [96, 96] -> 96, 1x1
    u = g.conv(g.input, 192, 1)
    v = g.conv(u, 96, 1)
    w = g.conv(u, 96, 1)
    out["96+96to96_1x1"] = (tail(g, g.conv(g.route(v, w), 96, 1)), 3, (192, 96, 96))
    return out
