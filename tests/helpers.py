"""Shared builders for the parity tests."""
import numpy as np

from yolo_v3_tf2_amd.graph import Program, _Builder, _lower


def mini_program(in_channels, convs_chain, heads):
    """input [B,S,S,in_channels] -> chain of convs -> three 'head' convs, all raw outputs (nclasses=0).
    convs_chain / heads: lists of dict(filters,size,stride,bn,act[,shortcut]) in the model-YAML vocabulary."""
    b = _Builder(0, None)
    x = b.new_tensor(in_channels, 1, "input")
    inp = x
    layers = [x]
    for c in convs_chain:
        conf = {"filters": c["filters"], "size": c["size"], "stride": c.get("stride", 1),
                "activation": c.get("act", "leaky")}
        if c.get("bn", True):
            conf["batch_normalize"] = 1
        x = b.conv(x, conf, "body")
        layers.append(x)
        if c.get("shortcut"):
            x = b.shortcut(x, {"from": c["shortcut"], "activation": "linear"}, layers, "body")
            layers.append(x)
    outs = []
    for h in heads:
        conf = {"filters": h["filters"], "size": h["size"], "stride": h.get("stride", 1),
                "activation": h.get("act", "leaky")}
        if h.get("bn", True):
            conf["batch_normalize"] = 1
        outs.append(b.conv(x, conf, "head"))
    p = Program(b.tensors, b.nodes, [], inp, outs, 0)
    p.conv_nodes = [n for n in b.nodes if n.kind == "conv"]
    _lower(p)
    return p


class _Graph:
    """A _Builder plus the running `layers` list its shortcut / route take their sources from."""

    def __init__(self, in_channels):
        self.b = _Builder(0, None)
        self.input = self.b.new_tensor(in_channels, 1, "input")
        self.layers = []

    def _keep(self, t):
        self.layers.append(t)
        return t

    def conv(self, x, filters, size, stride=1, bn=True, act="leaky", sub="body"):
        conf = {"filters": filters, "size": size, "stride": stride, "activation": act}
        if bn:
            conf["batch_normalize"] = 1
        return self._keep(self.b.conv(x, conf, sub))

    def shortcut(self, x, frm):
        return self._keep(self.b.shortcut(x, {"from": self.layers.index(frm), "activation": "linear"}, self.layers, "body"))

    def upsample(self, x):
        return self._keep(self.b.upsample(x, {"stride": 2}, "body"))

    def route(self, a, c):
        return self._keep(self.b.route({"source": {"layers": [self.layers.index(a), self.layers.index(c)]}}, None, self.layers, "body"))

    def program(self, outs):
        p = Program(self.b.tensors, self.b.nodes, [], self.input, list(outs), 0)
        p.conv_nodes = [n for n in self.b.nodes if n.kind == "conv"]
        _lower(p)
        return p


def tile_feature_program(bn, bk=32):
    """Every launch form a conv tile of N-width bn and K step bk can take, in one program on a [B,H,W,64] input (H, W even):

      a   3x3/1  64 -> wd, BN, leaky                       stored output, plain
      b   1x1    wd -> 64, BN, leaky                        (helper)
      c   3x3/1  64 -> wd, BN, linear, + a                  stored output, shortcut, no activation
      d   3x3/2  wd -> 64, BN, leaky       (reads c)        (helper: the half-resolution source)
      e   1x1    wd -> 64, BN, leaky       (reads c)        (helper: the full-resolution source)
      f   1x1    [up(d), e] -> wd, BN, leaky                stored output, two sources, the first up-sampled, C0 = 64
      h0  1x1    [e, b] -> nh0, bias, linear                head: two sources at one resolution, ragged N
      h1  3x3/2  wd -> bn, BN, leaky       (reads f)        head: stride 2, K = 9 wd
      h2  1x1    wd -> bn, BN, linear      (reads f)        head

    wd, the width of the stored tensors, is bn -- except for a tile narrower than its own K step (bn % bk != 0: the 128x32 bf16 tile
    with BK = 64), which could not read a bn-wide tensor back in h1 / h2: there wd = lcm(bn, bk), two N tiles of the launch.
    nh0 is one short of a padded width the tile divides: bn - 1, and 255 (the detection heads' own width) from bn = 128 on.
    Returns (program, {name: the ConvOp}), names as above."""
    wd = bn if bn % bk == 0 else bn * bk // np.gcd(bn, bk)
    nh0 = 255 if bn >= 128 else bn - 1
    g = _Graph(64)
    a = g.conv(g.input, wd, 3)
    b = g.conv(a, 64, 1)
    c = g.shortcut(g.conv(b, wd, 3, act="linear"), a)
    d = g.conv(c, 64, 3, stride=2)
    e = g.conv(c, 64, 1)
    f = g.conv(g.route(g.upsample(d), e), wd, 1)
    h0 = g.conv(g.route(e, b), nh0, 1, bn=False, act="linear", sub="head")
    h1 = g.conv(f, bn, 3, stride=2, sub="head")
    h2 = g.conv(f, bn, 1, act="linear", sub="head")
    p = g.program([h0, h1, h2])
    by_dst = {o.dst: o for o in p.conv_ops()}
    return p, {k: by_dst[t] for k, t in dict(a=a, b=b, c=c, d=d, e=e, f=f, h0=h0, h1=h1, h2=h2).items()}


def unfolded_program():
    """A graph none of whose add / upsample / concat folds into a conv launch, on a [B,H,W,64] input (H, W even):
    t2 = conv1x1(conv3x3(x)) feeds the add AND head 0, so the add stays on its own; the up-sampled tensor is read by a 3x3 conv and by
    head 1; the concat (64 + 32 = 96 channels) is read by a 3x3 conv, head 2.  Returns (program, {"add" | "upsample" | "concat": tensor id})."""
    g = _Graph(64)
    t1 = g.conv(g.input, 64, 3)
    t2 = g.conv(t1, 64, 1)
    add = g.shortcut(t2, t1)
    h0 = g.conv(t2, 32, 1, bn=False, act="linear", sub="head")
    d = g.conv(add, 32, 3, stride=2)
    up = g.upsample(d)
    e = g.conv(up, 64, 3)
    h1 = g.conv(up, 64, 1, sub="head")
    cat = g.route(e, up)
    h2 = g.conv(cat, 64, 3, act="linear", sub="head")
    return g.program([h0, h1, h2]), {"add": add, "upsample": up, "concat": cat}


def oracle_launch(O, op, weights, tensor, acc64=True, bf16_weights=False):
    """One fused conv launch restated with the oracle's separate layers, from the launch's own input tensors (tensor(id) -> fp32 NHWC):
    [upsample] [concat] conv [+ BN] [+ leaky] [+ shortcut], nothing rounded.  bf16_weights: the conv weights rounded to bf16 first."""
    x = tensor(op.src0)
    if op.src0_upsample:
        x = O.upsample2x(x)
    if op.src1 >= 0:
        x = O.concat(x, tensor(op.src1))
    i = op.conv_index
    w = {k: v for k, v in weights.items() if k.startswith(f"conv{i}.")}
    if bf16_weights:
        w[f"conv{i}.w"] = O.round_bf16(w[f"conv{i}.w"])
    y = O.conv_block(x, w, i, op.size, op.stride, op.bn, op.leaky, acc64)
    if op.residual >= 0:
        y = O.add(tensor(op.residual), y)
    return y


# The bars the parity suites hold a conv launch's fp32 output to, in one place so that the class-count suite
# (tests/test_class_counts_gpu.py) applies the very bars the 80-class tests apply.
NETWORK_GRID_BAR = 1e-4      # free-running fp32 head logits against the oracle, absolute (test_network_grids_match_oracle)


def f32_conv_bar(ref):
    """An fp32 output of one conv launch against the oracle on the same inputs: 2e-5 of the output's magnitude (fp32 with another
    summation order over K <= 4608).  test_conv_layers_match_oracle, the x3 / x2 layer tests, and the fp32 head outputs of the
    bf16 / fp16 teacher-forced tests."""
    return 2e-5 * max(1.0, float(np.abs(ref).max()))


def bf16_tile_bar(ref):
    """A forced bf16 tile's fp32 output against the bf16-emulating oracle, free running over one layer (test_bf16_every_tile)."""
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


def check_f32_conv(got, ref, what):
    """assert |got - ref|max <= f32_conv_bar(ref); -> (deviation, bar)."""
    err, bar = float(np.abs(got - ref).max()), f32_conv_bar(ref)
    assert err <= bar, (what, err, bar)
    return err, bar


# the per-tile matrix (tests/test_tile_matrix_gpu.py, tests/test_tile_matrix_host.py): one seed, three images, a square and a non-square canvas
TILE_MATRIX_SEED = 3
TILE_MATRIX_BATCH = 3
TILE_MATRIX_CANVASES = ((14, 14), (14, 10))    # M = 588 / 147 and 420 / 105: ragged against every BM, tiles span images; Ho != Wo


def tile_matrix_inputs(program, canvas):
    """(weights, fp32 input [3, H, W, 64]) of a tile_feature_program on `canvas`."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    h, w = canvas
    x = np.random.default_rng(TILE_MATRIX_SEED).standard_normal((TILE_MATRIX_BATCH, h, w, 64)).astype(np.float32)
    return synthetic_weights(program, seed=TILE_MATRIX_SEED), x


def nms_stress_set(rng, B, N, dup_frac=0.05, score_scale=1.0):
    """centres U(0,1), w,h log-normal(-2,0.8), scores Beta(0.5,4), 5 % exact duplicates of
    boxes and of scores (forces IoU == 1 and sort ties)."""
    cx, cy = rng.random((B, N)), rng.random((B, N))
    w = np.exp(rng.normal(-2.0, 0.8, (B, N)))
    h = np.exp(rng.normal(-2.0, 0.8, (B, N)))
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
    scores = (rng.beta(0.5, 4.0, (B, N)) * score_scale).astype(np.float32)
    nd = int(N * dup_frac)
    for b in range(B):
        src = rng.integers(0, N, nd)
        dst = rng.integers(0, N, nd)
        boxes[b, dst] = boxes[b, src]
        src = rng.integers(0, N, nd)
        dst = rng.integers(0, N, nd)
        scores[b, dst] = scores[b, src]
    return boxes, scores


import io  # noqa: E402
import os  # noqa: E402


def jpeg_bytes(rng, h, w):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=95)
    return buf.getvalue()


def make_tfrecord_dataset(dirpath, rng, n=5, sizes=((40, 56), (64, 64), (30, 90))):
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    payloads, truth = [], []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        k = i % 3          # 0, 1 or 2 boxes
        lo = rng.random((k, 2)).astype(np.float32) * 0.5
        hi = lo + 0.1 + rng.random((k, 2)).astype(np.float32) * 0.4
        names = [[b"circle", b"square", b"no such class"][j % 3] for j in range(k)]
        jpg = jpeg_bytes(rng, h, w)
        payloads.append(m.make_example({"image/encoded": jpg, "image/object/class/text": names,
                                        "image/object/bbox/xmin": lo[:, 0], "image/object/bbox/ymin": lo[:, 1],
                                        "image/object/bbox/xmax": hi[:, 0], "image/object/bbox/ymax": hi[:, 1]}))
        truth.append((jpg, lo, hi, names))
    m.write_records(os.path.join(dirpath, "a_00.tfrec"), payloads[:3])
    m.write_records(os.path.join(dirpath, "b_01.tfrec"), payloads[3:])
    return truth
