"""What tests/test_footprint_host.py and tests/test_footprint_gpu.py share: the FOOTPRINT of a launch -- that a call writes all of its own
tensor and nothing outside it -- as opposed to its values, which the parity suites hold to the oracle.

Three things are here.

1. The lane regions.  A forward on several lanes cuts every arena block into one region per lane (include/y3.h, y3_lane_offset: the
   function Slice::ptr evaluates).  sweep_sizes() / check_lane_regions() state what the regions must satisfy, over per-image sizes that
   are no multiple of 256 as well as the shipped networks' own; lane_chain_program() is the small graph that reaches such sizes on the
   device.

2. Guards.  guarded(shape, dtype) is one flat uint8 device allocation filled with the 32-bit word POISON (0x7FC5A5A5: a quiet NaN as
   fp32, an index above any class count as the low half of an int64, a count above any batch as int32) with the tensor a view of its
   middle.  Each guard is at least guard_bytes(): max(64 KiB, 256 rows of the tensor), rounded up to 256 bytes -- a missing row mask of
   the tallest tile (256 rows) or a missing column mask of the widest (256 columns < one more row) lands in memory the test owns and
   looks at.  A condition, not a measurement.  "Written": both guards hold POISON in every byte; no POISON word is left in the body
   (grids, boxes, class indices, scores, num_valid: every element of those is stored by the call); the body equals, bit for bit, the
   same call into an ordinary tensor.

3. The case table CASES of the guarded calls, with launches(): (M, Cout, tile width) of every conv launch of a case from y3_choose_tile
   and the Python mirrors of the tile tables, for the host file's conditions.

NumPy, the package's host code and the library's pure functions only; torch is imported where a device tensor is made."""
import functools
import os
from collections import namedtuple

import numpy as np

from yolo_v3_tf2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YOLO_MODEL = os.path.join(ROOT, "config", "models", "yolov3", "model.yaml")
YOLO_ANCHORS = os.path.join(ROOT, "datasets", "coco2012", "anchors.txt")

MODES = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16, "f32x3": _lib.Y3_DTYPE_F32X3,
         "f32x2": _lib.Y3_DTYPE_F32X2, "i8": _lib.Y3_DTYPE_I8}
# bytes per stored element of a plan's arena tensors (an int8 plan: fp16 before its cut, int8 behind it)
ELEM_BYTES = {"f32": (4,), "bf16": (2,), "f16": (2,), "f32x3": (6,), "f32x2": (4,), "i8": (2, 1)}
SEED = 4321            # the weights of the 80-class fixtures (tests/conftest.py)
IMAGE_SEED = 515

# ---------------------------------------------------------------------------------------------- 1. lane regions
MAX_LANES = 4
SLACK = 4096           # bytes behind every arena block (place_tensors)


def lane_starts(batch, lanes):
    """First image of every lane, and the end: the split of run() in csrc/y3_forward.cpp."""
    return [batch * l // lanes for l in range(lanes + 1)]


def old_lane_offset(block_bytes, batch, lanes, lane):
    """The rule before y3_lane_offset existed, kept to show what the sweep is for: every lane's start scaled to the block and rounded up on
    its own, so a start that was rounded up runs into the next one that was not."""
    if lanes > batch:
        return -1
    b0 = lane_starts(batch, lanes)[lane]
    return (int(float(block_bytes) * b0 / batch) + 255) & ~255 if lane else 0


@functools.lru_cache(maxsize=None)
def shipped_image_bytes():
    """Per-image bytes of every tensor of YOLOv3 and YOLOv3-tiny at 416^2 and 96^2, at the stored widths, in all six modes."""
    from yolo_v3_tf2_amd.graph import load_program
    from tests.tiny_cases import TINY_MODEL
    sizes = set()
    for model in (YOLO_MODEL, TINY_MODEL):
        p = load_program(model, 80)
        stored = list(p.stored) if p.stored else [t.channels for t in p.tensors]
        for S in (416, 96):
            for t, c in zip(p.tensors, stored):
                for ebs in ELEM_BYTES.values():
                    sizes.update((S // t.div) ** 2 * c * eb for eb in ebs)
    return tuple(sorted(sizes))


def sweep_sizes():
    """Per-image sizes of the lane sweep: every multiple of 16 up to 8192, and the shipped networks' own."""
    return tuple(range(16, 8192 + 1, 16)) + shipped_image_bytes()


def check_lane_regions(offset, image_bytes, max_batch, batch, lanes, block_bytes):
    """What the regions of one forward must satisfy; `offset` is y3_lane_offset (or a rule to be shown wrong).  -> None, or the first
    violated condition as text.

    A block of block_bytes holds max_batch images of some tensor of at most block_bytes / max_batch bytes each, so a lane of nb images
    of a forward of batch <= max_batch images writes at most nb * block_bytes / batch <= ceil(block_bytes * nb / batch) bytes whichever
    tensor shares the block.  (a) every offset is a multiple of 256; (b) off[l] + ceil(block_bytes * nb[l] / batch) <= off[l+1]: the
    regions nest for ANY such tensor; (b') the same with nb[l] * ceil(block_bytes / batch), the bound as first written down, wherever
    batch divides block_bytes -- where it does not, (b') contradicts (d): 8 images of 64 bytes, batch 6 on two lanes has
    block_bytes * 3 / 6 = 256 exactly and 3 * ceil(512 / 6) = 258; (b) is what disjointness needs; (b'') the tensor the sweep names:
    off[l] + nb[l] * image_bytes <= off[l+1]; (c) the last region ends within block_bytes + SLACK; (d) where block_bytes * start[l] /
    batch is a multiple of 256 for every lane the offsets are exactly those values: the shipped networks keep their addresses."""
    if lanes > batch:
        return None if all(offset(block_bytes, batch, lanes, l) == -1 for l in range(lanes)) else "lanes > batch must be refused"
    start = lane_starts(batch, lanes)
    off = [offset(block_bytes, batch, lanes, l) for l in range(lanes)]
    what = f"image_bytes {image_bytes} max_batch {max_batch} batch {batch} lanes {lanes} block {block_bytes}: offsets {off}"
    if off[0] != 0 or any(o < 0 or o % 256 for o in off):
        return "(a) " + what
    ends = off[1:] + [block_bytes + SLACK]
    for l in range(lanes):
        nb = start[l + 1] - start[l]
        if off[l] + -(-block_bytes * nb // batch) > ends[l]:
            return ("(b) " if l + 1 < lanes else "(c) ") + what
        if block_bytes % batch == 0 and off[l] + nb * -(-block_bytes // batch) > ends[l]:
            return "(b') " + what
        if off[l] + nb * image_bytes > ends[l]:
            return "(b'') " + what
    exact = [block_bytes * s // batch for s in start[:lanes]]
    if all(block_bytes * s % batch == 0 and e % 256 == 0 for s, e in zip(start, exact)) and off != exact:
        return "(d) " + what
    return None


def lane_sweep(offset, sizes=None):
    """The whole sweep -> (combinations checked, [the violations' texts]).  block_bytes: the tensor itself, and a reused block with a
    4096-aligned excess."""
    n, bad = 0, []
    for ib in sizes or sweep_sizes():
        for max_batch in range(1, 9):
            exact = max_batch * ib
            for block in (exact, (exact + 4096 + 4095) // 4096 * 4096):
                for batch in range(1, max_batch + 1):
                    for lanes in range(1, MAX_LANES + 1):
                        n += 1
                        r = check_lane_regions(offset, ib, max_batch, batch, lanes, block)
                        if r:
                            bad.append(r)
    return n, bad


def lane_chain_program():
    """Three 1x1 and 3x3 convs on a [B,5,5,64] input whose stored tensors have 32 and 96 channels, then three raw heads.  On 25 pixels no
    per-image size is a multiple of 256: 3200 (32 ch fp32; 64 ch bf16), 9600 (96 ch fp32), 4800 (96 ch bf16) and, in an int8 plan, a
    128-channel int8 tensor (3200 bytes) behind the cut.  -> {mode: program}."""
    from tests.helpers import mini_program
    heads = [dict(filters=64, size=1), dict(filters=32, size=3), dict(filters=64, size=1, bn=False, act="linear")]
    f32 = mini_program(64, [dict(filters=32, size=1), dict(filters=96, size=3), dict(filters=32, size=1)], heads)
    # the 16-bit tables have no tile for a 32-wide conv of K step 32: 64- and 128-channel tensors there (3200- and 6400-byte images)
    b16 = mini_program(64, [dict(filters=64, size=1), dict(filters=128, size=3), dict(filters=64, size=1)], heads)
    # int8: every conv behind the cut has Cin % 128 == 0 -- conv 1 (3x3, 128 -> 128) stores a 128-channel int8 tensor behind it
    i8 = mini_program(64, [dict(filters=128, size=1), dict(filters=128, size=3), dict(filters=128, size=1)],
                      [dict(filters=64, size=1), dict(filters=128, size=3), dict(filters=64, size=1, bn=False, act="linear")])
    return {"f32": f32, "bf16": b16, "i8": i8}


LANE_CHAIN_CANVAS = 5
LANE_CHAIN_BATCHES = (4, 6)


def stored_image_bytes(program, mode, canvas):
    """{tensor: per-image bytes in the arena} of the conv outputs a plan of `mode` stores (not the caller's grids)."""
    from yolo_v3_tf2_amd import quant
    h, w = (canvas, canvas) if isinstance(canvas, int) else canvas
    stored = list(program.stored) if program.stored else [t.channels for t in program.tensors]
    convs = program.conv_ops()
    cut = quant.first_i8_conv(program) if mode == "i8" else len(convs)
    out = {}
    for slot, o in enumerate(convs):
        if o.dst in program.outputs:
            continue
        eb = ELEM_BYTES[mode][0] if mode != "i8" else 1 if slot >= cut else 2
        t = program.tensors[o.dst]
        out[o.dst] = (h // t.div) * (w // t.div) * stored[o.dst] * eb
    return out


# ---------------------------------------------------------------------------------------------- 2. guards
POISON = 0x7FC5A5A5
MIN_GUARD = 64 * 1024
GUARD_ROWS = 256       # the tallest conv tile


def row_elems(shape):
    """Elements per row of the launch that writes the tensor: per pixel of [B,h,w,...], per box of [B,N,...], one of a vector."""
    k = 3 if len(shape) >= 4 else 2 if len(shape) == 3 else len(shape)
    return int(np.prod(shape[k:], dtype=np.int64))


def guard_bytes(shape, itemsize):
    need = max(MIN_GUARD, GUARD_ROWS * row_elems(shape) * itemsize)
    return (need + 255) // 256 * 256


Guarded = namedtuple("Guarded", "tensor buf lo hi")      # buf: the flat uint8 allocation; the tensor is buf[lo:hi]


def guarded(shape, dtype, guard=None):
    """A tensor of `shape` between two poisoned guards of `guard` bytes (default, and at least: guard_bytes)."""
    import torch
    itemsize = torch.empty((), dtype=dtype).element_size()
    need = guard_bytes(shape, itemsize)
    guard = need if guard is None else int(guard)
    assert guard >= need and guard % 256 == 0, (guard, need)
    body = int(np.prod(shape, dtype=np.int64)) * itemsize
    total = guard + (body + 255) // 256 * 256 + guard       # the body's round-up belongs to the guard behind it
    buf = torch.full((total // 4,), POISON, dtype=torch.int32, device="cuda").view(torch.uint8)
    return Guarded(buf[guard:guard + body].view(dtype).view(tuple(shape)), buf, guard, guard + body)


def _words(bytes_):
    import torch
    n = bytes_.numel() // 4 * 4
    return bytes_[:n].view(torch.int32)


def guards_intact(g):
    """Both guards hold POISON in every byte (the bytes between the body's end and the next word boundary are compared one by one)."""
    import torch
    pattern = torch.tensor([0xA5, 0xA5, 0xC5, 0x7F], dtype=torch.uint8, device=g.buf.device)
    ok = bool((_words(g.buf[:g.lo]) == POISON).all())
    tail = g.buf[g.hi:]
    head = (-g.hi) % 4
    if head:
        ok = ok and bool((tail[:head] == pattern[4 - head:]).all())
    return ok and bool((_words(tail[head:]) == POISON).all())


def poison_words(t):
    """How many aligned 32-bit words of tensor t (a view into a guarded buffer, or any contiguous tensor) hold POISON."""
    import torch
    return int((t.contiguous().view(torch.uint8).view(torch.int32) == POISON).sum())


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------- 3. the guarded calls
# call: the C entry the case guards; net: which program; mode; canvas: int or (H, W); max_batch and the batches run on the one plan;
# lanes; opts: what else the case switches (a dict as sorted items)
Case = namedtuple("Case", "name call net mode canvas max_batch batches lanes opts")
RECT = (64, 96)
RAW_CANVAS = (12, 20)
NC_BELOW, NC_INSIDE = 69, 75      # one below and one inside the 70..80 window of tests/class_count_cases.head_route


def _c(name, call, net, mode, canvas, max_batch, batches, lanes=(1,), **opts):
    return Case(name, call, net, mode, canvas, max_batch, tuple(batches), tuple(lanes), tuple(sorted(opts.items())))


def _cases():
    out = []
    for mode in MODES:       # y3_net_forward, YOLOv3, nc = 80
        for canvas, tag in ((96, "s96"), (RECT, "r64x96")):
            out.append(_c(f"forward_yolov3_{mode}_{tag}", "y3_net_forward", "yolov3_nc80", mode, canvas, 4, (3, 4), (1, 2)))
    for nc in (NC_BELOW, NC_INSIDE):      # class counts: the fp32 ragged-grid route and the fused one
        for mode in ("f32", "bf16"):
            out.append(_c(f"forward_yolov3_nc{nc}_{mode}", "y3_net_forward", f"yolov3_nc{nc}", mode, 96, 4, (3,)))
    # YOLOv3-tiny, two heads, the fused stem on and off -- off in fp32 alone: the 16-bit tables have no tile for the 32 -> 32 conv of
    # the stem at K step 32, so a bf16 or fp16 plan of tiny exists only with the stem fused (include/y3.h, y3_net_set_tiny_stem_fusion)
    for mode in ("f32", "bf16", "f16"):
        for fused in ((0, 1) if mode == "f32" else (1,)):
            out.append(_c(f"forward_tiny_{mode}_stem{fused}", "y3_net_forward", "tiny_nc80", mode, 96, 4, (3,), tiny_stem=fused))
    # raw-feature programs (nclasses = 0); the 16-bit one's staged outputs go through launch_to_f32.  unfolded_program runs in fp32
    # alone: its stand-alone add is fp32 arithmetic and a 16-bit forward refuses it (tests/test_f16_gpu.py)
    out.append(_c("forward_tile64_f32", "y3_net_forward", "tile64", "f32", RAW_CANVAS, 3, (3,)))
    out.append(_c("forward_tile64_bf16", "y3_net_forward", "tile64", "bf16", RAW_CANVAS, 3, (3,)))
    out.append(_c("forward_unfolded_f32", "y3_net_forward", "unfolded", "f32", RAW_CANVAS, 3, (3,)))
    for mode in ("f32", "bf16"):          # boxes, class indices, scores: 27 pixels of the coarsest grid in a 64-pixel tile
        out.append(_c(f"forward_decode_{mode}", "y3_net_forward_decode", "yolov3_nc80", mode, 96, 4, (3,), (1, 2)))
    for call in ("y3_net_detect", "y3_net_detect_grids"):
        for mode in ("f32", "bf16"):
            for per_class in (0, 1):
                out.append(_c(f"{call[7:]}_{mode}_nms{per_class}", call, "yolov3_nc80", mode, 96, 4, (3,), per_class=per_class))
        out.append(_c(f"{call[7:]}_f32_multilabel", call, "yolov3_nc80", "f32", 96, 4, (3,), multi_label=1, per_class=1))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# every (call, network family, mode) the table must hold: tests/test_footprint_host.py compares
REQUIRED = (
    [("y3_net_forward", "yolov3_nc80", m) for m in MODES]
    + [("y3_net_forward", f"yolov3_nc{nc}", m) for nc in (NC_BELOW, NC_INSIDE) for m in ("f32", "bf16")]
    + [("y3_net_forward", "tiny_nc80", m) for m in ("f32", "bf16", "f16")]
    + [("y3_net_forward", "tile64", "f32"), ("y3_net_forward", "tile64", "bf16"), ("y3_net_forward", "unfolded", "f32")]
    + [(c, "yolov3_nc80", m) for c in ("y3_net_forward_decode", "y3_net_detect", "y3_net_detect_grids") for m in ("f32", "bf16")])


@functools.lru_cache(maxsize=None)
def program(net):
    """The program of a case's `net` key."""
    from yolo_v3_tf2_amd.graph import load_program
    if net.startswith("yolov3_nc"):
        return load_program(YOLO_MODEL, int(net[len("yolov3_nc"):]))
    if net == "tiny_nc80":
        from tests.tiny_cases import tiny_program
        return tiny_program(80)
    from tests.helpers import tile_feature_program, unfolded_program
    return {"tile64": lambda: tile_feature_program(64)[0], "unfolded": lambda: unfolded_program()[0]}[net]()


@functools.lru_cache(maxsize=None)
def weights(net):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    w = synthetic_weights(program(net), seed=SEED)
    for v in w.values():
        v.setflags(write=False)
    return w


def canvas_hw(canvas):
    return (canvas, canvas) if isinstance(canvas, int) else tuple(canvas)


@functools.lru_cache(maxsize=None)
def images(net, canvas, batch):
    """fp32 input batch of a case, read-only: images in [0, 1) for a 3-channel input, N(0, 1) features otherwise (the first images of a
    larger batch are those of a smaller one)."""
    h, w = canvas_hw(canvas)
    cin = program(net).tensors[program(net).input_tensor].channels
    rng = np.random.default_rng(IMAGE_SEED)
    x = np.stack([rng.random((h, w, cin), dtype=np.float32) if cin == 3 else rng.standard_normal((h, w, cin)).astype(np.float32)
                  for _ in range(batch)])
    x.setflags(write=False)
    return x


def anchors(net):
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from tests.tiny_cases import TINY_ANCHORS
    return get_anchors(TINY_ANCHORS if net.startswith("tiny") else YOLO_ANCHORS).astype(np.float32)


def grid_shapes(case, batch):
    """Shapes of the caller's grids of a case for `batch` images."""
    p = program(case.net)
    h, w = canvas_hw(case.canvas)
    stored = [t.channels for t in p.tensors]
    out = []
    for o in p.outputs:
        gh, gw = h // p.tensors[o].div, w // p.tensors[o].div
        out.append((batch, gh, gw, 3, 5 + p.nclasses) if p.nclasses > 0 else (batch, gh, gw, stored[o]))
    return out


def n_boxes(case):
    return sum(3 * s[1] * s[2] for s in grid_shapes(case, 1))


_TABLE = {"f32": _lib.TILES, "bf16": _lib.TILES_BF16, "f16": _lib.TILES_BF16, "i8": _lib.TILES_BF16, "f32x3": _lib.TILES_X3,
          "f32x2": _lib.TILES_X3}


def launches(case, batch):
    """[(conv slot, M, Cout, tile width or None)] of the conv launches of a one-lane forward of `batch` images: M = batch * Ho * Wo rows;
    the tile y3_choose_tile gives the conv at those rows in the case's mode (an int8 plan: fp16 before its cut), its N width from the
    table's mirror; None for a conv that launches no tile of the table (the Cin = 3 first layer, a conv without a 16-bit tile inside the
    fused tiny stem).  A conv inside the fused YOLOv3 stem is listed with the tile it takes when the stem is not fused."""
    from yolo_v3_tf2_amd import quant
    lib = _lib.load()
    p = program(case.net)
    h, w = canvas_hw(case.canvas)
    convs = p.conv_ops()
    cut = quant.first_i8_conv(p) if case.mode == "i8" else len(convs)
    out = []
    for slot, o in enumerate(convs):
        M, M_plan = batch * (h // o.out_div) * (w // o.out_div), case.max_batch * (h // o.out_div) * (w // o.out_div)
        if o.cin == 3:
            out.append((slot, M, o.cout, None))
            continue
        dtype = MODES[case.mode] if case.mode != "i8" or slot >= cut else _lib.Y3_DTYPE_F16
        t = lib.y3_choose_tile(dtype, o.size, o.stride, o.cin, o.c0 if o.src1 >= 0 else -1, o.cout, M, M_plan, int(o.dst not in p.outputs))
        assert t >= 0 or (t == -1 and dict(case.opts).get("tiny_stem")), (case.name, slot, t)      # -1: a conv inside the fused tiny stem
        out.append((slot, M, o.cout, _TABLE[case.mode][t][1] if t >= 0 else None))
    return out


def guarded_outputs(case):
    """[(what, shape, dtype name)] of the caller-owned outputs a case puts between guards, allocated for max_batch images where the case
    looks at the images behind the call's batch (the grids of y3_net_forward), else for the call's batch."""
    B = max(case.batches)
    shapes = grid_shapes(case, case.max_batch if case.call == "y3_net_forward" else B)
    opts = dict(case.opts)
    if case.call == "y3_net_forward":
        return [(f"grid{k}", s, "float32") for k, s in enumerate(shapes)]
    N = n_boxes(case)
    if case.call == "y3_net_forward_decode":
        return [("boxes", (B, N, 4), "float32"), ("cls", (B, N), "int64"), ("scores", (B, N), "float32")]
    outs = [("packed", (B, MAX_BOXES, 7), "int32"), ("num_valid", (B,), "int32")]
    if case.call == "y3_net_detect_grids":
        outs += [(f"grid{k}", s, "float32") for k, s in enumerate(shapes)]
    assert not opts.get("tiny_stem")
    return outs


MAX_BOXES, IOU, SCORE = 100, 0.5, 0.1      # the detect cases' NMS arguments (those of smoke())

# ---------------------------------------------------------------------------------------------- stand-alone ops
# ops.maxpool2x2(out=): (shape, stride); every element type on each
POOL_CASES = (((3, 13, 13, 32), 1), ((3, 6, 10, 64), 2), ((2, 4, 4, 8), 1), ((2, 4, 4, 8), 2))
POOL_DTYPES = ("float32", "bfloat16", "float16")
DECODE_GRIDS = (2, 4, 8)
DECODE_NC = (7, 80)
DECODE_BATCH = 3


def decode_grids(nc, batch=DECODE_BATCH):
    """Three random grids [batch, g, g, 3, 5 + nc] for g in DECODE_GRIDS, logits N(0, 2)."""
    rng = np.random.default_rng(IMAGE_SEED + nc)
    return [(2.0 * rng.standard_normal((batch, g, g, 3, 5 + nc))).astype(np.float32) for g in DECODE_GRIDS]


# ---------------------------------------------------------------------------------------------- arena tensors beyond the call's batch
BEYOND_MAX_BATCH, BEYOND_BATCH = 5, 3
BEYOND_NETS = [("yolov3_nc80", m) for m in MODES] + [("tiny_nc80", m) for m in ("f32", "bf16", "f16")]
BEYOND_STEMS = [(f, m) for f in ("stem", "tiny") for m in ("f32", "bf16", "f16")]
