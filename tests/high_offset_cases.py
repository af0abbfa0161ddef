"""The cases of tests/test_high_offsets_host.py and tests/test_high_offsets_gpu.py: conv launches whose operands lie between 2 GiB and the
4 GiB guard of y3_net_plan_hw, where every byte offset has bit 31 set -- and, for int8, the element index itself passes 2^31.

A high offset is a property of the byte offset, not of the image: the canvas stays 14 x 10 (16 x 10 where a two-lane case needs an odd batch) and the batch goes to tens of thousands, so a
host reference of the few images a case checks costs milliseconds.  Everything here is arithmetic on the program's own tensor table (channels,
divisor, element size of the plan); NumPy only, no library call and no GPU.

Programs.  tests/helpers.tile_feature_program cannot carry a 16-bit destination past 2 GiB: its full-resolution fp32 heads are as wide as
its stored tensors, twice their bytes, and pass 4 GiB first.  body_program is the same body (plain 3x3, 1x1, 3x3 + shortcut without
activation, stride 2, two sources with the first up-sampled) with the three heads at half resolution, and with the widths open: in its
"uniform" form (every stored tensor wd channels, the half-resolution one 4 wd) all stored tensors have ONE size, so one batch puts the
destination, the single source, the second source, the up-sampled first source and the shortcut operand above 2 GiB together.
guard_program is the smallest program in which a 3x3 / stride-1 launch reads a tensor that ends within one image of the guard; on a
three-channel input that launch is conv_first.  The fused stems have no case: STEM_FAMILIES says why."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from tests.helpers import _Graph
from yolo_v3_tf2_amd import _lib

GUARD = 0xFFFFFFF0          # y3_net_plan_hw refuses a tensor of this many bytes or more
HIGH = 1 << 31
BUDGET = 24 << 30           # summed bytes of a case's plan, input and outputs included: the machines are shared
CANVAS = (14, 10)           # 140 positions: ragged against every BM, tiles span images, Ho != Wo
SEED = 31

ROLES = ("destination", "single_source", "second_source", "upsampled_first_source", "shortcut", "f32_grid", "staged_to_f32", "quantize_cut")

# mode -> plan dtype, bytes per stored element (the planes of x3 / x2 counted in), tile table, the generic tile ids of the per-tile suites,
# setter, K step (None: column 3 of the table), the multiple Cout is padded to
MODES = {
    "f32": dict(dtype=_lib.Y3_DTYPE_F32, eb=4, table=_lib.TILES, setter="set_tile", bk=32, pad=32, resident=33,
                tiles=[t for t in range(len(_lib.TILES)) if t not in _lib.RETIRED_TILES and t != 33]),
    "bf16": dict(dtype=_lib.Y3_DTYPE_BF16, eb=2, table=_lib.TILES_BF16, setter="set_tile_bf16", bk=None, pad=32, resident=32,
                 tiles=[t for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32]),
    "f16": dict(dtype=_lib.Y3_DTYPE_F16, eb=2, table=_lib.TILES_BF16, setter="set_tile_bf16", bk=None, pad=32, resident=32,
                tiles=[t for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32]),
    "f32x3": dict(dtype=_lib.Y3_DTYPE_F32X3, eb=6, table=_lib.TILES_X3, setter="set_tile_x3", bk=32, pad=64, resident=None,
                  tiles=list(_lib.TILES_X3_BUILT)),
    "f32x2": dict(dtype=_lib.Y3_DTYPE_F32X2, eb=4, table=_lib.TILES_X3, setter="set_tile_x2", bk=32, pad=64, resident=None,
                  tiles=list(_lib.TILES_X2_BUILT)),
    "i8": dict(dtype=_lib.Y3_DTYPE_I8, eb=1, table=_lib.TILES_BF16, setter="set_tile_bf16", bk=128, pad=64, resident=None,
               tiles=list(_lib.TILES_I8_BUILT)),
}

# family -> the operand roles a launch of it can have above 2 GiB under the guard.  What is left out, and why:
#   f32_resident (tile 33: Cin = 32, Cout % 64 == 0): its source is at most half its destination, so it cannot pass 2 GiB under the guard;
#       single source only.  The 16-bit resident kernel (Cin = 64 -> 64) can; it has no second source either.
#   f32_border_skip: single-source 3x3 convs only (y3::resolve_border).
#   fp32 plans store fp32 everywhere: no "f32_grid" of another format, nothing staged.  An int8 plan converts a staged output with
#       i8_to_f32, not to_f32_kernel; quantize_cut is the fp16 tensor read by quantize16_to_i8 (its int8 copy is half its bytes).
_CONV5 = ("destination", "single_source", "second_source", "upsampled_first_source", "shortcut")
FAMILY_ROLES = {
    "f32_generic": _CONV5,
    "f32_resident": ("destination", "shortcut"),
    "f32_border_skip": ("destination", "single_source", "shortcut"),
    "bf16_conv16": _CONV5 + ("f32_grid", "staged_to_f32"),
    "f16_conv16": _CONV5 + ("f32_grid", "staged_to_f32"),
    "i8_conv16": _CONV5 + ("f32_grid", "quantize_cut"),
    "bf16_resident": ("destination", "single_source", "shortcut"),
    "f16_resident": ("destination", "single_source", "shortcut"),
    "f32x3": _CONV5 + ("f32_grid", "staged_to_f32"),
    "f32x2": _CONV5 + ("f32_grid", "staged_to_f32"),
    # conv_first (the Cin = 3 layer, one instantiation per format it stores): its destination only -- its source, the fp32 image, has
    # 12 bytes a pixel against the destination's 64 or more, so it stays under 0.75 GiB (test_conv_first_source_cannot_be_high)
    "conv_first_f32": ("destination",), "conv_first_bf16": ("destination",), "conv_first_f16": ("destination",),
    "conv_first_f32x3": ("destination",), "conv_first_f32x2": ("destination",),
}
# The fused stems have NO operand a plan under the guard can put above 2 GiB: y3_net_plan_hw sizes conv0's own destination
# [B,H,W,32] although the fused kernel keeps it on chip, and refuses it at 0xFFFFFFF0 bytes; the stem's first destination (conv1's
# output [B,H/2,W/2,64]) is exactly half of it, its second (the 1x1 after conv1, [B,H/2,W/2,32]) a quarter, its source (the fp32 image)
# at most 3/16.  family -> bytes per stored element; tests/test_high_offsets_host.py proves the bound, the GPU file the refusal.
STEM_FAMILIES = {"conv_stem_f32": 4, "conv_stem16_bf16": 2, "conv_stem16_f16": 2}
FIRST = -1                  # forcing(): the Cin = 3 conv, which runs conv_first and takes no tile
# family -> (mode, the tile ids it can launch: each must have its destination high in some case)
FAMILY_TILES = {
    "f32_generic": ("f32", MODES["f32"]["tiles"]), "f32_resident": ("f32", [33]), "f32_border_skip": ("f32", []),
    "bf16_conv16": ("bf16", MODES["bf16"]["tiles"]), "f16_conv16": ("f16", MODES["f16"]["tiles"]), "i8_conv16": ("i8", MODES["i8"]["tiles"]),
    "bf16_resident": ("bf16", [32]), "f16_resident": ("f16", [32]),
    "f32x3": ("f32x3", MODES["f32x3"]["tiles"]), "f32x2": ("f32x2", MODES["f32x2"]["tiles"]),
    "conv_first_f32": ("f32", []), "conv_first_bf16": ("bf16", []), "conv_first_f16": ("f16", []),
    "conv_first_f32x3": ("f32x3", []), "conv_first_f32x2": ("f32x2", []),
}


# ------------------------------------------------------------------------------------------------ programs
def body_program(cin, wd, mid, dch, hw, heads="half", out_c=False):
    """On a [B,H,W,cin] input (H, W even):

      a   3x3/1  cin -> wd, BN, leaky                     plain
      b   1x1    wd -> mid, BN, leaky       (reads a)      single source
      c   3x3/1  mid -> wd, BN, linear, + a                shortcut, no activation
      d   3x3/2  wd -> dch, BN, leaky       (reads c)      stride 2: the half-resolution source
      e   1x1    wd -> mid, BN, leaky       (reads c)
      f   1x1    [up(d), e] -> wd, BN, leaky               two sources, the first up-sampled
      h0  3x3/2  wd -> hw - 1, bias, linear (reads f)      fp32 head, ragged N
      h1  3x3/2  wd -> hw, BN, leaky        (reads f)      fp32 head
      h2  1x1    dch -> hw, BN, linear      (reads d)      fp32 head; heads = "full": 1x1 wd -> hw reading f, a full-resolution fp32 grid

    out_c: h2 is left out and c itself is the third output -- written by a shortcut conv and read again, so a non-fp32 plan stages it and
    converts it at the end of the forward.  Returns (program, {name: ConvOp})."""
    g = _Graph(cin)
    a = g.conv(g.input, wd, 3)
    b = g.conv(a, mid, 1)
    c = g.shortcut(g.conv(b, wd, 3, act="linear"), a)
    d = g.conv(c, dch, 3, stride=2)
    e = g.conv(c, mid, 1)
    f = g.conv(g.route(g.upsample(d), e), wd, 1)
    h0 = g.conv(f, hw - 1, 3, stride=2, bn=False, act="linear", sub="head")
    h1 = g.conv(f, hw, 3, stride=2, sub="head")
    named = dict(a=a, b=b, c=c, d=d, e=e, f=f, h0=h0, h1=h1)
    if out_c:
        outs = [h0, h1, c]
    else:
        named["h2"] = g.conv(f if heads == "full" else d, hw, 1, act="linear", sub="head")
        outs = [h0, h1, named["h2"]]
    p = g.program(outs)
    by_dst = {o.dst: o for o in p.conv_ops()}
    return p, {k: by_dst[t] for k, t in named.items()}


def guard_program(cin, wd, hw, lead_1x1=False):
    """x -> [a 1x1 cin -> wd ->] s 3x3/1 -> wd -> three 3x3/2 heads (hw - 1 with bias, hw, hw).  The 3x3 / stride-1 launch s reads the
    input, or with lead_1x1 (int8: the launch must read an int8 tensor) the tensor a.  Returns (program, {name: ConvOp})."""
    g = _Graph(cin)
    named = {}
    x = g.input
    if lead_1x1:
        x = named["a"] = g.conv(x, wd, 1)
    s = named["s"] = g.conv(x, wd, 3)
    named["h0"] = g.conv(s, hw - 1, 3, stride=2, bn=False, act="linear", sub="head")
    named["h1"] = g.conv(s, hw, 3, stride=2, sub="head")
    named["h2"] = g.conv(s, hw, 3, stride=2, act="linear", sub="head")
    p = g.program([named["h0"], named["h1"], named["h2"]])
    by_dst = {o.dst: o for o in p.conv_ops()}
    return p, {k: by_dst[t] for k, t in named.items()}


# ------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    family: str
    mode: str
    tiles: Tuple[int, ...]               # per conv the first of these that fits is forced; tiles[0] is the tile under test
    kind: str                            # "body" | "guard"
    args: dict
    batch: int
    lanes: int = 1
    border_skip: bool = False
    canvas: Tuple[int, int] = CANVAS
    near_guard: Optional[str] = None     # the conv whose source ends within one image of the guard
    batch_independent: bool = True       # every family here runs an image the same way in any batch: forced tiles, no sum split by batch
    _built: tuple = field(default=None, repr=False, compare=False)

    def program(self):
        if self._built is None:
            self._built = (body_program if self.kind == "body" else guard_program)(**self.args)
        return self._built


def staged_outputs(p):
    """y3::output_staged: the outputs a non-fp32 plan keeps in its own format and converts at the end of the forward."""
    convs = p.conv_ops()
    return {t for t in p.outputs if any(t in (o.src0, o.src1, o.residual) or (o.dst == t and (o.residual >= 0 or o.cin == 3)) for o in convs)}


def elem_bytes(case, t):
    """Bytes per element of tensor t as the launches address it (Slice::elem_bytes): an fp32 grid 4, everything else the plan's format --
    an int8 plan of these programs cuts before conv 0: its input is fp16, every stored tensor int8.  The three-channel input of a
    conv_first case is the fp32 image in every mode."""
    p, _ = case.program()
    if t == p.input_tensor and p.tensors[t].channels == 3:
        return 4
    if t in p.outputs and (case.mode == "f32" or t not in staged_outputs(p)):
        return 4
    if case.mode == "i8":
        return 2 if t == p.input_tensor else 1
    return MODES[case.mode]["eb"]


def image_bytes(case, t):
    p, _ = case.program()
    h, w = case.canvas
    return (h // p.tensors[t].div) * (w // p.tensors[t].div) * p.tensors[t].channels * elem_bytes(case, t)


def plan_tensors(case):
    """The tensors a plan of the case touches: the input, every conv destination."""
    p, _ = case.program()
    return [p.input_tensor] + [o.dst for o in p.conv_ops()]


def tensor_bytes(case, t, images=None):
    return (case.batch if images is None else images) * image_bytes(case, t)


def total_bytes(case):
    """All tensors of the plan (activations kept: one block each), the input and the outputs; an int8 plan's int8 copy of its input; the
    fp32 grid a staged output is converted into; the largest whole-batch copy read_tensor makes of a stored tensor while the test
    slices the checked images out of it (fp32, an int8 plan's in int8), one at a time."""
    p, _ = case.program()
    n = sum(tensor_bytes(case, t) for t in plan_tensors(case))
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs] + ([p.input_tensor] if case.mode == "i8" else [])
    n += max(tensor_bytes(case, t) // elem_bytes(case, t) * (1 if case.mode == "i8" else 4) for t in stored)
    if case.mode == "i8":
        n += tensor_bytes(case, p.input_tensor) // 2
    if case.mode != "f32":
        n += sum(tensor_bytes(case, t) // elem_bytes(case, t) * 4 for t in staged_outputs(p))
    return n


def lane_ranges(case):
    """[(first image, images)] of the sub-batches of a forward (y3_net_forward: start[l] = batch * l / lanes)."""
    s = [case.batch * l // case.lanes for l in range(case.lanes + 1)]
    return [(s[l], s[l + 1] - s[l]) for l in range(case.lanes)]


def high_tensors(case):
    """{tensor: (first image of the launch's view, images in it)} of the tensors that pass 2 GiB in ONE launch's view: with lanes every
    sub-batch addresses its own images from offset 0, so the view is the lane's -- the last lane's, the largest."""
    b0, nb = lane_ranges(case)[-1]
    return {t: (b0, nb) for t in plan_tensors(case) if tensor_bytes(case, t, nb) > HIGH}


def straddle_image(case, t):
    """The image of tensor t whose bytes hold offset 2^31 of the launch's view."""
    b0, _ = high_tensors(case)[t]
    return b0 + HIGH // image_bytes(case, t)


def checked_images(case):
    """Image 0 (low addresses), the first image of the last lane, of every high tensor the image across offset 2^31, the last image."""
    imgs = {0, lane_ranges(case)[-1][0], case.batch - 1}
    imgs.update(straddle_image(case, t) for t in high_tensors(case))
    return sorted(imgs)


def _fits(case, o, tile):
    m = MODES[case.mode]
    p, _ = case.program()
    if tile == m["resident"]:
        if case.mode == "f32":
            return o.size == 3 and o.stride == 1 and o.src1 < 0 and o.cin == 32 and o.cout % 64 == 0
        fp32_out = o.dst in p.outputs and o.dst not in staged_outputs(p)
        return o.size == 3 and o.stride == 1 and o.src1 < 0 and o.cin in (32, 64) and o.cout % 64 == 0 and not fp32_out
    row = m["table"][tile]
    bk = m["bk"] if m["bk"] is not None else row[3]
    cout_pad = -(-o.cout // m["pad"]) * m["pad"]
    return row[0] > 0 and o.cin % bk == 0 and cout_pad % row[1] == 0 and (o.src1 < 0 or o.c0 % bk == 0)


def forcing(case):
    """{conv slot: tile id}: per conv the first tile of case.tiles that divides it (y3::tile_fits and the resident kernels' rules).
    Every conv of every case gets one, so no launch is left to a heuristic that looks at the batch."""
    p, _ = case.program()
    out = {}
    for slot, o in enumerate(p.conv_ops()):
        out[slot] = FIRST if o.cin == 3 else next((t for t in case.tiles if _fits(case, o, t)), None)
    return out


def roles(case):
    """{(role, tile id)}: what the case puts above 2 GiB, per launch, with the tile the launch is forced to."""
    p, _ = case.program()
    high, staged, force = high_tensors(case), staged_outputs(p), forcing(case)
    out = set()
    for slot, o in enumerate(p.conv_ops()):
        t = force[slot]
        # the launches of the case's own family: the resident kernel's in a resident case, the single-source 3x3 convs with the border skip
        if (t == MODES[case.mode]["resident"]) != case.family.endswith("resident") or (case.border_skip and not (o.size == 3 and o.src1 < 0)):
            continue
        if (o.cin == 3) != case.family.startswith("conv_first"):      # a conv_first case counts its Cin = 3 launch alone
            continue
        if o.dst in high:
            grid = o.dst in p.outputs and o.dst not in staged
            out.add(("f32_grid" if grid and case.mode != "f32" else "destination", t))
        if o.src0 in high:
            out.add(("upsampled_first_source" if o.src0_upsample else "single_source" if o.src1 < 0 else "first_source", t))
        if o.src1 in high:
            out.add(("second_source", t))
        if o.residual in high:
            out.add(("shortcut", t))
        if case.mode == "i8" and o.src0 == p.input_tensor and p.input_tensor in high:
            out.add(("quantize_cut", None))
    if case.mode != "f32" and any(t in high for t in staged):
        out.add(("staged_to_f32", None))
    return out


def _batch_over(img_bytes, factor):
    return int(np.ceil(factor * HIGH / img_bytes)) + 1


def _uniform(mode, wd, **kw):
    """body_program with every stored tensor of one size: cin 64 (int8: 128, wd 256)."""
    cin = 128 if mode == "i8" else 64
    return dict(cin=cin, wd=wd, mid=wd, dch=4 * wd, hw=wd, **kw)


def _case(name, family, mode, tiles, kind, args, key, factor=(1.2, 1.1, 1.05, 1.01), **kw):
    """The batch that puts tensor `key` (a name of the program) at factor x 2 GiB: the largest factor under the budget."""
    c = Case(name, family, mode, tuple(tiles), kind, args, 1, **kw)
    _, ops = c.program()
    img = image_bytes(c, ops[key].dst)
    for f in factor:
        c.batch = _batch_over(img, f)
        if total_bytes(c) < BUDGET:
            break
    return c


# base tiles by width, behind the tile under test: whatever the program holds gets a forced tile
_BASE = {"f32": (11, 8), "bf16": (11, 4, 6), "f16": (11, 4, 6), "f32x3": (2,), "f32x2": (2,), "i8": (11,)}


def _all_cases():
    out = []
    # 1. every generic tile of every mode: uniform program, every conv on the tile
    for fam, (mode, tiles) in FAMILY_TILES.items():
        if fam.endswith("resident") or fam == "f32_border_skip":
            continue
        for t in tiles:
            wd = 256 if mode == "i8" else max(64, MODES[mode]["table"][t][1])
            out.append(_case(f"{mode}-t{t}", fam, mode, (t,) + _BASE[mode], "body", _uniform(mode, wd), "a"))
    # 2. the weight-resident 3x3 kernels: fp32 tile 33 needs Cin = 32 (a and c: 32 -> 64); the 16-bit tile 32 takes a and c of the uniform program
    out.append(_case("f32-t33", "f32_resident", "f32", (33, 11, 8), "body", dict(cin=32, wd=64, mid=32, dch=128, hw=64), "a"))
    for mode in ("bf16", "f16"):
        out.append(_case(f"{mode}-t32", f"{mode}_resident", mode, (32,) + _BASE[mode], "body", _uniform(mode, 64), "a"))
    # 3. batch-minor border-skip rows: lane batches of whole 32-image groups
    c = _case("f32-border-skip", "f32_border_skip", "f32", (11, 8), "body", _uniform("f32", 64), "a", border_skip=True)
    c.batch = -(-c.batch // 32) * 32
    out.append(c)
    # 4. an fp32 grid stored by a non-fp32 launch: the full-resolution head h2 at 1.2 x 2 GiB; only a, c, f stay wide (the budget)
    #    (int8 needs no case of its own: the half-resolution fp32 heads of its uniform program, 256 channels wide, are high already)
    for mode, fam, t in (("bf16", "bf16_conv16", 8), ("f16", "f16_conv16", 12), ("f32x3", "f32x3", 0), ("f32x2", "f32x2", 4)):
        args = dict(cin=64, wd=128, mid=64, dch=64, hw=128, heads="full")
        out.append(_case(f"{mode}-grid", fam, mode, (t,) + _BASE[mode], "body", args, "h2"))
    # 5. a staged output, converted by to_f32_kernel at the end of the forward
    for mode, fam in (("bf16", "bf16_conv16"), ("f16", "f16_conv16"), ("f32x3", "f32x3"), ("f32x2", "f32x2")):
        args = dict(cin=64, wd=64, mid=64, dch=64, hw=64, out_c=True)
        out.append(_case(f"{mode}-staged", fam, mode, _BASE[mode], "body", args, "c"))
    # 6. two lanes: the second lane alone holds a high tensor.  The whole tensor must stay under the guard, so the lane passes 2 GiB only
    #    when the batch is odd and ends within one image of the guard: B = floor((guard - 1) / image bytes), on a canvas where that is odd.
    #    guard_program (the budget: the read of a stored tensor is a whole-batch fp32 copy on top of the plan): a 3x3 / stride-1 launch
    #    whose source and destination both pass 2 GiB in the second lane's view, and three stride-2 heads.
    for mode, fam in (("f32", "f32_generic"), ("bf16", "bf16_conv16")):
        for canvas in ((14, 10), (14, 14), (10, 10), (12, 10), (12, 14), (10, 14), (16, 10), (12, 12), (16, 14), (10, 6), (18, 10)):
            c = Case(f"{mode}-lanes2", fam, mode, _BASE[mode], "guard", dict(cin=64, wd=64, hw=32), 1, lanes=2, canvas=canvas)
            _, ops = c.program()
            c.batch = (GUARD - 1) // image_bytes(c, ops["s"].dst)
            if c.batch % 2 == 1 and high_tensors(c) and total_bytes(c) < BUDGET:
                out.append(c)
                break
    # 7. near the guard, one case per element size: the source of a 3x3 / stride-1 launch ends within one image of 0xFFFFFFF0
    for mode, fam, args in (("f32", "f32_generic", dict(cin=64, wd=64, hw=32)), ("bf16", "bf16_conv16", dict(cin=64, wd=64, hw=32)),
                            ("i8", "i8_conv16", dict(cin=128, wd=256, hw=64, lead_1x1=True))):
        c = Case(f"{mode}-near-guard", fam, mode, _BASE[mode], "guard", args, 1, near_guard="s")
        _, ops = c.program()
        c.batch = (GUARD - 1) // image_bytes(c, ops["s"].src0)
        out.append(c)
    # 8. conv_first in every format it stores: the Cin = 3 layer of guard_program, its [B,H,W,32] destination at 1.2 x 2 GiB
    for mode in ("f32", "bf16", "f16", "f32x3", "f32x2"):
        out.append(_case(f"{mode}-conv-first", f"conv_first_{mode}", mode, _BASE[mode], "guard", dict(cin=3, wd=32, hw=64), "s"))
    return out


CASES = _all_cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def coverage():
    """-> ({(family, role)} the cases put above 2 GiB, {(family, tile)} with the tile's destination -- stored, or an fp32 grid -- above 2 GiB)."""
    pairs, tiles = set(), set()
    for c in CASES:
        for role, t in roles(c):
            pairs.add((c.family, role))
            if role in ("destination", "f32_grid") and t is not None:
                tiles.add((c.family, t))
    return pairs, tiles


# ------------------------------------------------------------------------------------------------ bars (restated from the per-tile suites)
def bf16_ulp_elem(a, b):
    """tests/test_tile_matrix_gpu.py: per element, the spacing of bf16 numbers in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


DIFFER_CAP = {"bf16": 2e-3, "f16": 1e-2}      # the share of a launch's stored elements that may differ at all (the per-tile suites' caps)
