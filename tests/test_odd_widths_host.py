"""Tile choice at conv widths outside YOLOv3's own (no GPU): y3_choose_tile, the heuristic of every plan mode through the functions the
launch decision calls, swept over Cin, the concat boundary c0, Cout, the rows of the call and of the plan, and judged against the Python
mirrors of the tile tables (_lib.TILES*) and the rule of y3::tile_fits restated here.  A chooser may never name a tile that does not
divide the conv while a built one does; where none does it says -1 and y3_net_plan refuses the mode (tests/test_odd_widths_gpu.py).
The network's own 75 convs keep the ids of the chooser before this sweep existed (tests/golden/yolov3_heuristic_tiles.json).
Also here: the lowering the GPU file relies on, and the condition under which its caps on differing 16-bit elements mean something."""
import json
import os

import numpy as np
import pytest

from tests import odd_width_cases as W
from tests.f16_oracle import launch_flip_fraction
from tests.helpers import oracle_launch
from yolo_v3_tf2_amd import _lib, quant
from yolo_v3_tf2_amd.graph import ConvOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yolov3_heuristic_tiles.json")
F32, BF16, X3, X2, F16, I8 = (_lib.Y3_DTYPE_F32, _lib.Y3_DTYPE_BF16, _lib.Y3_DTYPE_F32X3, _lib.Y3_DTYPE_F32X2, _lib.Y3_DTYPE_F16,
                              _lib.Y3_DTYPE_I8)
COUTS = (1, 18, 32, 33, 64, 96, 100, 128, 160, 192, 255, 256, 258, 288, 384, 512, 1024)
ROWS = ((1, 1), (64, 64), (588, 588), (5000, 200000), (200000, 200000))


def _generic_tiles(dtype):
    """{tile id: (bn, bk)} of the mode's built generic tiles (not the weight-resident kernel), and the padding of Cout in the mode."""
    if dtype == F32:
        return {t: (r[1], 32) for t, r in enumerate(_lib.TILES) if r[0] > 0 and t != 33}, 32
    if dtype in (BF16, F16):
        return {t: (r[1], r[3]) for t, r in enumerate(_lib.TILES_BF16) if r[0] > 0 and t != 32}, 32
    if dtype == I8:
        return {t: (_lib.TILES_BF16[t][1], 128) for t in _lib.TILES_I8_BUILT}, 64
    built = _lib.TILES_X3_BUILT if dtype == X3 else _lib.TILES_X2_BUILT
    return {t: (_lib.TILES_X3[t][1], _lib.TILES_X3[t][3]) for t in built}, 64


def _fits(bn, bk, cin, c0, cout_pad):
    """y3::tile_fits: the K step divides Cin and the concat boundary, the tile's width divides the padded Cout."""
    return cin % bk == 0 and cout_pad % bn == 0 and (c0 < 0 or c0 % bk == 0)


def _resident_allowed(dtype, size, stride, cin, c0, cout, arena_out):
    """resident_rule_f32 / resident_rule_bf16 with conv_res_*_fits: 3x3 / stride 1, one source, Cin 32 (16-bit: or 64), Cout % 64 == 0;
    the 16-bit kernel stores its own format only."""
    shape = size == 3 and stride == 1 and c0 < 0 and cout % 64 == 0
    if dtype == F32:
        return 33 if shape and cin == 32 else None
    if dtype in (BF16, F16):
        return 32 if shape and cin in (32, 64) and arena_out else None
    return None


def _shapes(dtype):
    step = 128 if dtype == I8 else 32       # int8: only what lies behind the cut
    for cin in range(step, 1025, step):
        yield 3, 1, cin, -1
        yield 3, 2, cin, -1
        yield 1, 1, cin, -1
        for c0 in range(step, cin, step):
            yield 1, 1, cin, c0


@pytest.mark.parametrize("dtype", [F32, BF16, X3, X2, F16, I8], ids=lambda d: _lib.DTYPE_TAGS[d])
def test_chooser_names_a_fitting_built_tile_or_none(dtype):
    lib = _lib.load()
    tiles, pad = _generic_tiles(dtype)
    assert all(lib.y3_tile_built(dtype, t) for t in tiles)
    resident_id = {F32: 33, BF16: 32, F16: 32}.get(dtype)
    bad, seen, refused, unfit_while_one_fits, n = [], set(), 0, 0, 0
    for size, stride, cin, c0 in _shapes(dtype):
        for cout in COUTS:
            cp = (cout + pad - 1) // pad * pad
            generic = {t for t, (bn, bk) in tiles.items() if _fits(bn, bk, cin, c0, cp)}
            for arena_out in (0, 1):
                res = _resident_allowed(dtype, size, stride, cin, c0, cout, arena_out)
                fitting = generic | ({res} if res is not None else set())
                for M, M_plan in ROWS:
                    t = lib.y3_choose_tile(dtype, size, stride, cin, c0, cout, M, M_plan, arena_out)
                    n += 1
                    refused += t == -1
                    ok = (t in fitting) if fitting else (t == -1)
                    if t == resident_id and res is None:
                        ok = False
                    if t >= 0:
                        seen.add(t)
                    if not ok:
                        bad.append(f"{size}x{size}/{stride} cin {cin} c0 {c0} cout {cout} M {M}/{M_plan} arena_out {arena_out}: "
                                   f"tile {t}, fitting {sorted(fitting)}")
                        unfit_while_one_fits += bool(fitting)
            if dtype in (F32, X3, X2):
                assert generic, (size, stride, cin, c0, cout)       # the fp32-accurate modes run every accepted width
    print(f"{_lib.DTYPE_TAGS[dtype]}: {n} shapes asked, {refused} without a tile, {len(bad)} wrong "
          f"({unfit_while_one_fits} while a built tile fits, {len(bad) - unfit_while_one_fits} where none does); tiles named: {sorted(seen)}")
    assert all(lib.y3_tile_built(dtype, t) for t in seen), sorted(seen)
    assert not bad, f"{len(bad)} wrong, e.g. " + " | ".join(bad[:: max(1, len(bad) // 6)][:6])
    if dtype in (F32, X3, X2):
        assert refused == 0


def test_chooser_refuses_what_net_create_refuses():
    lib = _lib.load()
    assert lib.y3_choose_tile(BF16, 1, 1, 256, 160, 384, 588, 588, 1) in (5, 6)        # [up(160), 96] -> 384
    assert lib.y3_choose_tile(BF16, 1, 1, 192, 96, 255, 588, 588, 0) in (5, 6)         # [96, 96] -> 255
    for dtype in (BF16, F16):
        assert lib.y3_choose_tile(dtype, 3, 1, 96, -1, 96, 588, 588, 1) == -1
        assert lib.y3_choose_tile(dtype, 1, 1, 32, -1, 32, 588, 588, 1) == -1
        assert lib.y3_choose_tile(dtype, 1, 1, 192, 96, 96, 588, 588, 1) == -1
    for args in ((99, 1, 1, 64, -1, 64, 1, 1, 1), (F32, 2, 1, 64, -1, 64, 1, 1, 1), (F32, 1, 2, 64, -1, 64, 1, 1, 1), (F32, 1, 1, 48, -1, 64, 1, 1, 1),
                 (F32, 1, 1, 64, 16, 64, 1, 1, 1), (F32, 3, 1, 64, 32, 64, 1, 1, 1), (F32, 1, 1, 64, 64, 64, 1, 1, 1), (F32, 1, 1, 64, -1, 0, 1, 1, 1),
                 (F32, 1, 1, 64, -1, 64, 0, 1, 1)):
        assert lib.y3_choose_tile(*args) == -2, args


def network_queries(program, batch, size=416):
    """(size, stride, cin, c0, cout, M, M_plan, arena_out) of every conv of the program that launches a tile, planned and called at
    `batch` images of size x size; arena_out: not one of the three heads (none of YOLOv3's is staged)."""
    out = []
    for o in program.conv_ops():
        if o.cin == 3:
            continue
        M = batch * (size // o.out_div) ** 2
        out.append((o.size, o.stride, o.cin, o.c0 if o.src1 >= 0 else -1, o.cout, M, M, int(o.dst not in program.outputs)))
    return out


def test_the_networks_own_tiles_are_unchanged(program):
    """The 74 tile-launching convs of YOLOv3 at 64 x 416^2 and 1 x 416^2 in every mode: the id the chooser gave before it learnt to
    say -1 (recorded from that chooser through y3_choose_tile).  int8: the convs the cut's shape rule admits."""
    lib = _lib.load()
    with open(GOLDEN) as f:
        golden = json.load(f)
    for dtype in (F32, BF16, X3, X2, F16, I8):
        for batch in (64, 1):
            qs = [q for q in network_queries(program, batch) if dtype != I8 or (q[2] % 128 == 0 and (q[3] < 0 or q[3] % 128 == 0))]
            got = [lib.y3_choose_tile(dtype, *q) for q in qs]
            want = golden[_lib.DTYPE_TAGS[dtype]][str(batch)]
            assert len(got) == len(want) and min(got) >= 0
            assert got == want, (_lib.DTYPE_TAGS[dtype], batch, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])


# ---------------------------------------------------------------------------------------------- what the GPU file relies on
def test_program_lowers_to_the_launches_the_gpu_file_is_about():
    p, ops = W.odd_width_program()
    assert all(isinstance(o, ConvOp) for o in p.ops) and [o for o in p.ops] == [ops[k] for k in W.NAMES]
    sig = {k: (o.size, o.stride, o.cin, o.c0 if o.src1 >= 0 else -1, o.cout) for k, o in ops.items()}
    assert sig == dict(a=(3, 1, 96, -1, 192), b=(1, 1, 192, -1, 96), c=(3, 1, 96, -1, 192), d=(3, 2, 192, -1, 160), e=(1, 1, 192, -1, 96),
                       h0=(1, 1, 192, 96, 255), f=(1, 1, 256, 160, 384), g=(3, 1, 384, -1, 384), h1=(3, 2, 384, -1, 96), h2=(1, 1, 384, -1, 160))
    assert ops["c"].residual == ops["a"].dst and not ops["c"].leaky and ops["f"].src0_upsample and not ops["h0"].src0_upsample
    assert (ops["h0"].src0, ops["h0"].src1, ops["f"].src0, ops["f"].src1) == (ops["e"].dst, ops["b"].dst, ops["d"].dst, ops["e"].dst)
    assert p.outputs == [ops[k].dst for k in ("h0", "h1", "h2")] and all(quant.writes_f32(p, ops[k]) for k in ("h0", "h1", "h2"))
    assert quant.first_i8_conv(p) == W.NAMES.index("g")
    assert max(o.size * o.size * o.cin for o in p.conv_ops()) == 3456          # inside f32_conv_bar's K <= 4608
    # tile counts in N that are no power of two: 3 and 6 (a, c: 192; g: 384), 3 (b, e: 96), 5 (d: 160)
    assert {k: -(-o.cout // 32) for k, o in ops.items() if k in ("b", "d", "e")} == dict(b=3, d=5, e=3)


def test_unrunnable_programs_hold_one_conv_no_16bit_tile_divides():
    lib = _lib.load()
    for name, (p, slot, (cin, c0, cout)) in W.unrunnable_programs().items():
        convs = p.conv_ops()
        for s, o in enumerate(convs):
            if o.cin == 3:
                continue
            shape = (o.size, o.stride, o.cin, o.c0 if o.src1 >= 0 else -1, o.cout)
            t = lib.y3_choose_tile(BF16, *shape, 432, 432, int(o.dst not in p.outputs))
            assert (t == -1) == (s == slot), (name, s, shape, t)
            assert all(lib.y3_choose_tile(d, *shape, 432, 432, int(o.dst not in p.outputs)) >= 0 for d in (F32, X3, X2)), (name, s)
        assert (convs[slot].cin, convs[slot].c0 if convs[slot].src1 >= 0 else -1, convs[slot].cout) == (cin, c0, cout)


def test_detect_program_takes_the_composed_route():
    p = W.detect_program()
    heads = [o for o in p.conv_ops() if o.dst in p.outputs]
    assert [o.cin for o in heads] == [96, 160, 96] and all(o.cout == 255 and o.cin % 64 for o in heads)
    assert [p.tensors[t].div for t in p.outputs] == [16, 8, 4]
    lib = _lib.load()
    for o in p.conv_ops()[1:]:
        shape = (o.size, o.stride, o.cin, -1, o.cout)
        assert all(lib.y3_choose_tile(d, *shape, 48, 48, int(o.dst not in p.outputs)) >= 0 for d in (F32, BF16, F16)), shape


@pytest.mark.parametrize("canvas", W.CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_reference_alone_flips_at_most_half_the_cap(fmt, canvas):
    """The GPU file lets at most 2e-3 (bf16) / 1e-2 (fp16) of a stored launch's elements differ from the rounded double-accumulating
    oracle.  That says something about the kernel only while another fp32 summation order alone stays well inside it: per stored launch
    of the program, from the same oracle-made 16-bit input tensors, the rounded fp32-accumulating launch against the rounded
    double-accumulating one -- at most half the cap (tests/test_tile_matrix_host.py, tests/test_f16_host.py)."""
    from oracle import oracle as O
    from tests.f16_oracle import forward_f16, round_f16
    p, ops = W.odd_width_program()
    w, x = W.inputs(p, canvas)
    keep = set(range(len(p.tensors)))
    if fmt == "bf16":
        _, kept = O.forward(p, w, x, bf16=True, keep=keep)
        kept[p.input_tensor] = O.round_bf16(x)
        cap = W.BF16_DIFFER_CAP
    else:
        _, kept = forward_f16(p, w, x, keep=keep)
        kept[p.input_tensor] = round_f16(x)
        cap = W.F16_DIFFER_CAP
    worst = 0.0
    for name in W.STORED:
        if fmt == "bf16":
            y32 = O.round_bf16(oracle_launch(O, ops[name], w, kept.__getitem__, acc64=False, bf16_weights=True))
            y64 = O.round_bf16(oracle_launch(O, ops[name], w, kept.__getitem__, acc64=True, bf16_weights=True))
            frac = float((y32 != y64).mean())
        else:
            frac, y32 = launch_flip_fraction(ops[name], w, kept.__getitem__)
        assert np.array_equal(y32, kept[ops[name].dst]), name                   # the restated launch IS the walker's layer
        print(f"odd widths {fmt} {canvas[0]}x{canvas[1]} conv {name}: reference-alone flip fraction {frac:.2e} (cap {cap:.0e})")
        worst = max(worst, frac)
        assert frac <= cap / 2, (name, frac)
    print(f"odd widths {fmt} {canvas[0]}x{canvas[1]}: worst reference-alone flip fraction {worst:.2e}")
