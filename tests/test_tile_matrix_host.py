"""Host side of the per-tile conv matrix (tests/test_tile_matrix_gpu.py), no GPU: the lowering pattern the matrix relies on, and the
condition under which its cap on differing bf16 elements means something -- the reference alone must stay well inside it."""
import numpy as np
import pytest

from tests.helpers import (TILE_MATRIX_CANVASES, oracle_launch, tile_feature_program, tile_matrix_inputs, unfolded_program)
from yolo_v3_tf2_amd import _lib
from yolo_v3_tf2_amd.graph import AuxOp, ConvOp

STORED = ("a", "b", "c", "d", "e", "f")       # written in the plan's format; a, c and f are the ones every tile is forced on


def _geometries():
    """(bn, bk) of every tile the matrix forces, per mode (fp32: K step 32, last table column is the LDS stage count)."""
    f32 = {(row[1], 32) for t, row in enumerate(_lib.TILES) if row[0] > 0 and t != 33}
    bf16 = {(row[1], row[3]) for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32}
    x = {(_lib.TILES_X3[t][1], _lib.TILES_X3[t][3]) for t in set(_lib.TILES_X3_BUILT) | set(_lib.TILES_X2_BUILT)}
    return {"f32": sorted(f32), "bf16": sorted(bf16), "x": sorted(x)}


GEOMETRIES = _geometries()


@pytest.mark.parametrize("bn,bk", sorted({g for gs in GEOMETRIES.values() for g in gs}))
def test_feature_program_lowers_to_the_launch_forms_the_matrix_is_about(bn, bk):
    p, ops = tile_feature_program(bn, bk)
    assert all(isinstance(o, ConvOp) for o in p.ops) and len(p.ops) == 9          # no AuxOp left over
    wd = ops["a"].cout
    assert wd % bn == 0 and wd % bk == 0 and (wd == bn or bn % bk)
    a, b, c, d, e, f, h0, h1, h2 = (ops[k] for k in ("a", "b", "c", "d", "e", "f", "h0", "h1", "h2"))
    assert (a.size, a.stride, a.cin, a.leaky, a.residual, a.src1) == (3, 1, 64, True, -1, -1)
    # c: the shortcut folded into the launch, written to the add's tensor, no activation
    assert (c.size, c.cin, c.cout, c.leaky, c.bn) == (3, 64, wd, False, True) and c.residual == a.dst and c.src0 == b.dst
    assert p.tensors[c.dst].producer.endswith(".add")
    # f: two sources, the first read through the up-sampling
    assert (f.size, f.cin, f.c0, f.cout, f.src0_upsample, f.src0, f.src1) == (1, 128, 64, wd, True, d.dst, e.dst)
    assert (d.size, d.stride, d.src0, e.size, e.src0) == (3, 2, c.dst, 1, c.dst)
    # h0: two sources at one resolution, one filter short of a padded width the tile divides
    assert (h0.size, h0.cin, h0.c0, h0.src0_upsample, h0.src0, h0.src1, h0.bn, h0.leaky) == (1, 128, 64, False, e.dst, b.dst, False, False)
    assert h0.cout == (255 if bn >= 128 else bn - 1) and (h0.cout + 1) % bn == 0
    assert (h1.size, h1.stride, h1.cin, h1.cout, h1.src0, h1.leaky) == (3, 2, wd, bn, f.dst, True)
    assert (h2.size, h2.cin, h2.cout, h2.src0, h2.leaky, h2.bn) == (1, wd, bn, f.dst, False, True)
    assert p.outputs == [h0.dst, h1.dst, h2.dst]
    # only the three heads are plan outputs, none of them read again or behind a shortcut: the rest is stored in the plan's format
    reads = {t for o in p.ops for t in (o.src0, o.src1, o.residual)}
    assert not reads & set(p.outputs) and all(o.residual < 0 for o in (h0, h1, h2))
    # every channel count a forced tile has to divide
    for o in (a, c, f, h0, h1, h2):
        assert o.cin % bk == 0 and (o.src1 < 0 or o.c0 % bk == 0)


def test_unfolded_program_keeps_its_three_aux_ops():
    p, aux = unfolded_program()
    kinds = [(o.kind, o.dst) for o in p.ops if isinstance(o, AuxOp)]
    assert kinds == [("add", aux["add"]), ("upsample", aux["upsample"]), ("concat", aux["concat"])]
    convs = p.conv_ops()
    assert len(convs) == 7 and all(o.src1 < 0 and o.residual < 0 and not o.src0_upsample for o in convs)
    by_src = {}
    for o in convs:
        by_src.setdefault(o.src0, []).append(o)
    assert sorted(o.size for o in by_src[aux["upsample"]]) == [1, 3]              # read by a 3x3 conv and by a head
    (cat,) = by_src[aux["concat"]]
    assert (cat.size, cat.cin, cat.dst) == (3, 96, p.outputs[2])
    assert [o.dst for o in by_src[aux["add"]]] != [] and len(p.outputs) == 3


@pytest.mark.parametrize("canvas", TILE_MATRIX_CANVASES)
@pytest.mark.parametrize("bn,bk", GEOMETRIES["bf16"])
def test_reference_alone_flips_at_most_half_the_bf16_cap(bn, bk, canvas):
    """The GPU matrix lets at most 2e-3 of a bf16 launch's elements differ from the rounded double-accumulating oracle.  That cap says
    something about the kernel only while a DIFFERENT fp32 summation order alone stays well inside it: per stored launch of the
    program, from the same (oracle-made, bf16) input tensors, round_bf16 of the fp32-accumulating oracle against round_bf16 of the
    double-accumulating one -- at most 1e-3 of the elements differ, half the cap."""
    from oracle import oracle as O
    p, ops = tile_feature_program(bn, bk)
    w, x = tile_matrix_inputs(p, canvas)
    _, kept = O.forward(p, w, x, bf16=True, keep=set(range(len(p.tensors))))
    kept[p.input_tensor] = O.round_bf16(x)
    worst = 0.0
    for name in STORED:
        y32 = O.round_bf16(oracle_launch(O, ops[name], w, kept.__getitem__, acc64=False, bf16_weights=True))
        y64 = O.round_bf16(oracle_launch(O, ops[name], w, kept.__getitem__, acc64=True, bf16_weights=True))
        assert np.array_equal(y32, kept[ops[name].dst])                            # the restated launch IS the walker's layer
        frac = float((y32 != y64).mean())
        worst = max(worst, frac)
        assert frac <= 1e-3, (name, frac)
    print(f"bn {bn} bk {bk} canvas {canvas}: worst reference-alone flip fraction {worst:.2e}")
