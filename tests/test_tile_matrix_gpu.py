"""Per-tile conv matrix: every built generic tile id of every plan mode, forced on a program (tests/helpers.tile_feature_program) whose
convs take every launch form the tile's templates are instantiated for -- one and two sources (the first up-sampled or not), output stored
in the plan's format and fp32 head output, shortcut, linear and leaky epilogues, Cout short of the padded width, stride 2 -- on a square and
a non-square canvas, each launch held to the oracle on the launch's OWN device inputs (teacher-forced), with double accumulation on the
reference side.  Bars are the project's per-layer ones (tests/test_gpu_parity.py):

  fp32, f32x3, f32x2 and every fp32 head of a bf16 plan:  |got - ref| <= 2e-5 * max(1, |ref|max) per launch (K <= 2304 here);
  bf16 stored outputs:  every element within its own bf16 ulp (+ 1e-5 |ref|max) of the rounded reference, at most 2e-3 of a launch's
  elements different at all (tests/test_tile_matrix_host.py: the reference alone, summed in fp32 instead of double, stays under 1e-3).

The weight-resident kernels (fp32 tile 33, bf16 tile 32), split-K and the chunk-major K order have their own tests.
Also here: a graph whose add / upsample / concat do NOT fold into conv launches (the stand-alone kernels of csrc/elementwise.hip)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import (TILE_MATRIX_BATCH, TILE_MATRIX_CANVASES, oracle_launch, tile_feature_program,  # noqa: E402
                           tile_matrix_inputs, unfolded_program)
from yolo_v3_tf2_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_ulp_elem(a, b):
    """Per element: the spacing of bf16 numbers (8 significand bits) in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


# mode -> (plan dtype, tile table, the tile ids of the mode's existing every-tile test, setter, column of the table that holds BK or None)
MODES = {
    "f32": (_lib.Y3_DTYPE_F32, _lib.TILES, [t for t in range(len(_lib.TILES)) if t not in _lib.RETIRED_TILES and t != 33], "set_tile", None),
    "bf16": (_lib.Y3_DTYPE_BF16, _lib.TILES_BF16, [t for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32], "set_tile_bf16", 3),
    "f32x3": (_lib.Y3_DTYPE_F32X3, _lib.TILES_X3, list(_lib.TILES_X3_BUILT), "set_tile_x3", 3),
    "f32x2": (_lib.Y3_DTYPE_F32X2, _lib.TILES_X3, list(_lib.TILES_X2_BUILT), "set_tile_x2", 3),
}
CASES = [(mode, t) for mode, spec in MODES.items() for t in spec[2]]
MUST_FORCE = ("a", "c", "f", "h0", "h1", "h2")


def _feed(rt, mode, x):
    """The fp32 input in the form a plan of `mode` takes for an input that feeds an MFMA conv directly."""
    if mode == "bf16":
        return _cuda(x).to(torch.bfloat16)      # x is bf16-exact already
    if mode == "f32x3":
        return rt.split3_planes(_cuda(x))
    if mode == "f32x2":
        return rt.split2_planes(_cuda(x))
    return _cuda(x)


def _force_everywhere(rt, net, setter, tile):
    """The tile on every conv it fits; -> the convs that took it.  Only the setter's misfit refusal is a 'does not fit'."""
    forced = []
    for slot, o in enumerate(net.conv_ops):
        try:
            getattr(net, setter)(slot, tile)
        except rt.Y3Error as e:
            if "tile does not" not in str(e):
                raise
            continue
        forced.append(o)
    return forced


@pytest.mark.parametrize("canvas", TILE_MATRIX_CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("mode,tile", CASES, ids=[f"{m}-t{t}" for m, t in CASES])
def test_every_tile_every_launch_form_teacher_forced(rt, mode, tile, canvas):
    from oracle import oracle as O
    dtype, table, _, setter, bk_col = MODES[mode]
    bn, bk = table[tile][1], (table[tile][bk_col] if bk_col is not None else 32)
    p, ops = tile_feature_program(bn, bk)
    w, x = tile_matrix_inputs(p, canvas)
    if mode == "bf16":
        x = O.round_bf16(x)
    B = TILE_MATRIX_BATCH
    net = rt.Net(p)
    net.load_weights(w)
    forced = _force_everywhere(rt, net, setter, tile)
    missed = [k for k in MUST_FORCE if not any(o is ops[k] for o in forced)]
    assert not missed, f"tile {tile} was refused on conv(s) {missed}: the matrix would not run them"
    net.keep_activations(True)
    net.plan(B, canvas, dtype)
    xin = _feed(rt, mode, x)
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    first = [g.clone() for g in net.forward(xin)] + [net.read_tensor(t, B).clone() for t in stored]
    grids = net.forward(xin)
    again = list(grids) + [net.read_tensor(t, B) for t in stored]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two forwards of one plan differ"
    dev = {t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(p.outputs, grids)}
    dev.update({t: g.cpu().numpy() for t, g in zip(stored, again[3:])})
    dev[p.input_tensor] = x

    worst, worst_frac = 0.0, 0.0
    for o in p.conv_ops():
        name = next(k for k, v in ops.items() if v is o)
        ref = oracle_launch(O, o, w, dev.__getitem__, acc64=True, bf16_weights=(mode == "bf16"))
        got = dev[o.dst]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if mode == "bf16" and o.dst not in p.outputs:
            exp = O.round_bf16(ref)
            diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
            bar = _bf16_ulp_elem(got, exp) + 1e-5 * float(np.abs(exp).max())
            frac = float((diff > 0).mean())
            print(f"tile-matrix {mode} tile {tile} {canvas[0]}x{canvas[1]} conv {name}: worst {float((diff / bar).max()):.3f} of the bar, "
                  f"{frac:.2e} of the elements differ")
            assert (diff <= bar).all(), (name, float((diff / bar).max()))
            assert frac <= 2e-3, (name, frac)
            worst, worst_frac = max(worst, float((diff / bar).max())), max(worst_frac, frac)
        else:
            err, bar = float(np.abs(got - ref).max()), 2e-5 * max(1.0, float(np.abs(ref).max()))
            print(f"tile-matrix {mode} tile {tile} {canvas[0]}x{canvas[1]} conv {name}: worst {err / bar:.3f} of the bar")
            assert err <= bar, (name, err, bar)
            worst = max(worst, err / bar)
    print(f"tile-matrix {mode} tile {tile} {canvas[0]}x{canvas[1]} summary: forced {len(forced)} convs, worst {worst:.3f} of the bar, "
          f"worst bf16 mismatch fraction {worst_frac:.2e}")


@pytest.mark.parametrize("mode", list(MODES))
def test_forced_tile_that_does_not_fit_is_refused(rt, mode):
    """A 128-wide tile on the 64-filter helper conv b of the bn = 64 program: refused by the setter, by name."""
    _, table, tiles, setter, _ = MODES[mode]
    wide = next(t for t in tiles if table[t][1] == 128)
    p, ops = tile_feature_program(64, 32)
    net = rt.Net(p)
    slot = next(s for s, o in enumerate(net.conv_ops) if o is ops["b"])
    with pytest.raises(rt.Y3Error, match="tile does not"):
        getattr(net, setter)(slot, wide)
    getattr(net, setter)(next(s for s, o in enumerate(net.conv_ops) if o is ops["a"]), next(t for t in tiles if table[t][1] == 64))


# ---------------------------------------------------------------------------------------------- un-folded graphs
UNFOLDED_B, UNFOLDED_S = 2, 12


def _unfolded_inputs():
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p, aux = unfolded_program()
    x = np.random.default_rng(12).standard_normal((UNFOLDED_B, UNFOLDED_S, UNFOLDED_S, 64)).astype(np.float32)
    return p, aux, synthetic_weights(p, seed=12), x


def test_standalone_add_upsample_concat_match_oracle(rt):
    """The stand-alone add / upsample2x / concat kernels: the three outputs behind them against the oracle's walk at the fp32 layer bar,
    and each aux tensor bit-equal to the oracle's layer applied to the device's own operands (two pure copies and one fp32 add)."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.graph import AuxOp
    p, aux, w, x = _unfolded_inputs()
    B = UNFOLDED_B
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    net.plan(B, UNFOLDED_S)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        g = g.cpu().numpy().reshape(r.shape)
        assert np.abs(g - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max())), float(np.abs(g - r).max())
    layer = {"add": O.add, "upsample": O.upsample2x, "concat": O.concat}
    seen = []
    for o in p.ops:
        if not isinstance(o, AuxOp):
            continue
        operands = [net.read_tensor(t, B).cpu().numpy() for t in o.inputs]
        exp = layer[o.kind](*operands)
        g = net.read_tensor(o.dst, B).cpu().numpy()
        assert g.shape == exp.shape and np.array_equal(g.view(np.uint32), exp.view(np.uint32)), o.kind
        assert np.abs(exp).max() > 0.1      # not a comparison of two empty buffers
        seen.append(o.kind)
    assert seen == ["add", "upsample", "concat"] and sorted(aux) == sorted(seen)


@pytest.mark.parametrize("mode", ["bf16", "f32x3", "f32x2"])
def test_standalone_aux_ops_are_refused_outside_fp32(rt, mode):
    p, _, w, x = _unfolded_inputs()
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(UNFOLDED_B, UNFOLDED_S, MODES[mode][0])
    with pytest.raises(rt.Y3Error, match="stand-alone add/upsample/concat ops are fp32 only"):
        net.forward(_feed(rt, mode, x))
    torch.cuda.synchronize()
