"""Per-tile conv matrix for fp16 plans (Y3_DTYPE_F16): tests/test_tile_matrix_gpu.py's every-tile test for the fp16 instantiations of the
16-bit conv kernel (csrc/conv_16bit.h through csrc/conv_f16.hip).  Every built generic tile id of the bf16 family (fp16 plans share the ids
and y3_net_set_tile_bf16) forced on tests/helpers.tile_feature_program, on a square and a non-square canvas, each launch held to the
double-accumulating oracle on the launch's OWN device inputs with fp16-rounded weights.  Bars: the project's per-layer ones with fp16 in
place of bf16 --

  an fp32 head fed fp16 inputs:  |got - ref| <= 2e-5 * max(1, |ref|max)  (K <= 2304 here);
  a stored fp16 output:  every element within f16_ulp_elem + 1e-5 |ref|max of round_f16(ref), at most 1e-2 of a launch's elements
  different at all (tests/test_f16_host.py: the reference alone, summed in fp32 instead of double, stays under 5e-3: fp16's 11
  significand bits put 8 times as many fp32 sums near a rounding boundary as bf16's 8 do).

The weight-resident tile 32 has its own test (tests/test_f16_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16  # noqa: E402
from tests.helpers import TILE_MATRIX_BATCH, TILE_MATRIX_CANVASES, oracle_launch, tile_feature_program, tile_matrix_inputs  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

TILES = [t for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32]
MUST_FORCE = ("a", "c", "f", "h0", "h1", "h2")
DIFFER_CAP = 1e-2


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


@pytest.mark.parametrize("canvas", TILE_MATRIX_CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("tile", TILES, ids=[f"f16-t{t}" for t in TILES])
def test_every_tile_every_launch_form_teacher_forced_f16(rt, tile, canvas):
    from oracle import oracle as O
    bn, bk = _lib.TILES_BF16[tile][1], _lib.TILES_BF16[tile][3]
    p, ops = tile_feature_program(bn, bk)
    w, x = tile_matrix_inputs(p, canvas)
    x = round_f16(x)
    B = TILE_MATRIX_BATCH
    net = rt.Net(p)
    net.load_weights(w)
    forced = []
    for slot, o in enumerate(net.conv_ops):
        try:
            net.set_tile_bf16(slot, tile)
        except rt.Y3Error as e:
            if "tile does not" not in str(e):
                raise
            continue
        forced.append(o)
    missed = [k for k in MUST_FORCE if not any(o is ops[k] for o in forced)]
    assert not missed, f"tile {tile} was refused on conv(s) {missed}: the matrix would not run them"
    net.keep_activations(True)
    net.plan(B, canvas, _lib.Y3_DTYPE_F16)
    xin = torch.from_numpy(x).cuda().to(torch.float16)      # x is fp16-exact already
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
        with f16_emulation():
            ref = oracle_launch(O, o, w, dev.__getitem__, acc64=True, bf16_weights=True)     # the weights rounded to fp16
        got = dev[o.dst]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if o.dst not in p.outputs:
            assert np.array_equal(round_f16(got), got), name                                  # what is stored is fp16
            exp = round_f16(ref)
            diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
            bar = f16_ulp_elem(got, exp) + 1e-5 * float(np.abs(exp).max())
            frac = float((diff > 0).mean())
            print(f"tile-matrix f16 tile {tile} {canvas[0]}x{canvas[1]} conv {name}: worst {float((diff / bar).max()):.3f} of the bar, "
                  f"{frac:.2e} of the elements differ")
            assert (diff <= bar).all(), (name, float((diff / bar).max()))
            assert frac <= DIFFER_CAP, (name, frac)
            worst, worst_frac = max(worst, float((diff / bar).max())), max(worst_frac, frac)
        else:
            err, bar = float(np.abs(got - ref).max()), 2e-5 * max(1.0, float(np.abs(ref).max()))
            print(f"tile-matrix f16 tile {tile} {canvas[0]}x{canvas[1]} conv {name}: worst {err / bar:.3f} of the bar")
            assert err <= bar, (name, err, bar)
            worst = max(worst, err / bar)
    line = (f"tile-matrix f16 tile {tile} {canvas[0]}x{canvas[1]}: forced {len(forced)} convs, worst {worst:.3f} of the bar, "
            f"worst differing fraction {worst_frac:.2e} (cap {DIFFER_CAP:.0e})")
    print(line)
