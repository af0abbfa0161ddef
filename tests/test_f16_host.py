"""fp16 plans (Y3_DTYPE_F16), host side, no GPU: the tile ids the mode shares with bf16, the fp16-emulating oracle of the GPU tests
(tests/f16_oracle.py) -- that it leaves no trace, how far it is from itself under another summation order (the floor of the free-running GPU
test) and from fp32 -- and the condition under which the GPU tests' caps on differing elements mean something: the reference alone, summed
in fp32 instead of double, stays within half of them."""
import numpy as np
import pytest

from tests.f16_oracle import (f16_emulation, f16_ulp_elem, forward_f16, free_running_floor, launch_flip_fraction, rel_l2, round_f16)
from tests.helpers import TILE_MATRIX_CANVASES, tile_feature_program, tile_matrix_inputs
from yolo_v3_tf2_amd import _lib

REAL_CAP = 6e-3       # half of the GPU teacher-forced cap on the real network (1.2e-2)
MATRIX_CAP = 5e-3     # half of the GPU per-tile matrix cap (1e-2)


def test_f16_dtype_and_tile_ids():
    """The first thing an fp16 plan needs: the dtype value, its tag, and the bf16 family's tile table under it."""
    assert _lib.Y3_DTYPE_F16 == 4 and _lib.DTYPE_TAGS[_lib.Y3_DTYPE_F16] == "f16"
    built = [t for t in range(len(_lib.TILES_BF16)) if _lib.tile_built(_lib.Y3_DTYPE_F16, t)]
    for t in range(len(_lib.TILES_BF16)):
        assert _lib.tile_built(_lib.Y3_DTYPE_F16, t) == _lib.tile_built(_lib.Y3_DTYPE_BF16, t), t
    assert built and built == [t for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0]
    assert not _lib.tile_built(_lib.Y3_DTYPE_F16, len(_lib.TILES_BF16)) and not _lib.tile_built(5, 0)


def test_round_f16_and_ulp():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, -1e6, 2.0 ** -24, 2.0 ** -26, 3 * 2.0 ** -25], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, np.inf, -np.inf, 2.0 ** -24, 0.0, 2.0 ** -23], np.float32)
    assert np.array_equal(round_f16(x), want)                                   # ties to even, IEEE overflow, subnormals kept
    assert np.array_equal(f16_ulp_elem(np.array([1.0, 1.5, 2.0, 48.5, 1e-9], np.float32), np.zeros(5, np.float32)),
                          [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -5, 2.0 ** -24])


def test_helper_leaves_no_trace(program, weights):
    from oracle import oracle as O
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    original = O.round_bf16
    p = mini_program(64, [], [dict(filters=64, size=3), dict(filters=64, size=1), dict(filters=32, size=1)])
    w = synthetic_weights(p, seed=1)
    x = np.random.default_rng(1).standard_normal((1, 8, 8, 64)).astype(np.float32)
    before = O.forward(p, w, x, bf16=True)
    f16 = forward_f16(p, w, x)
    assert O.round_bf16 is original
    with pytest.raises(ZeroDivisionError):
        with f16_emulation():
            assert O.round_bf16 is round_f16
            1 / 0
    assert O.round_bf16 is original
    after = O.forward(p, w, x, bf16=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))             # bf16 numbers again
    assert any(not np.array_equal(a, b) for a, b in zip(before, f16))           # and the substitute did act
    y = np.float32(1.0 + 2.0 ** -9)
    assert O.round_bf16(np.array([y]))[0] == 1.0 and round_f16(np.array([y]))[0] == y


@pytest.fixture(scope="module")
def real(program, weights):
    """The real network at 2 x 96^2, input seed 1234: the four oracle walks, with every conv launch's output kept from the fp16 walk."""
    x = np.random.default_rng(1234).random((2, 96, 96, 3), dtype=np.float32)
    keep = {o.dst for o in program.conv_ops()}
    return x, free_running_floor(program, weights, x, keep=keep)


def test_f16_free_running_floor(program, real):
    """The fp16-emulating oracle against itself with double accumulation: the floor of the free-running GPU comparison, and how much
    closer to fp32 than bf16 the format is."""
    _, r = real
    print("fp16 oracle vs itself (acc64): rel", ["%.2e" % v for v in r["floor_rel"]], "max", ["%.2e" % v for v in r["floor_max"]])
    for k in range(3):
        assert 2e-4 < r["floor_rel"][k] < 2e-3, (k, r["floor_rel"][k])
        d16, dbf = rel_l2(r["f16"][k], r["f32"][k]), rel_l2(r["bf16"][k], r["f32"][k])
        print(f"head {k}: fp16 oracle vs fp32 oracle rel {d16:.2e} max {np.abs(r['f16'][k] - r['f32'][k]).max():.2e}; "
              f"bf16 oracle rel {dbf:.2e} max {np.abs(r['bf16'][k] - r['f32'][k]).max():.2e}; gain {dbf / d16:.1f} x")
        assert dbf >= 4.0 * d16, (k, d16, dbf)
    stored = [o.dst for o in program.conv_ops() if o.dst not in program.outputs]
    assert len(stored) == 72
    for t in stored:
        v = r["kept"][t]
        assert np.isfinite(v).all() and np.array_equal(round_f16(v), v), t
    assert all(np.isfinite(g).all() for g in r["f16"])


def test_real_network_reference_alone_flips_at_most_half_the_cap(program, weights, real):
    """Every stored launch of the real network from the fp16 walk's own tensors: fp32 against double accumulation, rounded to fp16."""
    x, r = real
    kept = dict(r["kept"])
    kept[program.input_tensor] = x
    fracs = {}
    for o in program.conv_ops():
        if o.dst in program.outputs:
            continue
        frac, y32 = launch_flip_fraction(o, weights, kept.__getitem__)
        assert np.array_equal(y32, r["kept"][o.dst]), o.conv_index               # the restated launch IS the walker's layer
        fracs[o.conv_index] = frac
    worst = max(fracs, key=fracs.get)
    print(f"real network, reference alone: worst flip fraction {fracs[worst]:.2e} at conv {worst}, median {np.median(list(fracs.values())):.2e}")
    assert fracs[worst] <= REAL_CAP, (worst, fracs[worst])


def _bf16_geometries():
    return sorted({(row[1], row[3]) for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32})


@pytest.mark.parametrize("canvas", TILE_MATRIX_CANVASES)
@pytest.mark.parametrize("bn,bk", _bf16_geometries())
def test_tile_program_reference_alone_flips_at_most_half_the_cap(bn, bk, canvas):
    """The form of test_reference_alone_flips_at_most_half_the_bf16_cap with fp16 roundings: launches a .. f of the per-tile program."""
    p, ops = tile_feature_program(bn, bk)
    w, x = tile_matrix_inputs(p, canvas)
    _, kept = forward_f16(p, w, x, keep=set(range(len(p.tensors))))
    kept[p.input_tensor] = round_f16(x)
    worst = 0.0
    for name in ("a", "b", "c", "d", "e", "f"):
        frac, y32 = launch_flip_fraction(ops[name], w, kept.__getitem__)
        assert np.array_equal(y32, kept[ops[name].dst]), name
        worst = max(worst, frac)
        assert frac <= MATRIX_CAP, (name, frac)
    print(f"bn {bn} bk {bk} canvas {canvas}: worst reference-alone fp16 flip fraction {worst:.2e}")
