"""The int8 edge cases of tests/i8_edge_cases.py on the host: each case must do what it is for, asserted from the NumPy restatement
(yolo_v3_tf2_amd/quant.py) alone.  tests/test_i8_edges_gpu.py then holds the device to the restatement on the same cases, bit for bit.
The shares are conditions on the cases, not measurements of the device; each test prints what it found."""
import numpy as np
import pytest

import yolo_v3_tf2_amd  # noqa: F401
from tests import i8_edge_cases as E
from yolo_v3_tf2_amd import quant

F32 = np.float32


def _parts_checked(case, ref, t):
    """epilogue_parts of the conv writing t, after holding it to quant.conv_i8's own answer."""
    acc, v, tt = E.parts(case, ref, t)
    if tt is None:
        assert ref[t].dtype == F32 and np.array_equal(v, ref[t])
    else:
        assert ref[t].dtype == np.int8 and np.array_equal(np.clip(np.rint(tt), -127.0, 127.0).astype(np.int8), ref[t])
    return acc, v, tt


@pytest.mark.parametrize("name", list(E.BUILDERS))
def test_every_case_is_int8_from_conv_0_and_within_the_size_limits(name):
    case, xq, ref = E.get(name)
    p = case.program
    assert quant.first_i8_conv(p) == 0 and p.tensors[p.input_tensor].channels in (128, 256)
    assert case.B <= 3 and max(case.canvas) <= 24
    assert np.array_equal(case.x, E.round_f16(case.x)) and np.isfinite(case.x).all()
    for o in p.conv_ops():
        f32 = quant.writes_f32(p, o)
        assert f32 == (o.dst in p.outputs)
        assert f32 or case.scales[o.dst] > 0
        if o.src1 >= 0:
            assert case.scales[o.src0] == case.scales[o.src1]
    for t in list(case.stored.values()) + list(case.heads.values()):
        _parts_checked(case, ref, t)
    assert all(np.isfinite(ref[t]).all() for t in p.outputs)


def test_ties_case_rounds_exact_halves_everywhere():
    case, xq, ref = E.get("ties")
    p = case.program
    xt = case.x * (F32(1.0) / F32(case.scales[p.input_tensor]))
    share = E.is_half(xt).mean()
    print(f"ties: input values on an exact half {share:.1%}")
    assert share >= 0.40
    assert np.array_equal(xq, quant.quantize(case.x, case.scales[p.input_tensor]))
    assert (E.round_half_away(xt) != xq).mean() >= 0.10
    for role, t in case.stored.items():
        o = case.op(t)
        assert not o.bn and o.src0 == p.input_tensor and o.residual == (p.input_tensor if role in "bd" else -1)
        assert (o.size, o.leaky) == dict(a=(1, False), b=(3, False), c=(1, True), d=(3, True))[role]
        acc, v, tt = _parts_checked(case, ref, t)
        if not o.leaky:      # the construction is exact: t is a multiple of 1/2 (0.1f v on the negative side of a leaky conv is not)
            assert (np.rint(tt * 2) == tt * 2).all()
        half = (E.is_half(tt) & (np.abs(tt) < 127)).mean()
        away = (E.round_half_away(tt) != ref[t]).mean()
        print(f"ties: conv {role} ({o.size}x{o.size}{' leaky' if o.leaky else ' linear'}{' + input' if o.residual >= 0 else ''}): "
              f"unsaturated outputs on an exact half {half:.1%}, bytes a round-half-away epilogue changes {away:.1%}")
        assert half >= (0.15 if o.leaky else 0.30)
        assert away >= 0.10


def test_saturation_case_clamps_on_both_sides():
    case, xq, ref = E.get("saturation")
    p = case.program
    hi, lo = (xq == 127).mean(), (xq == -127).mean()
    print(f"saturation: input +127 {hi:.1%}, -127 {lo:.1%}")
    assert hi >= 0.10 and lo >= 0.10 and (xq == -128).sum() == 0
    forms = dict(a=(False, False), b=(False, True), c=(True, True), d=(True, False))      # role -> (leaky, shortcut)
    for role, t in case.stored.items():
        o = case.op(t)
        assert o.bn and (o.leaky, o.residual >= 0) == forms[role]
        acc, v, tt = _parts_checked(case, ref, t)
        hi, lo = (ref[t] == 127).mean(), (ref[t] == -127).mean()
        beyond = (np.abs(tt) > 127.5).mean()
        print(f"saturation: conv {role} ({'leaky' if o.leaky else 'linear'}{' + shortcut' if o.residual >= 0 else ''}): "
              f"+127 {hi:.1%}, -127 {lo:.1%}, beyond the clamp {beyond:.1%}")
        assert hi >= 0.10 and hi + lo <= 0.60
        assert lo >= 0.10 or role == "d"          # leaky alone cannot reach -127
        assert beyond >= 0.9 * (hi + lo) - 0.02   # the bytes at +-127 are clamped values, not values that round to +-127
        assert (tt > 129).any() and (role == "d" or (tt < -129).any())      # values a wrap through & 0xff would turn round


def _truncated_f32(acc):
    """int64 -> fp32 rounded toward zero."""
    f = acc.astype(F32)
    over = np.abs(f.astype(np.float64)) > np.abs(acc)
    return np.where(over, np.nextafter(f, F32(0.0)), f).astype(F32)


def test_wide_case_accumulators_are_not_fp32_numbers():
    case, xq, ref = E.get("wide")
    p = case.program
    assert xq.min() >= 118 and xq.max() == 127
    for role, t in list(case.stored.items()) + list(case.heads.items()):
        o = case.op(t)
        assert (o.size, o.cin, o.size * o.size * o.cin) == (3, 256, 2304)
        wq, _ = quant.quantize_weights(case.weights[f"conv{o.conv_index}.w"])
        assert np.abs(wq.astype(np.int32)).min() >= 100
        sign = np.sign(wq.astype(np.int32)).reshape(-1, o.cout)
        assert (sign == sign[0]).all() and (sign[0, 0::2] == 1).all() and (sign[0, 1::2] == -1).all()
        acc, v, tt = _parts_checked(case, ref, t)
        inexact = (acc.astype(F32).astype(np.int64) != acc).mean()
        print(f"wide: conv {role}: max |acc| {np.abs(acc).max():.3e}, accumulators that are no fp32 number {inexact:.1%}")
        assert np.abs(acc).max() > 2 ** 24 and inexact >= 0.30
    h = case.heads["h"]
    o = case.op(h)
    assert o.cout == 255 and quant.writes_f32(p, o)
    acc, v, _ = E.parts(case, ref, h)
    _, sw = quant.quantize_weights(case.weights[f"conv{o.conv_index}.w"])
    sc = (F32(case.scales[p.input_tensor]) * sw).astype(F32)
    assert np.array_equal((acc.astype(F32) * sc).astype(F32) + quant.bn_fold(o, case.weights)[1], v)
    changed = (((_truncated_f32(acc) * sc).astype(F32) + quant.bn_fold(o, case.weights)[1]) != v).mean()
    print(f"wide: fp32 head outputs a truncating (float)acc changes {changed:.1%}")
    assert changed >= 0.10
    a = ref[case.stored["a"]]
    assert 0.02 < (np.abs(a.astype(np.int32)) == 127).mean() < 0.5 and len(np.unique(a)) > 40      # the stored conv does not all saturate


def test_weights_case_channels_quantise_as_the_scheme_says():
    case, xq, ref = E.get("weights")
    names = E.WEIGHT_CHANNELS
    for t, bn in ((case.stored["a"], True), (case.stored["b"], True), (case.heads["h"], False)):
        o = case.op(t)
        W = case.weights[f"conv{o.conv_index}.w"]
        q, s = quant.quantize_weights(W)
        q = q.astype(np.int32).reshape(-1, o.cout)      # [K, Cout], k as the packed rows count it
        flat = W.reshape(-1, o.cout)
        K = flat.shape[0]
        c = names.index("zero")
        assert s[c] == 1.0 and not q[:, c].any()
        if not bn:
            assert o.cout == 255 and s[254] == 1.0 and not q[:, 254].any() and not flat[:, 254].any()
        c = names.index("last_k_only")
        assert np.flatnonzero(q[:, c]).tolist() == [K - 1] and q[K - 1, c] == 127
        c = names.index("negative_absmax")
        assert q[:, c].min() == -127 and q[:, c].max() < 127 and s[c] == -flat[:, c].min() / F32(127.0)
        c = names.index("ties")
        assert s[c] == F32(2.0 ** -6)
        exact = flat[:, c] / s[c]
        halves = E.is_half(exact)
        assert halves.sum() == K - 1 and (q[halves, c] % 2 == 0).all() and np.array_equal(q[halves, c], np.rint(exact[halves]))
        assert (E.round_half_away(exact[halves]) != q[halves, c]).mean() > 0.4      # half of them round the other way under half-away
        c = names.index("absmax_1e-30")
        assert F32(7e-33) < s[c] < F32(9e-33) and np.abs(q[:, c]).max() == 127 and len(np.unique(q[:, c])) > 50
        c = names.index("absmax_1e4")
        assert F32(78.0) < s[c] < F32(79.0) and np.abs(q[:, c]).max() == 127
        assert s[names.index("absmax_1e4")] / s[names.index("absmax_1e-30")] > 1e33
        c = names.index("all_plus_mx")
        assert (q[:, c] == 127).all() and s[c] == F32(2.0 ** -6)
        if bn:
            scale, shift = quant.bn_fold(o, case.weights)
            g0, gn = names.index("gamma_zero"), names.index("gamma_negative")
            assert scale[g0] == 0 and scale[gn] < 0 and (np.delete(scale, [g0, gn]) > 0).all()
            acc, v, tt = _parts_checked(case, ref, t)
            assert np.abs(acc[..., g0]).max() > 1000 and len(np.unique(v[..., g0])) == 1      # the shift alone, whatever the conv sums
            assert len(np.unique(ref[t][..., gn])) > 20
        else:
            acc, v, tt = _parts_checked(case, ref, t)
            bias = case.weights[f"conv{o.conv_index}.bias"]
            assert (v[..., 0] == bias[0]).all() and (v[..., 254] == bias[254]).all()
        live = [names.index(n) for n in ("last_k_only", "negative_absmax", "ties", "absmax_1e-30", "absmax_1e4", "all_plus_mx")][:6 if bn else 3]
        out = ref[t]
        assert all(len(np.unique(out[..., c])) > 3 for c in live), [len(np.unique(out[..., c])) for c in live]


def test_call_order_case_changes_every_stored_byte_pattern():
    """The three states of the call-order test differ from each other, so a device that kept an earlier state would be seen."""
    case, scales_b, second = E.call_order_case()
    p = case.program

    def run(w, s):
        xq = quant.quantize(case.x, s[p.input_tensor])
        return xq, quant.forward_i8(p, w, s, {p.input_tensor: xq}, 0)

    xa, ra = run(case.weights, case.scales)
    xb, rb = run(case.weights, scales_b)
    xc, rc = run(second, scales_b)
    assert (xa != xb).mean() > 0.3
    for t in list(case.stored.values()) + list(p.outputs):
        assert (ra[t] != rb[t]).mean() > 0.3 and (rb[t] != rc[t]).mean() > 0.3, t
    # stale epilogue scales with new weights (sc = s_in * s_w * bn_scale not uploaded again) would differ as well
    a = case.stored["a"]
    o = case.op(a)
    _, sw1 = quant.quantize_weights(case.weights[f"conv{o.conv_index}.w"])
    _, sw2 = quant.quantize_weights(second[f"conv{o.conv_index}.w"])
    assert (sw1 != sw2).mean() > 0.9
