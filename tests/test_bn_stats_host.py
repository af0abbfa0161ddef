"""Host side of the trained-like batch-norm suite (tests/bn_stat_cases.py, tests/test_bn_stats_gpu.py), no GPU: the recipe really has
the statistics it claims on every program the GPU tier runs, and every bar the GPU tier applies means something -- the reference ALONE
stays well inside it.

Measured here (worst over all cases): the oracle summing in fp32 against the oracle summing in double reaches 0.16 of the per-channel
fp32 bar (the network's K = 4608 convs; 0.16 on the K = 2304 convs of the tile programs), 0.15 with the BN scale folded into the
weights first (the fp32 plans' arithmetic), both under the quarter the bar's use requires, so no launch needs a bar of its own; the
share of 16-bit roundings that flip between the two summations reaches 7.3e-4 (bf16, cap 2e-3) and 4.0e-3 (fp16, cap 1e-2), both on the
network."""
import numpy as np
import pytest

from tests import bn_stat_cases as C
from tests.f16_oracle import round_f16

CASES = C.all_cases()
TAGS = list(CASES) + ["network"]
MODE_CASES = [(t, m) for t in CASES for m in CASES[t][1]] + [("network", m) for m in ("f32", "bf16", "f16")]


def _case(tag, program):
    make, modes = (C.all_cases(program) if tag == "network" else CASES)[tag]
    return make() + (modes,)


# ---------------------------------------------------------------------------------------------- the recipe
@pytest.mark.parametrize("tag", TAGS)
def test_recipe_has_the_statistics_it_claims(tag, program):
    from oracle import oracle as O
    p, w, x, _ = _case(tag, program)
    scales = []
    for o in p.conv_ops():
        i = o.conv_index
        if not o.bn:
            assert tag.startswith("stem-identity") or float(np.abs(w[f"conv{i}.bias"]).max()) > 1.0      # biases of order 1
            continue
        assert o.cout % 16 == 0
        gamma, var = w[f"conv{i}.gamma"], w[f"conv{i}.var"]
        c = np.arange(o.cout) % 16
        # every class channel in every group of 16, and nowhere else
        assert np.array_equal(gamma == 0, c == C.CLASS_GAMMA_ZERO) and np.array_equal(var == 0, c == C.CLASS_VAR_ZERO)
        tiny = np.abs(gamma) == np.float32(C.TINY_GAMMA)
        assert tiny[c == C.CLASS_GAMMA_TINY].all() or (tag.startswith("stem") and i == 0) or (tag.startswith("range") and i == 0)
        assert (gamma < 0).any() and (gamma > 0).any()
        scale, shift = C.fold(O, o, w)
        scales.append(np.abs(scale))
        assert float(np.abs(shift).max()) > 1.0                                                          # shifts of order 1
        raw, scaled = C.scaled_weights(O, o, w)
        K = raw.shape[0]
        live = scaled != 0
        lo_raw, lo_scaled = float((np.abs(raw) < 2.0 ** -14).mean()), float((np.abs(scaled[live]) < 2.0 ** -13).mean())
        if K >= 128:
            assert lo_raw > 0 and lo_scaled > 0, (i, K, lo_raw, lo_scaled)
    if scales:
        s = np.concatenate(scales)
        print(f"{tag}: |scale| spans {s[s > 0].min():.1e} .. {s.max():.1e}")
        assert s[s > 0].min() <= 1e-3 and s.max() >= 3e1
    for mode in ("f32", "f16"):
        kept = C.oracle_tensors(p, w, x, mode)
        top = max(float(np.abs(v).max()) for v in kept.values())
        assert np.isfinite(top) and top < 1000.0, (mode, top)
    print(f"{tag}: |output|max {top:.1f}")


def test_stem_cases_carry_the_channels_the_normalisation_is_for():
    for S, B in C.STEM_SIZES:
        for kind in ("block", "identity"):
            _, w, _ = C.stem_case(kind, S, B)
            w0 = w["conv0.w"]
            assert 0 < float(np.abs(w0[..., C.STEM_TINY_CHANNEL]).max()) < 2.0 ** -14           # all of the channel's raw weights: fp16 subnormals
            assert w["conv0.gamma"][3] == 0 and w["conv0.gamma"][19] == 0 and w["conv0.gamma"][C.STEM_TINY_CHANNEL] != 0
            others = np.delete(np.abs(w0).reshape(27, 32).max(axis=0), C.STEM_TINY_CHANNEL)
            assert (others > 2.0 ** -14).all()


def test_calibrated_statistics_are_the_measured_ones(program):
    """The network's BN mean / var ARE the per-channel mean / variance of the conv's pre-BN output on the calibration images (var = 0
    class: exactly 0, the weights rescaled until the variance is the BN epsilon), so the normalised output has unit variance."""
    from oracle import oracle as O
    w, x = C.network_case(program)
    kept = C.oracle_tensors(program, w, x)
    for o in program.conv_ops()[:12]:
        if o.src1 >= 0 or not o.bn:
            continue
        acc = O.conv2d(kept[o.src0], w[f"conv{o.conv_index}.w"], o.stride).reshape(-1, o.cout).astype(np.float64)
        var, zero = w[f"conv{o.conv_index}.var"], np.arange(o.cout) % 16 == C.CLASS_VAR_ZERO
        assert np.allclose(acc.mean(axis=0), w[f"conv{o.conv_index}.mean"], rtol=1e-4, atol=1e-6 * float(np.abs(acc).max()))
        assert np.allclose(acc.var(axis=0)[~zero], var[~zero], rtol=1e-3)
        assert np.allclose(acc.var(axis=0)[zero], C.BN_EPS, rtol=1e-3) and not var[zero].any()


# ---------------------------------------------------------------------------------------------- the reference alone against the bars
def _folded_launch(O, op, weights, tensor):
    """The launch as an fp32 plan computes it: the BN scale folded into the weights in fp32, fp32 sums, then shift, leaky, residual."""
    i = op.conv_index
    scale, shift = C.fold(O, op, weights)
    x = tensor(op.src0)
    if op.src0_upsample:
        x = O.upsample2x(x)
    if op.src1 >= 0:
        x = O.concat(x, tensor(op.src1))
    y = O.conv2d(x, (weights[f"conv{i}.w"] * scale).astype(np.float32), op.stride) + shift
    if op.leaky:
        y = np.where(y >= 0, y, np.float32(0.1) * y).astype(np.float32)
    return O.add(tensor(op.residual), y) if op.residual >= 0 else y


@pytest.mark.parametrize("tag,mode", MODE_CASES)
def test_reference_alone_stays_within_its_share_of_the_bars(tag, mode, program):
    """Per launch, from the oracle's own tensors: fp32 sums against double sums at or under a quarter of the per-channel fp32 bar (also with
    the scale folded into the weights first), and at most half of the 16-bit caps of roundings flipped."""
    from oracle import oracle as O
    p, w, x, _ = _case(tag, program)
    kept = C.oracle_tensors(p, w, x, mode)
    worst, worst_folded, worst_flip = 0.0, 0.0, 0.0
    with C.mode_oracle(mode):
        for o in p.conv_ops():
            r32 = C.launch_reference(O, o, w, kept.__getitem__, mode, acc64=False)
            r64 = C.launch_reference(O, o, w, kept.__getitem__, mode, acc64=True)
            m = C.channel_magnitude(O, o, C.mode_weights(w, o, mode), kept.__getitem__)
            assert (m > 0).all()
            if mode != "f32" and o.dst not in p.outputs:
                rnd = round_f16 if mode == "f16" else O.round_bf16
                flip = float((rnd(r32) != rnd(r64)).mean())
                worst_flip = max(worst_flip, flip)
                assert flip <= C.DIFFER_CAP[mode] / 2, (o.conv_index, flip)
                continue
            bar = C.F32_CHANNEL_BAR_OVERRIDES.get((tag, o.conv_index), C.F32_CHANNEL_BAR)
            share = float((np.abs(r32.astype(np.float64) - r64).reshape(-1, o.cout).max(axis=0) / (bar * m)).max())
            worst = max(worst, share)
            assert share <= 0.25, (o.conv_index, o.size * o.size * o.cin, share)
            if mode == "f32":
                f = _folded_launch(O, o, w, kept.__getitem__)
                share = float((np.abs(f.astype(np.float64) - r64).reshape(-1, o.cout).max(axis=0) / (bar * m)).max())
                worst_folded = max(worst_folded, share)
                assert share <= 0.25, (o.conv_index, o.size * o.size * o.cin, "folded", share)
    print(f"{tag} {mode}: reference alone at most {worst:.3f} of the per-channel fp32 bar ({worst_folded:.3f} with the scale folded), "
          f"flips at most {worst_flip:.2e} of a stored launch")


@pytest.mark.parametrize("S,B", C.STEM_SIZES)
def test_fused_fp32_stem_floor(S, B):
    """The fp32 fused stem runs conv0, conv1 and the 1x1 free of the oracle: the oracle's own walk with fp32 sums against the walk with
    double sums, at the program's outputs, stays under a quarter of the per-channel bar."""
    from oracle import oracle as O
    p, w, x = C.stem_case("block", S, B)
    a, b = O.forward(p, w, x), O.forward(p, w, x, acc64=True)
    kept = C.oracle_tensors(p, w, x)
    by_dst = {o.dst: o for o in p.conv_ops()}
    for t, ya, yb in zip(p.outputs, a, b):
        m = C.channel_magnitude(O, by_dst[t], w, kept.__getitem__)
        share = float((np.abs(ya.astype(np.float64) - yb).reshape(-1, m.size).max(axis=0) / (C.F32_CHANNEL_BAR * m)).max())
        print(f"stem block {S} x{B} output {t}: free-running reference alone {share:.3f} of the bar")
        assert share <= 0.25


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("S,B", C.STEM_SIZES)
def test_fused_16bit_stem_caps_hold_for_the_reference_alone(S, B, fmt):
    r = C.stem_references(S, B, fmt)
    pairs = [("oracle, double vs fp32 sums", r["oracle64"], r["oracle"])]
    if fmt == "f16":
        pairs += [("restated vs oracle", r["restated"], r["oracle"]), ("restated vs oracle with double sums", r["restated"], r["oracle64"])]
    for what, a, b in pairs:
        frac, beyond, worst = C.stem_compare(a, b, r["m"], fmt)
        print(f"stem identity {S} x{B} {fmt}, {what}: {frac:.3e} differ, {beyond:.3e} beyond their own ulp, worst {worst:.3f} of the bar")
        assert frac <= C.STEM_DIFFER_CAP[fmt] / 2 and beyond <= C.STEM_BEYOND_CAP[fmt] / 2 and worst <= 1.0, (what, frac, beyond, worst)


# ---------------------------------------------------------------------------------------------- the weight formats of y3_net.cpp
def _bn_convs(program):
    for tag, (make, _) in C.all_cases(program).items():
        if tag.startswith(("tile", "network")):
            p, w, _ = make()
            for o in p.conv_ops():
                if o.bn and o.cin != 3:
                    yield tag, o, w


def _rms(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).mean(axis=0))


def test_two_plane_split_of_the_scaled_weights_keeps_2_pow_minus_22_per_channel(program):
    """The two-plane weights of y3_net_set_conv_weights restated (csrc/y3_net.cpp: normalise_rows, split_f16x2): the BN-scaled weights of
    an output channel divided by the power of two that brings the channel's largest into [1, 2), then h + l' / 2048.  Per element within
    2^-22 |w| where l' is a normal number (|w| > 2^-13 of the normalised channel) and within 2^-36 below; per output channel the rms
    representation error within 2^-22 of the channel's rms weight, subnormal h and l' kept.  The normalisation is exact and is what makes
    this hold: split as they are, the channels of a small gamma over a large variance (rms |w scale| = |gamma| / sqrt(K), 2e-5 for
    |gamma| = 2^-10 and K = 2304) have every l' subnormal and miss 2^-22 (3.0e-7 measured).  Were fp16 subnormal operands flushed in
    the kernel, the normalised planes would lose 1.5e-5 of a channel's rms weight, the un-normalised ones 0.9 of it."""
    from oracle import oracle as O
    worst, worst_plain, worst_flushed, worst_plain_flushed = 0.0, 0.0, 0.0, 0.0
    for tag, o, w in _bn_convs(program):
        scale, _ = C.fold(O, o, w)
        ws = (w[f"conv{o.conv_index}.w"].reshape(-1, o.cout) * scale).astype(np.float32)
        live = np.abs(ws).max(axis=0) > 0
        assert float(np.abs(ws).max()) < 65504.0
        wn, e = C.normalise_rows(ws)
        assert np.array_equal(np.ldexp(wn, e[None, :]).astype(np.float32), ws)                     # exact
        mx = np.abs(wn).max(axis=0)
        assert (mx[live] >= 1.0).all() and (mx[live] < 2.0).all() and not e[~live].any()
        h, lo = C.split_f16x2(wn)
        assert np.array_equal(round_f16(h), h) and np.array_equal(round_f16(lo), lo)
        err = np.abs(h.astype(np.float64) + lo.astype(np.float64) / 2048.0 - wn)
        big = np.abs(wn) > 2.0 ** -13
        assert (err[big] <= 2.0 ** -22 * np.abs(wn[big])).all() and (err[~big] <= 2.0 ** -36).all(), (tag, o.conv_index)
        share = _rms(err)[live] / _rms(wn)[live]
        flushed = C.flush_f16_subnormals(h).astype(np.float64) + C.flush_f16_subnormals(lo).astype(np.float64) / 2048.0
        worst, worst_flushed = max(worst, float(share.max())), max(worst_flushed, float((_rms(flushed - wn)[live] / _rms(wn)[live]).max()))
        assert share.max() <= 2.0 ** -22, (tag, o.conv_index, float(share.max()))
        h, lo = C.split_f16x2(ws)                                                                    # ... and without the normalisation
        plain = h.astype(np.float64) + lo.astype(np.float64) / 2048.0
        flushed = C.flush_f16_subnormals(h).astype(np.float64) + C.flush_f16_subnormals(lo).astype(np.float64) / 2048.0
        worst_plain = max(worst_plain, float((_rms(plain - ws)[live] / _rms(ws)[live]).max()))
        worst_plain_flushed = max(worst_plain_flushed, float((_rms(flushed - ws)[live] / _rms(ws)[live]).max()))
    print(f"two-plane split: worst per-channel rms error {worst:.2e} of the rms weight ({worst_flushed:.2e} with subnormals flushed); "
          f"without the normalisation {worst_plain:.2e} ({worst_plain_flushed:.2e} flushed)")
    assert worst_plain > 2.0 ** -22 and worst_plain_flushed > 0.1       # the recipe does reach the range the normalisation is for


def test_fp16_rounded_raw_weights_keep_2_pow_minus_11_per_channel(program):
    """f32_to_f16_rne (csrc/y3_net.cpp) restated: the raw weights of an fp16 plan, rounded with subnormals kept -- per element within
    2^-11 |w| or 2^-25, per output channel an rms error within 2^-11 of the channel's rms weight; flushed subnormals would cost a channel
    1e-2 of it and more."""
    worst, worst_flushed = 0.0, 0.0
    for tag, o, w in _bn_convs(program):
        raw = w[f"conv{o.conv_index}.w"].reshape(-1, o.cout)
        live = np.abs(raw).max(axis=0) > 0
        r16 = round_f16(raw)
        assert np.isfinite(r16).all()
        err = np.abs(r16.astype(np.float64) - raw)
        assert (err <= np.maximum(2.0 ** -11 * np.abs(raw), 2.0 ** -25)).all(), (tag, o.conv_index)
        share = _rms(err)[live] / _rms(raw)[live]
        flushed = _rms(C.flush_f16_subnormals(r16).astype(np.float64) - raw)[live] / _rms(raw)[live]
        worst, worst_flushed = max(worst, float(share.max())), max(worst_flushed, float(flushed.max()))
        assert share.max() <= 2.0 ** -11, (tag, o.conv_index, float(share.max()))
    print(f"fp16 raw weights: worst per-channel rms error {worst:.2e} of the rms weight, {worst_flushed:.2e} with subnormals flushed")
    assert worst_flushed > 2.0 ** -11


# ---------------------------------------------------------------------------------------------- the bars see what they are for
def _leaky(v):
    return np.where(v >= 0, v, np.float32(0.1) * v).astype(np.float32)


def _mutants(O, op, w, tensor):
    """Two wrong epilogues of one launch, restated on the host: the shift of channel n ^ 16, leaky before the shift."""
    scale, shift = C.fold(O, op, w)
    acc = O.conv2d(tensor(op.src0), w[f"conv{op.conv_index}.w"], op.stride, acc64=True)
    return {"shift of n ^ 16": _leaky(acc * scale + shift[np.arange(op.cout) ^ 16]), "leaky before the shift": _leaky(acc * scale) + shift}


def test_per_channel_bar_catches_what_the_whole_tensor_bar_lets_through():
    """The three reversions the suite is meant to notice, emulated on one launch (conv a of the 64-wide tile program).  A wrong shift
    index and a wrong epilogue order fail the per-channel fp32 bar.  fp16 subnormals zeroed in pack_planes are seen through the fp16 plans'
    raw weights (a channel 186 times over its stored-element bar); through the two-plane weights they are NOT seen any more: normalised
    per channel, the planes lose 0.12 of the bar to a flush (all of a small channel's weights before the normalisation), and a channel
    that wrong still sat inside the old whole-tensor bar."""
    from oracle import oracle as O
    from tests.helpers import f32_conv_bar
    p, ops, w, x = C.tile_case(64)
    op, tensor = ops["a"], {p.input_tensor: x}.__getitem__
    i = op.conv_index
    ref = C.launch_reference(O, op, w, tensor, "f32")
    m = C.channel_magnitude(O, op, w, tensor)
    assert C.check_per_channel(ref, ref, m, "the reference itself")[0] == 0.0
    for what, bad in _mutants(O, op, w, tensor).items():
        with pytest.raises(AssertionError):
            C.check_per_channel(bad, ref, m, what)
    # pack_planes<1>, an fp16 plan: the raw weights rounded to fp16 with the subnormals zeroed, the output stored in fp16
    scale, shift = C.fold(O, op, w)
    x16 = round_f16(x)
    t16 = {p.input_tensor: x16}.__getitem__
    with C.mode_oracle("f16"):
        ref16 = C.launch_reference(O, op, w, t16, "f16")
        m16 = C.channel_magnitude(O, op, C.mode_weights(w, op, "f16"), t16)
    flushed = C.flush_f16_subnormals(round_f16(w[f"conv{i}.w"]))
    with pytest.raises(AssertionError):
        C.check_per_channel(round_f16(_leaky(O.conv2d(x16, flushed, op.stride, acc64=True) * scale + shift)), ref16, m16, "fp16 weights flushed", stored="f16")
    # pack_planes<2>, the two-plane mode: the BN-scaled weights, with and without the per-channel normalisation, planes flushed
    ws = (w[f"conv{i}.w"].reshape(-1, op.cout) * scale).astype(np.float32)
    shares = {}
    for what, (wn, e) in (("normalised", C.normalise_rows(ws)), ("as they are", (ws, np.zeros(op.cout, np.int32)))):
        h, lo = C.split_f16x2(wn)
        planes = C.flush_f16_subnormals(h).astype(np.float64) + C.flush_f16_subnormals(lo).astype(np.float64) / 2048.0
        wf = np.ldexp(planes, e[None, :]).astype(np.float32).reshape(w[f"conv{i}.w"].shape)
        err = np.abs(_leaky(O.conv2d(x, wf, op.stride, acc64=True) + shift).astype(np.float64) - ref).reshape(-1, op.cout).max(axis=0)
        shares[what] = err / (C.F32_CHANNEL_BAR * m)
        if what == "as they are":
            quiet = int(((err > C.F32_CHANNEL_BAR * m) & (err <= f32_conv_bar(ref))).sum())
    print(f"two-plane weights with their subnormals flushed: worst channel {shares['normalised'].max():.3f} of the per-channel bar normalised, "
          f"{shares['as they are'].max():.1f} as they are ({quiet} channels over their own bar and inside the whole-tensor bar)")
    assert shares["normalised"].max() <= 0.25 and shares["as they are"].max() > 1.0 and quiet > 0
