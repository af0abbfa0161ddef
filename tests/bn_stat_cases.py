"""What tests/test_bn_stats_host.py and tests/test_bn_stats_gpu.py share: conv weights with the batch-norm statistics of a TRAINED
checkpoint, and bars that judge a launch channel by channel.

weights.synthetic_weights gives every channel of every layer a folded BN scale of 1 +- 15 % and a shift of about 0.07, so a scale or
shift read at the wrong channel, an epilogue applied in the wrong order, or a weight lost to the 16-bit formats' subnormal range all
pass the suites built on it.  The recipes here (variances N(0, v) are written with the VARIANCE as second argument throughout):

  trained_like_weights(program, seed) -- per output channel c of a BN conv with K = k * k * Cin:
      var    log-uniform in [1e-4, 1e2];  |gamma| log-uniform in [2^-6, 4], random sign;
      class channels, period 16 so that every 16- and 32-wide fragment column group of every tile holds each of them:
          c % 16 == 3: gamma = 0 (pruned);  c % 16 == 5: var = 0;  c % 16 == 7: |gamma| = 2^-10;
      w ~ N(0, (var_c + 1e-3) / K)  (the pre-BN output of a unit-variance input has the variance the statistics claim);
      beta ~ N(0, 1);  mean ~ N(0, 1) * sqrt(var_c + 1e-3).
    Bias convs: w ~ N(0, 1 / K), bias ~ N(0, 3).
  calibrated_weights(program, seed, images) -- for whole networks: the same gamma, beta and class channels, raw weights N(0, 1 / K)
    times 2^U(-8, 2) per output channel, and mean / var of every BN conv SET TO the measured per-channel mean and variance of that
    conv's pre-BN output in one fp32 oracle pass over `images`, as training would leave them (the uncalibrated recipe multiplies the
    activation variance by about 2.4 per layer: fine for nine convs, not for 75).  The var = 0 class keeps var exactly 0: its
    channels' weights are rescaled so that the measured variance is the BN epsilon, i.e. the normalised output still has unit variance.

The bars (check_per_channel), with m_c = |scale_c| max|acc_c| + |shift_c| (+ max|residual_c|) the magnitude the launch handles in
channel c (channel_magnitude; acc the double-accumulating conv of the launch's own inputs, scale / shift from the oracle's bn_fold,
1 and the bias for a bias conv):

  an fp32 output of any launch (fp32, f32x3, f32x2 plans and the fp32 heads of 16-bit plans):
      max_c |got - ref|_c / m_c <= 2e-5                      -- F32_CHANNEL_BAR, the project's layer constant applied per channel;
  a stored bf16 / fp16 output:
      every element within its own ulp + 1e-5 m_c of the rounded reference, and at most 2e-3 (bf16) / 1e-2 (fp16) of a launch's
      elements different at all -- the caps of the tile matrices.

tests/test_bn_stats_host.py holds these bars to the reference alone: the oracle summed in fp32 against the oracle summed in double
stays at or under a quarter of the fp32 bar per channel, and flips at most half of each cap."""
import numpy as np

from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16
from tests.helpers import oracle_launch

BN_EPS = 1e-3
F32_CHANNEL_BAR = 2e-5
# A launch whose reference alone (fp32 against double summation) exceeds a quarter of F32_CHANNEL_BAR gets 4 x its measured floor
# instead: {(case tag of all_cases(), conv_index): bar}.  Measured by tests/test_bn_stats_host.py; empty: no launch needs it.
F32_CHANNEL_BAR_OVERRIDES = {}
DIFFER_CAP = {"bf16": 2e-3, "f16": 1e-2}
CLASS_GAMMA_ZERO, CLASS_VAR_ZERO, CLASS_GAMMA_TINY = 3, 5, 7       # c % 16
TINY_GAMMA = 2.0 ** -10


def _bn_classes(rng, cout):
    """-> (gamma, beta, var) of the recipe, class channels included."""
    var = 10.0 ** rng.uniform(-4.0, 2.0, cout)
    sign = rng.choice([-1.0, 1.0], cout)
    gamma = sign * 2.0 ** rng.uniform(-6.0, 2.0, cout)
    c = np.arange(cout) % 16
    gamma[c == CLASS_GAMMA_ZERO] = 0.0
    var[c == CLASS_VAR_ZERO] = 0.0
    gamma[c == CLASS_GAMMA_TINY] = sign[c == CLASS_GAMMA_TINY] * TINY_GAMMA
    beta = rng.standard_normal(cout)
    return gamma, beta, var


def trained_like_weights(program, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for n in program.conv_nodes:
        cin = program.tensors[n.inputs[0]].channels
        k, cout, i = n.size, n.filters, n.conv_index
        K = k * k * cin
        if n.bn:
            gamma, beta, var = _bn_classes(rng, cout)
            out[f"conv{i}.w"] = (rng.standard_normal((k, k, cin, cout)) * np.sqrt((var + BN_EPS) / K)).astype(np.float32)
            out[f"conv{i}.gamma"] = gamma.astype(np.float32)
            out[f"conv{i}.beta"] = beta.astype(np.float32)
            out[f"conv{i}.mean"] = (rng.standard_normal(cout) * np.sqrt(var + BN_EPS)).astype(np.float32)
            out[f"conv{i}.var"] = var.astype(np.float32)
        else:
            out[f"conv{i}.w"] = (rng.standard_normal((k, k, cin, cout)) / np.sqrt(K)).astype(np.float32)
            out[f"conv{i}.bias"] = (rng.standard_normal(cout) * np.sqrt(3.0)).astype(np.float32)
    return out


def calibrated_weights(program, seed, images):
    """See the module docstring.  One fp32 oracle pass over `images`, node by node (conv, BN + leaky, add, upsample, concat)."""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    out = {}
    vals = {program.input_tensor: np.ascontiguousarray(images, np.float32)}
    for n in program.nodes:
        if n.kind == "add":
            vals[n.output] = O.add(vals[n.inputs[0]], vals[n.inputs[1]])
        elif n.kind == "upsample":
            vals[n.output] = O.upsample2x(vals[n.inputs[0]])
        elif n.kind == "concat":
            vals[n.output] = O.concat(vals[n.inputs[0]], vals[n.inputs[1]])
        elif n.kind == "yolo":
            vals[n.output] = vals[n.inputs[0]]
        else:
            assert n.kind == "conv", n.kind
            x = vals[n.inputs[0]]
            k, cout, i = n.size, n.filters, n.conv_index
            K = k * k * x.shape[-1]
            w = rng.standard_normal((k, k, x.shape[-1], cout)) / np.sqrt(K)
            if not n.bn:
                out[f"conv{i}.w"] = w.astype(np.float32)
                out[f"conv{i}.bias"] = (rng.standard_normal(cout) * np.sqrt(3.0)).astype(np.float32)
            else:
                gamma, beta, var = _bn_classes(rng, cout)
                w = (w * 2.0 ** rng.uniform(-8.0, 2.0, cout)).astype(np.float32)
                acc = O.conv2d(x, w, n.stride).reshape(-1, cout).astype(np.float64)
                zero = var == 0.0
                if zero.any():      # var stays exactly 0: the weights are rescaled until the measured variance is the BN epsilon
                    f = np.where(zero, np.sqrt(BN_EPS) / np.maximum(acc.std(axis=0), 1e-30), 1.0)
                    w = (w * f).astype(np.float32)
                    acc = O.conv2d(x, w, n.stride).reshape(-1, cout).astype(np.float64)
                out[f"conv{i}.w"] = w
                out[f"conv{i}.gamma"], out[f"conv{i}.beta"] = gamma.astype(np.float32), beta.astype(np.float32)
                out[f"conv{i}.mean"] = acc.mean(axis=0).astype(np.float32)
                out[f"conv{i}.var"] = np.where(zero, 0.0, acc.var(axis=0)).astype(np.float32)
            vals[n.output] = O.conv_block(x, out, i, k, n.stride, n.bn, n.leaky)
    return out


# ---------------------------------------------------------------------------------------------- references per plan mode
def mode_weights(weights, op, mode):
    """The conv's weights as a plan of `mode` holds them: rounded to bf16 / fp16 for the MFMA convs of a 16-bit plan (the Cin = 3
    first layer stays fp32), untouched otherwise."""
    i = op.conv_index
    w = {k: v for k, v in weights.items() if k.startswith(f"conv{i}.")}
    if mode in ("bf16", "f16") and op.cin != 3:
        from oracle import oracle as O
        w[f"conv{i}.w"] = round_f16(w[f"conv{i}.w"]) if mode == "f16" else O.round_bf16(w[f"conv{i}.w"])
    return w


def launch_reference(O, op, weights, tensor, mode, acc64=True):
    """helpers.oracle_launch of a launch in a plan of `mode`, nothing rounded but the 16-bit plans' weights."""
    return oracle_launch(O, op, mode_weights(weights, op, mode), tensor, acc64=acc64)


def fold(O, op, weights):
    """(scale, shift) of the launch's epilogue: the oracle's bn_fold, or 1 and the bias."""
    i = op.conv_index
    if op.bn:
        return O.bn_fold(weights[f"conv{i}.gamma"], weights[f"conv{i}.beta"], weights[f"conv{i}.mean"], weights[f"conv{i}.var"])
    return np.ones(op.cout, np.float32), np.asarray(weights[f"conv{i}.bias"], np.float32)


def channel_magnitude(O, op, weights, tensor):
    """m[c] = |scale_c| max|acc_c| + |shift_c| (+ max|residual_c|): acc the double-accumulating conv of the launch's own inputs
    (tensor(id) -> fp32 NHWC), `weights` holding the conv's weights as the plan does (mode_weights)."""
    x = tensor(op.src0)
    if op.src0_upsample:
        x = O.upsample2x(x)
    if op.src1 >= 0:
        x = O.concat(x, tensor(op.src1))
    acc = O.conv2d(x, weights[f"conv{op.conv_index}.w"], op.stride, acc64=True)
    scale, shift = fold(O, op, weights)
    m = np.abs(scale).astype(np.float64) * np.abs(acc).reshape(-1, op.cout).max(axis=0) + np.abs(shift)
    if op.residual >= 0:
        m = m + np.abs(tensor(op.residual)).reshape(-1, op.cout).max(axis=0)
    return m


def bf16_ulp_elem(a, b):
    """Per element: the spacing of bf16 numbers (8 significand bits) in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


def check_per_channel(got, ref, m, what, stored=None, bar=F32_CHANNEL_BAR):
    """Hold one launch's output [..., C] to the per-channel bars of the module docstring.  stored: None (an fp32 output), "bf16" or
    "f16" (an output stored in that format; `ref` is the unrounded reference).  -> (worst share of the bar, differing fraction)."""
    C = m.shape[0]
    assert got.shape == ref.shape and got.shape[-1] == C, (what, got.shape, ref.shape, C)
    assert np.isfinite(got).all(), what
    m = np.asarray(m, np.float64)
    assert (m > 0).all(), (what, "a channel of magnitude 0")
    if stored is None:
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).reshape(-1, C).max(axis=0)
        share = err / (bar * m)
        c = int(share.argmax())
        assert share[c] <= 1.0, (what, f"channel {c}: |got - ref| = {err[c]:.3e} is {share[c]:.2f} of the bar {bar:.1e} x m_c = {m[c]:.3e}")
        return float(share[c]), 0.0
    rnd, ulp = {"f16": (round_f16, f16_ulp_elem), "bf16": (_round_bf16, bf16_ulp_elem)}[stored]
    assert np.array_equal(rnd(got), got), (what, f"what is stored is not {stored}")
    exp = rnd(ref)
    diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    share = (diff / (ulp(got, exp) + 1e-5 * m)).reshape(-1, C).max(axis=0)
    frac = float((diff > 0).mean())
    c = int(share.argmax())
    assert share[c] <= 1.0, (what, f"channel {c}: {share[c]:.2f} of (ulp + 1e-5 x m_c = {m[c]:.3e})")
    assert frac <= DIFFER_CAP[stored], (what, frac)
    return float(share[c]), frac


def _round_bf16(a):
    from oracle import oracle as O
    return O.round_bf16(a)


def mode_oracle(mode):
    """Context in which the oracle's 16-bit rounding is the format of `mode` (fp16 emulation for "f16", nothing to do otherwise)."""
    import contextlib
    return f16_emulation() if mode == "f16" else contextlib.nullcontext()


# ---------------------------------------------------------------------------------------------- recipe facts
def scaled_weights(O, op, weights):
    """[K, Cout] raw weights and the same with the BN scale folded in, in double."""
    w = np.asarray(weights[f"conv{op.conv_index}.w"], np.float64).reshape(-1, op.cout)
    scale, _ = fold(O, op, weights)
    return w, w * scale.astype(np.float64)


# ---------------------------------------------------------------------------------------------- the f32x2 weight split, restated
def normalise_rows(ws):
    """csrc/y3_net.cpp, normalise_rows: the BN-scaled weights [K, Cout] with every output channel n divided by 2^e_n, e_n such that the
    channel's largest magnitude lands in [1, 2) (0 for an all-zero channel) -> (normalised weights, e)."""
    ws = np.ascontiguousarray(ws, np.float32)
    mx = np.abs(ws).max(axis=0)
    e = np.where(mx > 0, np.floor(np.log2(np.where(mx > 0, mx, 1.0).astype(np.float64))), 0).astype(np.int32)
    return np.ldexp(ws, -e[None, :]).astype(np.float32), e


def split_f16x2(v):
    """csrc/y3_net.cpp, split_f16x2: v (fp32) -> (h, l'), h = f16(v), l' = f16((v - h) * 2048), both round-to-nearest-even with
    subnormals kept; the kernel's sum is h + l' / 2048."""
    v = np.ascontiguousarray(v, np.float32)
    h = round_f16(v)
    lo = round_f16(((v - h) * np.float32(2048.0)).astype(np.float32))
    return h, lo


def flush_f16_subnormals(a):
    """fp16-exact values with the subnormals (|a| < 2^-14) replaced by zero: what a flush-to-zero operand path would read."""
    return np.where(np.abs(a) < np.float32(2.0 ** -14), np.float32(0.0), a).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the whole network of tier f
NET_S, NET_B, NET_SEED = 64, 2, 77
_net_cache = {}


def network_case(program):
    """(weights, images) of the calibrated 2 x 64^2 network, computed once per process and left read-only."""
    if "w" not in _net_cache:
        x = np.random.default_rng(NET_SEED).random((NET_B, NET_S, NET_S, 3), dtype=np.float32)
        w = calibrated_weights(program, NET_SEED, x)
        for a in list(w.values()) + [x]:
            a.setflags(write=False)
        _net_cache["w"], _net_cache["x"] = w, x
    return _net_cache["w"], _net_cache["x"]


# ---------------------------------------------------------------------------------------------- the programs of the GPU tier
# Every case is (program, weights, fp32 input), made once per process and left read-only; tests/test_bn_stats_host.py asserts the
# recipe facts and the reference floors on each of them, tests/test_bn_stats_gpu.py runs them.
SEED = 29
TILE_CANVAS, TILE_BATCH = (14, 10), 3          # M = 420 / 105: ragged against every BM, tiles span images, Ho != Wo
RESIDENT_F32 = [(64, 41, 2)]                                   # (cout, S, B), Cin 32: fp32 tile 33
RESIDENT_16 = [(64, 128, 36, 2), (32, 64, 33, 2)]              # (cin, cout, S, B): bf16 / fp16 tile 32
SPLITK_F32 = [("c64_13_res", 3, 11), ("head255", 4, 11), ("c256_13", 9, 10)]        # (name in tests/splitk_cases.LAYERS_F32, S, tile)
SPLITK_16 = [("c128_13_res", 3, 11), ("c128_13_head", 4, 12), ("c64_13_head", 8, 11), ("cin64_13_head", 3, 11),
             ("s2_14_head", 4, 11), ("b3_14_head", 4, 12)]     # the _res and _head cases of tests/splitk_cases.LAYERS_16, one S each
STEM_SIZES = [(32, 1), (64, 3)]                                # (S, B)
HEAD_GRIDS, HEAD_CANVAS, HEAD_BATCH = (2, 4, 8), 64, 3
HEAD_CLASS_COUNTS = (7, 80)                                    # 36 channels: the composed route; 255: the head convs decode their own tiles
STEM_TINY_CHANNEL = 9                                          # conv0 channel whose raw weights all lie below 2^-14
_cases = {}


def _frozen(key, make):
    if key not in _cases:
        out = make()
        for part in out:
            for a in (part.values() if isinstance(part, dict) else [part]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


def _normal(shape, seed=SEED):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def tile_case(bn, bk=32):
    """-> (program, {name: ConvOp}, weights, input [3, 14, 10, 64]) of helpers.tile_feature_program(bn, bk)."""
    from tests.helpers import tile_feature_program

    def make():
        p, ops = tile_feature_program(bn, bk)
        return p, ops, trained_like_weights(p, SEED), _normal((TILE_BATCH,) + TILE_CANVAS + (64,))
    return _frozen(("tile", bn, bk), make)


def resident_case(cin, cout, S, B):
    """The program of the weight-resident tests (tests/test_gpu_parity.py, tests/test_f16_gpu.py) on a [B, S, S, cin] input: three 3x3 /
    stride-1 convs cin -> cout -- BN + leaky, BN + leaky + shortcut, linear + bias -- with 1x1 convs between them and three 1x1 heads.
    cin = 32 is what fp32 tile 33 takes, cin = 32 / 64 what tile 32 of the 16-bit plans takes."""
    from tests.helpers import mini_program

    def make():
        chain = [dict(filters=cout, size=3), dict(filters=cin, size=1), dict(filters=cout, size=3, shortcut=-3),
                 dict(filters=cin, size=1, act="linear"), dict(filters=cout, size=3, bn=False, act="linear")]
        heads = [dict(filters=64, size=1), dict(filters=32, size=1), dict(filters=64, size=1, bn=False, act="linear")]
        p = mini_program(cin, chain, heads)
        return p, trained_like_weights(p, SEED + 1), _normal((B, S, S, cin), SEED + 1)
    return _frozen(("resident", cin, cout, S, B), make)


def splitk_case(sixteen, name):
    """A layer case of tests/splitk_cases.py, LAYERS_F32 (fp32) or LAYERS_16 (the 16-bit plans), with trained-like weights:
    -> (program, weights, input, B, size, split slots)."""
    from tests.helpers import mini_program

    def make():
        from tests.splitk_cases import LAYERS_16, LAYERS_F32
        LAYERS = LAYERS_16 if sixteen else LAYERS_F32
        in_ch, S, B, chain, heads, slots = LAYERS[name]
        p = mini_program(in_ch, chain, heads)
        return p, trained_like_weights(p, SEED + 2), _normal((B, S, S, in_ch), SEED + 2), B, S, tuple(slots)
    return _frozen(("splitk", bool(sixteen), name), make)


def _tiny_conv0_channel(w, c=STEM_TINY_CHANNEL):
    """conv0's channel c with every raw weight below 2^-14 and the same function: weights and BN mean x 2^-k, gamma x 2^k, k such that
    the channel's largest weight lands in [2^-15, 2^-14) -- the case pack_stem28_norm exists for."""
    mx = float(np.abs(w["conv0.w"][..., c]).max())
    k = 15 + int(np.floor(np.log2(mx)))
    for key, f in (("conv0.w", -k), ("conv0.mean", -k), ("conv0.gamma", k)):
        a = w[key].copy()
        a[..., c] = np.ldexp(a[..., c], f)
        w[key] = a
    assert 2.0 ** -15 <= float(np.abs(w["conv0.w"][..., c]).max()) < 2.0 ** -14 and w["conv0.gamma"][c] != 0
    return w


def stem_case(kind, S, B):
    """The stem programs on a [B, S, S, 3] image in [0, 1), trained-like conv0 / conv1 / conv2, conv0's channel 9 with raw weights below
    2^-14 and channels 3 and 19 with gamma 0.
      "block":    conv0, conv1, the 1x1 conv2 and the 3x3 + shortcut that closes the first residual block, three linear 32-filter 1x1
                  heads with bias (the program of test_fused_stem_bf16_third_layer_bit_identical_to_its_own_launch, all heads fp32);
      "identity": conv0, conv1 and three identity 1x1 heads through which conv1's stored output is read bit for bit."""
    from tests.helpers import mini_program

    def make():
        if kind == "block":
            lin = dict(filters=32, size=1, bn=False, act="linear")
            p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2), dict(filters=32, size=1),
                                 dict(filters=64, size=3, shortcut=-3)], [lin, lin, dict(filters=64, size=1)])
            w = trained_like_weights(p, SEED + 3)
        else:
            assert kind == "identity", kind
            ident = dict(filters=64, size=1, bn=False, act="linear")
            p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2)], [ident, ident, ident])
            w = trained_like_weights(p, SEED + 3)
            for i in (2, 3, 4):
                w[f"conv{i}.w"] = np.eye(64, dtype=np.float32).reshape(1, 1, 64, 64)
                w[f"conv{i}.bias"] = np.zeros(64, np.float32)
        w = _tiny_conv0_channel(w)
        return p, w, np.random.default_rng(SEED + 3).random((B, S, S, 3), dtype=np.float32)
    return _frozen(("stem", kind, S, B), make)


def head_case(nc):
    """One head conv per scale behind the smallest backbone that reaches the three scales from an image (forward_decode takes images
    only): conv0 3 -> 32, then five 3x3 / 2 convs to 64 channels; the last three feed one linear 1x1 head each, bias N(0, 3), 3 (5 + nc)
    channels, outputs coarsest first.  Three 64 x 64 images in [0, 1)."""
    from yolo_v3_tf2_amd.graph import Program, _Builder, _lower

    def make():
        b = _Builder(nc, None)
        x = b.new_tensor(3, 1, "input")
        bn = dict(size=3, activation="leaky", batch_normalize=1)
        head = dict(filters=3 * (5 + nc), size=1, stride=1, activation="linear")
        t = b.conv(x, dict(filters=32, stride=1, **bn), "body")
        scales = []
        for _ in range(5):
            t = b.conv(t, dict(filters=64, stride=2, **bn), "body")
            scales.append(t)
        outs = [b.yolo(b.conv(t, head, "head"), "head") for t in scales[:1:-1]]
        p = Program(b.tensors, b.nodes, [], x, outs, nc)
        p.conv_nodes = [n for n in b.nodes if n.kind == "conv"]
        _lower(p)
        images = np.random.default_rng(SEED + 4).random((HEAD_BATCH, HEAD_CANVAS, HEAD_CANVAS, 3), dtype=np.float32)
        return p, trained_like_weights(p, SEED + 4), images
    return _frozen(("head", nc), make)


RANGE_CHANNEL = 8


def range_case(over):
    """Three trained-like 1x1 BN convs 64 -> 64 on a [2, 8, 8, 64] input of N(0, 2^-24) (so that the outputs stay below 1000); conv0's
    channel 8 has BN mean 0 and its gamma set so that the largest BN-scaled weight of the channel, in the library's own fp32 arithmetic, is
    65504 x (1 + 1e-3) (over: the two-plane mode's range check refuses the net) or 65504 x (1 - 1e-3) (the net plans in every mode)."""
    from tests.helpers import mini_program

    def make():
        p = mini_program(64, [], [dict(filters=64, size=1)] * 3)
        w = trained_like_weights(p, SEED + 5)
        c = RANGE_CHANNEL
        inv = np.float32(1.0) / np.sqrt(w["conv0.var"][c] + np.float32(BN_EPS), dtype=np.float32)
        mx = float(np.abs(w["conv0.w"][..., c]).max())
        g = w["conv0.gamma"].copy()
        g[c] = np.float32(65504.0 * (1.0 + (1e-3 if over else -1e-3)) / (mx * float(inv)))
        w["conv0.gamma"] = g
        mean = w["conv0.mean"].copy()
        mean[c] = 0.0
        w["conv0.mean"] = mean
        top = float(np.abs(w["conv0.w"][..., c] * (inv * g[c])).max())
        assert (top >= 65504.0) == bool(over) and abs(top / 65504.0 - 1.0) < 2e-3, top
        return p, w, np.ldexp(_normal((2, 8, 8, 64), SEED + 5), -12)
    return _frozen(("range", bool(over)), make)


def oracle_tensors(program, weights, x, mode="f32"):
    """Every tensor of the oracle's own walk of `program` (fp32 sums), by the program's tensor ids: what the host tier feeds the launches
    it restates.  A 16-bit mode rounds where such a plan stores and holds the MFMA convs' weights in the format."""
    from oracle import oracle as O
    with mode_oracle(mode):
        _, kept = O._forward_nodes(program, weights, x, False, set(range(len(program.tensors))), mode in ("bf16", "f16"))
    kept[program.input_tensor] = np.ascontiguousarray(x, np.float32)
    if mode in ("bf16", "f16") and x.shape[-1] != 3:
        kept[program.input_tensor] = round_f16(x) if mode == "f16" else O.round_bf16(x)
    return kept


def tile_geometries():
    """(bn, bk) -> the plan modes whose built generic tiles have that geometry ("f32" also stands for f32x3 / f32x2: same reference)."""
    from yolo_v3_tf2_amd import _lib
    geo = {}
    for t, row in enumerate(_lib.TILES):
        if row[0] > 0 and t != 33:
            geo.setdefault((row[1], 32), set()).add("f32")
    for t in set(_lib.TILES_X3_BUILT) | set(_lib.TILES_X2_BUILT):
        geo.setdefault((_lib.TILES_X3[t][1], _lib.TILES_X3[t][3]), set()).add("f32")
    for t, row in enumerate(_lib.TILES_BF16):
        if row[0] > 0 and t != 32:
            geo.setdefault((row[1], row[3]), set()).update(("bf16", "f16"))
    return geo


def all_cases(program=None):
    """{tag: (factory -> (program, weights, input), modes)} of every program the GPU tier runs; `program`: the YOLOv3 program for the
    "network" case (left out when None)."""
    out = {}
    for (bn, bk), modes in sorted(tile_geometries().items()):
        out[f"tile-bn{bn}-bk{bk}"] = (lambda bn=bn, bk=bk: tuple(tile_case(bn, bk)[i] for i in (0, 2, 3)), sorted(modes))
    for cout, S, B in RESIDENT_F32:
        out[f"resident-32-{cout}-{S}x{B}"] = (lambda a=(32, cout, S, B): resident_case(*a), ["f32"])
    for a in RESIDENT_16:
        out["resident-%d-%d-%dx%d" % a] = (lambda a=a: resident_case(*a), ["bf16", "f16"])
    for name, _, _ in SPLITK_F32:
        out[f"splitk-f32-{name}"] = (lambda n=name: splitk_case(False, n)[:3], ["f32"])
    for name, _, _ in SPLITK_16:
        out[f"splitk-16-{name}"] = (lambda n=name: splitk_case(True, n)[:3], ["bf16", "f16"])
    for S, B in STEM_SIZES:
        out[f"stem-block-{S}x{B}"] = (lambda a=("block", S, B): stem_case(*a), ["f32", "bf16", "f16"])
        out[f"stem-identity-{S}x{B}"] = (lambda a=("identity", S, B): stem_case(*a), ["bf16", "f16"])
    for nc in HEAD_CLASS_COUNTS:
        out[f"heads-nc{nc}"] = (lambda nc=nc: head_case(nc), ["f32", "bf16", "f16"])
    out["range-under"] = (lambda: range_case(False), ["f32"])
    out["range-over"] = (lambda: range_case(True), ["f32"])
    if program is not None:
        out["network"] = (lambda: (program,) + network_case(program), ["f32", "bf16", "f16"])
    return out


# ---------------------------------------------------------------------------------------------- the fused 16-bit stems
# conv1's stored output behind the fused conv0 (read through identity heads), per channel: every element within its own ulp + one ulp
# of m_c at unit scale (a conv0 value rounded the other way moves a conv1 sum by |w scale| x one ulp of the conv0 value, an absolute
# amount however small the element is); the fractions of elements that differ at all / by more than their own ulp + 1e-5 m_c within
# the caps of the existing stem tests (tests/test_gpu_parity.py for bf16, tests/test_f16_stem_host.py for fp16), which
# tests/test_bn_stats_host.py holds to the reference alone at half.
STEM_SLACK = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
STEM_DIFFER_CAP = {"bf16": 0.05, "f16": 1.7e-2}
STEM_BEYOND_CAP = {"bf16": 0.01, "f16": 7.4e-4}


def stem_compare(a, b, m, fmt):
    """-> (differing fraction, fraction differing by more than the element's own ulp + 1e-5 m_c, worst |a - b| as a share of the
    per-element bar ulp + STEM_SLACK m_c)."""
    ulp = (f16_ulp_elem if fmt == "f16" else bf16_ulp_elem)(a, b)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return float((d > 0).mean()), float((d > ulp + 1e-5 * m).mean()), float((d / (ulp + STEM_SLACK[fmt] * m)).max())


def stem_references(S, B, fmt):
    """conv1's stored output of stem_case("identity", S, B) by the oracle alone, read-only: "oracle" (fp32 sums, conv0 in fp32 arithmetic
    on fp32 weights), "oracle64" (double sums), for fp16 also "restated" (conv1 from f16_stem_cases.conv0_restated, the fused kernel's
    conv0 arithmetic); "m": conv1's channel magnitudes."""
    def make():
        from oracle import oracle as O
        p, w, x = stem_case("identity", S, B)
        c0, c1 = p.conv_ops()[0], p.conv_ops()[1]
        rnd = round_f16 if fmt == "f16" else O.round_bf16
        out = {}
        with mode_oracle(fmt):
            for name, acc64 in (("oracle", False), ("oracle64", True)):
                y0 = rnd(launch_reference(O, c0, w, {p.input_tensor: x}.__getitem__, fmt, acc64=acc64))
                out[name] = rnd(launch_reference(O, c1, w, {c0.dst: y0}.__getitem__, fmt, acc64=acc64))
                if not acc64:
                    out["m"] = channel_magnitude(O, c1, mode_weights(w, c1, fmt), {c0.dst: y0}.__getitem__)
            if fmt == "f16":
                from tests.f16_stem_cases import conv0_restated
                out["restated"] = rnd(launch_reference(O, c1, w, {c0.dst: conv0_restated(w, x)}.__getitem__, fmt, acc64=False))
        return (out,)
    return _frozen(("stem-refs", S, B, fmt), make)[0]
