"""What tests/test_f16_stem_host.py and tests/test_f16_stem_gpu.py share: the programs, weights and images of the fp16 fused stem's cases,
a NumPy restatement of the kernel's conv0 arithmetic (csrc/conv_stem.hip, conv_stem16<F16Elem>; include/y3.h, y3_net_set_stem_fusion_f16)
and the references of a case, computed once per process and left read-only.

The program is that of tests/test_gpu_parity.py::test_fused_stem_bf16_conv0_error_bounded_through_identity_heads: conv0 (3x3 / 1, 3 -> 32),
conv1 (3x3 / 2, 32 -> 64) and three 1x1 heads with identity weights, through which conv1's stored fp16 output is read bit for bit."""
import numpy as np

from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16

# (canvas, images).  32 x 32, one image: two tiles of 16 x 32 image pixels, conv1's zero row and column in every tile; 64 x 64, three
# images: image boundaries; 416 x 416, two images: 676 tiles, so a persistent workgroup walks a second one (512 are resident); 64 x 96.
CASES = {"s32_b1": (32, 1), "s64_b3": (64, 3), "s416_b2": (416, 2), "r64x96_b2": ((64, 96), 2)}
# plain: the image in [0, 1).  w_small: conv0's weights x 2^-16 with gamma x 2^16 (and the BN mean x 2^-16, which makes it the same
# function exactly: the per-channel normalisation must make it the same numbers).  img255: the image x 255.  img_tiny: the image x 2^-12, a quarter of the pixels below 2^-14 (the hi = 0 branch).
VARIANTS = ("plain", "w_small", "img255", "img_tiny")
VARIANT_CASE = "s64_b3"        # the case the three variants run on
GPU_CASES = [(c, "plain") for c in CASES] + [(VARIANT_CASE, v) for v in VARIANTS[1:]]
SEED = 13


def hw(canvas):
    return (canvas, canvas) if isinstance(canvas, int) else tuple(canvas)


def stem_program():
    from tests.helpers import mini_program
    ident = dict(filters=64, size=1, bn=False, act="linear")
    return mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2)], [ident, ident, ident])


def stem_inputs(case, variant="plain"):
    """-> (program, weights, fp32 image batch) of a case."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = stem_program()
    w = dict(synthetic_weights(p, seed=SEED))
    for i in (2, 3, 4):
        w[f"conv{i}.w"] = np.eye(64, dtype=np.float32).reshape(1, 1, 64, 64)
        w[f"conv{i}.bias"] = np.zeros(64, np.float32)
    canvas, B = CASES[case]
    H, W = hw(canvas)
    x = np.random.default_rng(SEED).random((B, H, W, 3), dtype=np.float32)
    if variant == "w_small":
        w["conv0.w"] = (w["conv0.w"] * np.float32(2.0 ** -16)).astype(np.float32)
        w["conv0.gamma"] = (w["conv0.gamma"] * np.float32(2.0 ** 16)).astype(np.float32)
        w["conv0.mean"] = (w["conv0.mean"] * np.float32(2.0 ** -16)).astype(np.float32)
    elif variant == "img255":
        x = (x * np.float32(255.0)).astype(np.float32)
    elif variant == "img_tiny":
        x = (x * np.float32(2.0 ** -12)).astype(np.float32)
    else:
        assert variant == "plain", variant
    return p, w, x


# ---------------------------------------------------------------------------------------------- the kernel's conv0 arithmetic, restated
def split_f16(v):
    """v (fp32) -> (hi, lo'), both fp16-exact fp32 arrays: hi = |v| < 2^-14 ? 0 : f16(v), lo' = f16((v - hi) * 2048)."""
    v = np.ascontiguousarray(v, np.float32)
    hi = np.where(np.abs(v) < np.float32(2.0 ** -14), np.float32(0.0), round_f16(v)).astype(np.float32)
    lo = round_f16((v - hi) * np.float32(2048.0))
    return hi, lo


def normalise_w0(w_hwio):
    """conv0's weights [3, 3, 3, 32] -> ([28][32] rows k = (u * 3 + v) * 3 + c divided per output channel n by 2^e_n, row 27 zero; e [32]),
    e_n with max_k |w[k][n]| 2^-e_n in [1, 2), 0 for an all-zero channel: what y3_net_set_conv_weights uploads for the fp16 stem kernel."""
    w27 = np.ascontiguousarray(w_hwio, np.float32).reshape(27, -1)
    mx = np.abs(w27).max(axis=0)
    e = np.where(mx > 0, np.floor(np.log2(np.where(mx > 0, mx, 1.0).astype(np.float64))), 0).astype(np.int32)
    w28 = np.zeros((28, w27.shape[1]), np.float32)
    w28[:27] = np.ldexp(w27, -e[None, :]).astype(np.float32)
    return w28, e


# K slots of the two MFMA steps (16 each; conv_stem.hip): step 0 takes k = 0..7 and 9..16, step 1 k = 18..25 and 8, 17, 26 (the rest zero weight)
K_STEPS = ([0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16], [18, 19, 20, 21, 22, 23, 24, 25, 8, 17, 26])


def conv0_sums(x, w28):
    """The kernel's conv0 sums: [B, H, W, 32] fp32 from the image batch and the normalised weights.  Per MFMA the products are summed in
    double and the accumulator rounded to fp32 once (the matrix pipe's own order inside an instruction is not modelled); the order of the
    MFMAs is the kernel's: cross terms of step 0, of step 1, x 2^-11, then hi * hi of step 0 and of step 1."""
    B, H, W, _ = x.shape
    xp = np.zeros((B, H + 2, W + 2, 3), np.float32)
    xp[:, 1:-1, 1:-1] = x
    cols = np.stack([xp[:, u:u + H, v:v + W, c] for u in range(3) for v in range(3) for c in range(3)], axis=-1).reshape(-1, 27)
    xh, xl = split_f16(cols)
    wh, wl = split_f16(w28[:27])
    f64 = np.float64
    acc = np.zeros((cols.shape[0], w28.shape[1]), np.float32)
    for ks in K_STEPS:
        acc = (acc + xl[:, ks].astype(f64) @ wh[ks].astype(f64)).astype(np.float32)
        acc = (acc + xh[:, ks].astype(f64) @ wl[ks].astype(f64)).astype(np.float32)
    acc = acc * np.float32(2.0 ** -11)
    for ks in K_STEPS:
        acc = (acc + xh[:, ks].astype(f64) @ wh[ks].astype(f64)).astype(np.float32)
    return acc.reshape(B, H, W, -1)


def conv0_restated(w, x):
    """conv0 as the fused kernel stores it into its LDS patch: the sums above, * (scale * 2^e) + shift, leaky, rounded to fp16."""
    from oracle import oracle as O
    w28, e = normalise_w0(w["conv0.w"])
    scale, shift = O.bn_fold(w["conv0.gamma"], w["conv0.beta"], w["conv0.mean"], w["conv0.var"])
    v = conv0_sums(x, w28) * np.ldexp(scale, e).astype(np.float32) + shift
    v = np.maximum(v, np.float32(0.1) * v).astype(np.float32)
    return round_f16(v)


_refs = {}


def references(case, variant="plain"):
    """conv1's stored fp16 output [B, H/2, W/2, 64] three ways, read-only: "oracle" -- the fp16-emulating oracle (fp32 sums, conv0 in fp32
    arithmetic on fp32 weights: the one-launch-per-conv plan's arithmetic); "oracle64" -- the same with double accumulation (another order
    of the same sums, as a second pipeline has); "restated" -- conv1 (fp32 sums) from the restated conv0 of the fused kernel."""
    key = (case, variant)
    if key not in _refs:
        from oracle import oracle as O
        from tests.helpers import oracle_launch
        p, w, x = stem_inputs(case, variant)
        c0, c1 = p.conv_ops()[0], p.conv_ops()[1]
        out = {}
        with f16_emulation():
            for name, acc64 in (("oracle", False), ("oracle64", True)):
                y0 = round_f16(oracle_launch(O, c0, w, {p.input_tensor: x}.__getitem__, acc64=acc64))
                out[name] = round_f16(oracle_launch(O, c1, w, {c0.dst: y0}.__getitem__, acc64=acc64, bf16_weights=True))
            out["restated"] = round_f16(oracle_launch(O, c1, w, {c0.dst: conv0_restated(w, x)}.__getitem__, acc64=False, bf16_weights=True))
        for a in out.values():
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def compare(a, b, scale):
    """-> (differing fraction, fraction differing by more than the element's own fp16 ulp + 1e-5 scale, worst |a - b| as a fraction of
    the per-element bar f16_ulp_elem + 2^-11 scale)."""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    ulp = f16_ulp_elem(a, b)
    return float((d > 0).mean()), float((d > ulp + 1e-5 * scale).mean()), float((d / (ulp + 2.0 ** -11 * scale)).max())
