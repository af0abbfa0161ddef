// The net object of liby3hip.so behind the C ABI (include/y3.h): error buffer and exception barrier, create / destroy, weight packing,
// the setters, the conv families with their tile heuristics, the launch decision (choose_conv) and the split-K resolution.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>

#include "y3_host.h"

namespace {

// The last error of this thread: a fixed buffer, so that reporting a failure allocates nothing and cannot itself throw
// (include/y3.h: no entry point throws or aborts -- not even while it reports that the host ran out of memory).
thread_local char g_err[512] = "";

}  // namespace

namespace y3 {   // declared, with what they are for, in y3_host.h
int fail_msg(int code, const char *fmt, ...) noexcept
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int on_exception(const char *who) noexcept
{
    try {
        throw;
    } catch (const std::bad_alloc &) {
        return fail_msg(Y3_ERR_OOM, "%s: out of host memory (std::bad_alloc)", who);
    } catch (const std::exception &e) {
        return fail_msg(Y3_ERR_INTERNAL, "%s: C++ exception: %s", who, e.what());
    } catch (...) {
        return fail_msg(Y3_ERR_INTERNAL, "%s: unknown C++ exception", who);
    }
}

bool test_fail_alloc() noexcept
{
    const char *e = getenv("Y3_TEST_FAIL_ALLOC");
    return e && e[0] == '1';
}

}  // namespace y3

namespace {

unsigned short f32_to_bf16_rne(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);  // NaN stays NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

float bf16_to_f32(unsigned short h)
{
    unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// fp32 -> fp16 bits, round to nearest even, subnormals kept, >= 65520 -> inf
unsigned short f32_to_f16_rne(float f)
{
    unsigned x;
    memcpy(&x, &f, 4);
    const unsigned short sign = (unsigned short)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (unsigned short)(sign | 0x7e00u);
    if (x >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u);
    if (x < 0x38800000u) {   // below 2^-14: a multiple of 2^-24
        float a;
        memcpy(&a, &x, 4);
        return (unsigned short)(sign | (unsigned short)lrintf(a * 16777216.0f));
    }
    unsigned h = (((x >> 23) - 112u) << 10) | ((x & 0x7fffffu) >> 13);
    const unsigned rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
    return (unsigned short)(sign | h);
}

float f16_to_f32(unsigned short h)
{
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    float v;
    if (e == 0)
        v = ldexpf((float)m, -24);
    else if (e == 31)
        v = m ? NAN : INFINITY;
    else
        v = ldexpf((float)(1024 + m), e - 25);
    return (h & 0x8000) ? -v : v;
}

// ---- weight packing (y3_net_set_conv_weights): HWIO w is [K][Cout], k = tap*Cin + c

// [CoutPad][K], rows past Cout zero; scale (or null): folded into each output channel's row
std::vector<float> pack_rows(const float *w, int K, int cout, int cout_pad, const float *scale)
{
    std::vector<float> pk((size_t)cout_pad * K, 0.0f);
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < cout; ++n) pk[(size_t)n * K + k] = scale ? w[(size_t)k * cout + n] * scale[n] : w[(size_t)k * cout + n];
    return pk;
}

// first layer, fused stem kernel: conv0 on the matrix cores wants K = 27 padded to 28 rows of [Cout]; scale (or null) folded in
std::vector<float> pack_stem28(const float *w, int K, int cout, const float *scale)
{
    std::vector<float> w28((size_t)28 * cout, 0.0f);
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < cout; ++n) w28[(size_t)k * cout + n] = scale ? w[(size_t)k * cout + n] * scale[n] : w[(size_t)k * cout + n];
    return w28;
}

// fp16 plans' fused stem kernel: the 28 unscaled rows with every output channel n divided by 2^e_n, e_n such that the channel's largest
// magnitude lands in [1, 2) (0 for an all-zero channel) -- exact, a power of two -- and exps[n] = e_n for the kernel's conv0 scale
std::vector<float> pack_stem28_norm(const float *w, int K, int cout, std::vector<int> &exps)
{
    std::vector<float> w28 = pack_stem28(w, K, cout, nullptr);
    exps.assign(cout, 0);
    for (int n = 0; n < cout; ++n) {
        float mx = 0.0f;
        for (int k = 0; k < K; ++k) mx = std::max(mx, fabsf(w28[(size_t)k * cout + n]));
        if (!(mx > 0.0f) || !std::isfinite(mx)) continue;
        exps[n] = std::ilogb(mx);
        for (int k = 0; k < K; ++k) w28[(size_t)k * cout + n] = ldexpf(w28[(size_t)k * cout + n], -exps[n]);
    }
    return w28;
}

// three bf16 planes: x = hi + mid + lo exactly
void split_bf16x3(float x, unsigned short v[3])
{
    v[0] = f32_to_bf16_rne(x);
    const float r1 = x - bf16_to_f32(v[0]);
    v[1] = f32_to_bf16_rne(r1);
    v[2] = f32_to_bf16_rne(r1 - bf16_to_f32(v[1]));
}

// two-plane weights: every output channel's row of pk [CoutPad][K] divided by 2^e_n, e_n such that the row's largest magnitude lands in
// [1, 2) (0 for an all-zero row) -- exact, a power of two -- and pow2[n] = 2^e_n for the kernel's epilogue.  Without it a channel whose
// BN-scaled weights lie below 2^-13 (a small gamma over a large variance) has subnormal l' planes, 2^-36 absolute instead of 2^-22 relative.
std::vector<float> normalise_rows(std::vector<float> pk, int K, int cout, std::vector<float> &pow2)
{
    for (int n = 0; n < cout; ++n) {
        float mx = 0.0f;
        for (int k = 0; k < K; ++k) mx = std::max(mx, fabsf(pk[(size_t)n * K + k]));
        if (!(mx > 0.0f) || !std::isfinite(mx)) continue;
        const int e = std::ilogb(mx);
        pow2[n] = ldexpf(1.0f, e);
        for (int k = 0; k < K; ++k) pk[(size_t)n * K + k] = ldexpf(pk[(size_t)n * K + k], -e);
    }
    return pk;
}

// two fp16 planes: w = h + l' * 2^-11 (up to 2^-22 |w|) while |w| < 65504
void split_f16x2(float x, unsigned short v[2])
{
    v[0] = f32_to_f16_rne(x);
    v[1] = f32_to_f16_rne((x - f16_to_f32(v[0])) * 2048.0f);
}

// [rows][P][K] planes of [CoutPad][K] weights (rows past Cout zero), split(x, v) giving the P plane values of x
template <int P>
std::vector<unsigned short> pack_planes(const std::vector<float> &pk, int K, int cout, int rows, void (*split)(float, unsigned short *))
{
    std::vector<unsigned short> px((size_t)rows * P * K, 0);
    unsigned short v[P];
    for (int n = 0; n < cout; ++n)
        for (int k = 0; k < K; ++k) {
            split(pk[(size_t)n * K + k], v);
            for (int p = 0; p < P; ++p) px[((size_t)n * P + p) * K + k] = v[p];
        }
    return px;
}

// int8 plans: [rows][K] int8 of the raw [CoutPad][K] weights pk, symmetric per output channel: s_w[n] = absmax_n / 127 (1 for an all-zero
// channel), q = clamp(rint(w / s_w[n]), -127, 127) with a true fp32 division and round to nearest even; rows past Cout zero, their scale 1
std::vector<signed char> pack_i8(const std::vector<float> &pk, int K, int cout, int rows, std::vector<float> &sw)
{
    std::vector<signed char> q((size_t)rows * K, 0);
    sw.assign(rows, 1.0f);
    for (int n = 0; n < cout; ++n) {
        float mx = 0.0f;
        for (int k = 0; k < K; ++k) mx = std::max(mx, fabsf(pk[(size_t)n * K + k]));
        if (mx > 0.0f && std::isfinite(mx)) sw[n] = mx / 127.0f;
        for (int k = 0; k < K; ++k)
            q[(size_t)n * K + k] = (signed char)std::min(127.0f, std::max(-127.0f, nearbyintf(pk[(size_t)n * K + k] / sw[n])));
    }
    return q;
}

// hipMalloc the device buffer on first use, then copy the host vector into it
template <class P, class T>
hipError_t upload(P *&dev, const std::vector<T> &host)
{
    const size_t bytes = host.size() * sizeof(T);
    if (!dev)
        if (hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), bytes); e != hipSuccess) return e;
    return hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice);
}

// Does the tile divide the conv (y3::tile_fits)?  cout_pad: the padded Cout of the mode's weights (ConvSlot::cout_pad / cout_pad64)
bool fits(const y3::TileInfo &t, const ConvSlot &c, int cout_pad) { return y3::tile_fits(t, c.d.cin, c.d.src1 >= 0 ? c.d.c0 : -1, cout_pad); }

// The first candidate tile that fits the conv and gives at least `want` workgroups for M rows over `cout_pad` channels; when none
// reaches that count, the last candidate that fits (the lists run from the largest tile to the smallest); -1 when none fits at all.
template <size_t N>
int first_reaching(const int (&cand)[N], y3::TileInfo (*info)(int), const ConvSlot &c, int cout_pad, long long M, long long want)
{
    int last_fit = -1;
    for (int t : cand) {
        const y3::TileInfo s = info(t);
        if (!fits(s, c, cout_pad)) continue;
        if (((M + s.bm - 1) / s.bm) * (cout_pad / s.bn) >= want) return t;
        last_fit = t;
    }
    return last_fit;
}

int choose_tile_x2(const ConvSlot &c, long long M, long long, bool)
{
    // widest tile that still gives every CU at least two workgroups
    static constexpr int wide[] = {4, 8, 0, 3, 2}, narrow[] = {1, 2};
    if (c.cout_pad64 % 128 == 0) return first_reaching(wide, y3::conv_x3_tile_info, c, c.cout_pad64, M, 512);
    return first_reaching(narrow, y3::conv_x3_tile_info, c, c.cout_pad64, M, 512);
}

int choose_tile_x3(const ConvSlot &c, long long M, long long, bool)
{
    static constexpr int wide[] = {0, 3, 2}, narrow[] = {1, 2};
    if (c.cout_pad64 % 128 == 0) return first_reaching(wide, y3::conv_x3_tile_info, c, c.cout_pad64, M, 512);
    return first_reaching(narrow, y3::conv_x3_tile_info, c, c.cout_pad64, M, 512);
}

// M = rows of this call (per lane); M_plan = rows of the planned batch.  The MFMA SHAPE (16x16x32 vs 32x32x16: two K groupings,
// results differ in the last bits) is decided from plan-time quantities only, so that an image's result does not depend on the
// batch or lane it runs in (y3_net_set_lanes: "results are unchanged"); the tile SIZE within one shape follows the call.
int choose_tile_bf16(const ConvSlot &c, long long M, long long M_plan, bool bf16_out)
{
    auto blocks = [&](int t) {
        y3::TileInfo s = y3::conv_bf16_tile_info(t);
        return ((M + s.bm - 1) / s.bm) * (c.cout_pad / s.bn);
    };
    // large 3x3 convs: the 16x16x32 form once the PLANNED batch fills the chip with 256x256 tiles of 16 waves (tile 24 wins every
    // such signature of the 64- and 128-image tables, tuning/bf16_b*_s416.json); smaller calls of the same plan take the 128x128 /
    // 64x128 tiles of the same MFMA shape (27, 29)
    if (c.d.size == 3 && c.d.src1 < 0 && c.d.cin % 64 == 0 && c.cout_pad % 256 == 0 && ((M_plan + 255) / 256) * (c.cout_pad / 256) >= 256) {
        if (blocks(24) >= 256) return 24;
        return blocks(27) >= 512 ? 27 : 29;
    }
    // early 3x3 / stride-1 convs with Cin = 32 / 64 (K = 288 / 576): weights resident in LDS, input patch by LDS-DMA (tile id 32,
    // conv_res_bf16.hip) -- from the conv's shape alone, so batch- and lane-independent
    if (bf16_out && c.d.size == 3 && c.d.stride == 1 && c.d.src1 < 0 && (c.d.cin == 32 || c.d.cin == 64) && c.d.cout % 64 == 0) return 32;
    static constexpr int bk32[] = {5, 6},    // BK = 32, both 64 wide (the Cin = 32 layers; any Cin or concat boundary that 64 does not divide)
                         n128[] = {8, 12, 11},   // LDS-DMA variants: 128x128, 64x128, 64x64
                         n64[] = {10, 11}, n32[] = {4};
    // Cin % 64 == 0: the BK = 64 list of the widest N tile that divides Cout; its tiles fit unless the boundary c0 of a two-source conv is odd
    int t = -1;
    if (c.d.cin % 64 == 0)
        t = c.cout_pad % 128 == 0  ? first_reaching(n128, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512)
            : c.cout_pad % 64 == 0 ? first_reaching(n64, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512)
                                   : first_reaching(n32, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512);
    // Cin, or the boundary c0 of a two-source conv, is an odd multiple of 32: the BK = 32 tiles, which exist 64 wide only -- so a conv
    // whose padded Cout is an odd multiple of 32 as well has no 16-bit tile: -1, and y3_net_plan refuses the mode (conv_without_tile)
    if (t < 0) t = first_reaching(bk32, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512);
    return t;
}

// int8 plans: the bf16 chooser's tile where it has an int8 form (the LDS-DMA tiles with 128-byte rows, both MFMA shapes); where it has
// none (a Cout that only the 32-wide register-staged tile divides) the 64-wide LDS-DMA tiles over Cout padded to 64
int choose_tile_i8(const ConvSlot &c, long long M, long long M_plan, bool arena_out)
{
    const int t = choose_tile_bf16(c, M, M_plan, arena_out);
    if (t >= 0 && y3::conv_i8_tile_built(t) && fits(y3::conv_i8_tile_info(t), c, c.cout_pad64)) return t;
    static constexpr int n64[] = {10, 11};
    return first_reaching(n64, y3::conv_i8_tile_info, c, c.cout_pad64, M, 512);   // -1: Cin or c0 no multiple of 128 (never behind the cut)
}

// channels per K chunk of a 3x3 fp32 conv when the caller has not chosen (y3_net_set_k_chunk(-1)); Y3_K_CHUNK overrides (tools)
int default_k_chunk(const ConvSlot &c)
{
    static const int env = [] { const char *e = getenv("Y3_K_CHUNK"); return e ? atoi(e) : -1; }();
    if (env >= 0) return env;
    // 128 channels per chunk: traffic beyond L2 of the whole conv stack 42.1 -> 29.6 GB per 64-image step (1.96 x -> 1.42 x the
    // algorithmic bytes) at the same images/s (-0.1 %, inside the run-to-run spread); 64 per chunk: 27.2 GB but -0.4 %
    // (profiles/r03_k_chunk_sweep.txt, r03_traffic_per_layer_*.txt)
    return (c.d.size == 3 && c.d.cin >= 256) ? 128 : 0;
}

// the border-skip rule when the caller has not chosen (y3_net_set_border_skip(-1)): the eligible convs of at most kBorderSkipMaxPositions
// output positions; Y3_BORDER_SKIP=0 (off) and Y3_BORDER_SKIP_MAX_POS override (tools).  No limit: at 64 x 416^2 on two lanes the step reads
// 30.467 / 30.416 / 30.246 / 30.224 ms with the skip allowed up to 13^2 / 26^2 / 52^2 / everywhere, 30.823 ms off (profiles/border_skip_ab.txt)
constexpr int kBorderSkipMaxPositions = 1 << 30;
bool default_border_skip(const y3::ConvArgs &a)
{
    static const int env = [] { const char *e = getenv("Y3_BORDER_SKIP"); return e ? atoi(e) : -1; }();
    static const int max_pos = [] { const char *e = getenv("Y3_BORDER_SKIP_MAX_POS"); return e ? atoi(e) : kBorderSkipMaxPositions; }();
    return env != 0 && a.Ho * a.Wo <= max_pos;
}
// ... and its launches deal their border and interior tiles evenly over the XCD M-ranges (y3_kernels.h, balanced_tile); Y3_BORDER_BALANCE=0:
// the tile -> XCD mapping of the raster launches, under which one range gets every short tile (tools: the A/B of profiles/border_balance_ab.txt)
bool border_balance()
{
    static const int env = [] { const char *e = getenv("Y3_BORDER_BALANCE"); return e ? atoi(e) : 1; }();
    return env != 0;
}

// How the 8 XCDs (each with its own 4 MB L2) divide the tile matrix of one fp32 conv launch: as a (8/gn) x gn grid of
// blocks.  An XCD then streams 1/gn of the weights and 1/gm of the activations; the L2-miss traffic of the launch is
// about gn * (activation bytes) + gm * (weight bytes), provided an XCD's weight slice stays L2-resident (<= 2.5 MB) while
// its workgroups walk the K loop.  0 = not applicable (tile count too small / not divisible).
int choose_xcd_gn(const ConvSlot &c, const y3::ConvArgs &a, const y3::TileInfo &t)
{
    const int tilesN = a.CoutPad / t.bn;
    const long long tilesM = (a.M + t.bm - 1) / t.bm;
    if (tilesM * tilesN < 64) return 0;
    const double w_bytes = (double)a.CoutPad * c.K * 4.0, a_bytes = (double)a.src0_bytes + a.src1_bytes;
    int best = 0;
    double best_cost = 0;
    for (int gn = 1; gn <= 8; gn *= 2) {
        const int gm = 8 / gn;
        if (tilesN % gn || tilesM < gm) continue;
        double cost = gn * a_bytes + gm * w_bytes;
        if (w_bytes / gn > 2.5e6) cost += 8.0 * (a_bytes + w_bytes);   // weight slice does not stay in L2: last resort
        if (!best || cost < best_cost) {
            best = gn;
            best_cost = cost;
        }
    }
    return best > 1 ? best : 0;   // gn = 1 is the contiguous order (8 pixel-tile runs), which needs no padding workgroups
}

int choose_tile(const ConvSlot &c, long long M, long long, bool)
{
    // the first residual block's 3x3 (32 -> 64 @208): weights resident in registers, input patch by LDS-DMA (tile id 33, conv_res_f32.hip).
    // From the conv's shape alone (never the rows of the call); bit-identical to the generic tiles anyway.
    if (c.d.size == 3 && c.d.stride == 1 && c.d.src1 < 0 && c.d.cin == 32 && c.d.cout % 64 == 0 && c.cout_pad == c.d.cout) return 33;
    // measured on MI355X (tools/tune_tiles.py): many co-resident waves beat big wave tiles for the 64-cycle
    // fp32 MFMA; prefer the largest block tile that still yields >= 2 workgroups per CU
    static constexpr int n128[] = {10, 11}, n64[] = {11}, n32[] = {8};
    if (c.cout_pad % 128 == 0) return first_reaching(n128, y3::conv_tile_info, c, c.cout_pad, M, 1024);
    if (c.cout_pad % 64 == 0) return first_reaching(n64, y3::conv_tile_info, c, c.cout_pad, M, 1024);
    return first_reaching(n32, y3::conv_tile_info, c, c.cout_pad, M, 1024);
}

}  // namespace

// The first two ops are conv0 (3x3/1, 3 -> 32) and conv1 (3x3/2, 32 -> 64, no shortcut, single source) reading it, nobody
// else reads conv0's output, and the plan's mode has a fused stem with every intermediate reusable: the pair runs as csrc/conv_stem.hip.
bool y3::stem_applicable(const y3_net *net)
{
    if (!family_of(net).launch_stem || net->kept || net->height % 32 || net->width % 32 || net->early_ops > 0)
        return false;
    if (net->ops.size() < 2 || net->ops[0].kind != 0 || net->ops[1].kind != 0) return false;
    const ConvSlot &c0 = net->convs[net->ops[0].index], &c1 = net->convs[net->ops[1].index];
    const y3_conv_desc &a = c0.d, &b = c1.d;
    if (!c0.first_layer || a.size != 3 || a.stride != 1 || a.cout != 32 || a.residual >= 0 || a.src1 >= 0) return false;
    if (b.size != 3 || b.stride != 2 || b.cin != 32 || b.cout != 64 || b.residual >= 0 || b.src1 >= 0 || b.src0 != a.dst) return false;
    if (a.src0 != net->input_tensor) return false;
    if (is_output(net, a.dst) || is_output(net, b.dst)) return false;
    for (size_t i = 2; i < net->ops.size(); ++i) {
        if (net->ops[i].kind == 0) {
            const y3_conv_desc &d = net->convs[net->ops[i].index].d;
            if (d.src0 == a.dst || d.src1 == a.dst || d.residual == a.dst) return false;
        } else {
            const y3_aux_desc &x = net->aux[net->ops[i].index];
            if (x.src0 == a.dst || x.src1 == a.dst) return false;
        }
    }
    return true;
}

// third op = 1x1 conv 64 -> 32 reading conv1's output (backbone.yaml layer 3): computed by the stem kernel from the tile it
// still holds on chip (fp32 and bf16 plans)
bool y3::stem_conv2_applicable(const y3_net *net)
{
    if (!family_of(net).launch_stem || net->ops.size() < 3 || net->ops[2].kind != 0) return false;
    const y3_conv_desc &b = net->convs[net->ops[1].index].d, &c = net->convs[net->ops[2].index].d;
    if (c.size != 1 || c.stride != 1 || c.cin != 64 || c.cout != 32 || c.residual >= 0 || c.src1 >= 0 || c.src0 != b.dst) return false;
    return !is_output(net, c.dst);
}

// The planned mode's stem switch (y3_net_set_stem_fusion: fp32 and bf16 plans; y3_net_set_stem_fusion_f16: fp16 plans) and the graph decide
void y3::resolve_stem(y3_net *net)
{
    const ConvFamily &f = family_of(net);
    const int mode = f.launch_stem ? net->*f.stem_mode : 0;
    net->stem_fused = mode && stem_applicable(net);
    net->stem_conv2 = net->stem_fused && mode == 1 && stem_conv2_applicable(net);
}

// The fused stem of YOLOv3-tiny (csrc/conv_tiny_stem.hip).  Ops 0..3 are conv0 (the 3x3/1 first layer, 3 -> 16 stored as 32) reading the input,
// Y3_AUX_MAXPOOL2X2_S2 on it, a 3x3/1 conv 16 (stored 32) -> 32 with a single source and no shortcut, and Y3_AUX_MAXPOOL2X2_S2 on that; each of
// the first three outputs has exactly one reader, none of the four is a net output, there are no early chunks, and the plan's mode has the
// kernel (fp32, bf16, fp16; an int8 plan whose cut lies behind op 3 runs this part as an fp16 plan and takes the fp16 kernel).  The stored widths are all the graph tells: that conv0's channels 16..31 are zero pad channels is a property of its
// weights (ConvSlot::tiny_pad_zero), which the forward asks for.  keep_activations does not matter: the tensors inside are simply not stored.
bool y3::tiny_stem_applicable(const y3_net *net)
{
    if (net->height % 32 || net->width % 32 || net->early_ops > 0) return false;
    if (net->ops.size() < 5 || net->ops[0].kind != 0 || net->ops[1].kind == 0 || net->ops[2].kind != 0 || net->ops[3].kind == 0) return false;
    // the mode of conv1: the plan's, or fp16 before the cut of an int8 plan (resolve_i8 has run); conv1 itself behind the cut has no kernel
    if (!family_of_conv(net, net->ops[2].index).launch_tiny_stem) return false;
    const ConvSlot &c0 = net->convs[net->ops[0].index], &c1 = net->convs[net->ops[2].index];
    const y3_conv_desc &a = c0.d, &b = c1.d;
    const y3_aux_desc &p0 = net->aux[net->ops[1].index], &p1 = net->aux[net->ops[3].index];
    if (!c0.first_layer || a.size != 3 || a.stride != 1 || a.cout != 32 || a.residual >= 0 || a.src1 >= 0 || a.src0 != net->input_tensor) return false;
    if (p0.kind != Y3_AUX_MAXPOOL2X2_S2 || p0.src0 != a.dst) return false;
    if (b.size != 3 || b.stride != 1 || b.cin != 32 || b.cout != 32 || b.residual >= 0 || b.src1 >= 0 || b.src0 != p0.dst) return false;
    if (p1.kind != Y3_AUX_MAXPOOL2X2_S2 || p1.src0 != b.dst) return false;
    if (a.in_div != 1 || net->tensors[p1.dst].div != 4 || net->tensors[p1.dst].channels != 32) return false;
    const int inner[3] = {a.dst, p0.dst, b.dst};
    for (int t : {a.dst, p0.dst, b.dst, p1.dst})
        if (is_output(net, t) || t == net->input_tensor) return false;
    for (int t : inner) {   // exactly one reader, and nobody else writes it
        int readers = 0, writers = 0;
        for (const ConvSlot &c : net->convs) {
            readers += (c.d.src0 == t) + (c.d.src1 == t) + (c.d.residual == t);
            writers += c.d.dst == t;
        }
        for (const y3_aux_desc &x : net->aux) {
            readers += (x.src0 == t) + (x.src1 == t);
            writers += x.dst == t;
        }
        if (readers != 1 || writers != 1) return false;
    }
    return true;
}

void y3::resolve_tiny_stem(y3_net *net)
{
    net->tiny_stem_fused = net->tiny_stem_mode == 1 && tiny_stem_applicable(net);
    net->tiny_inner.assign(net->tensors.size(), 0);
    if (!net->tiny_stem_fused) return;
    net->tiny_inner[net->convs[net->ops[0].index].d.dst] = 1;
    net->tiny_inner[net->aux[net->ops[1].index].dst] = 1;
    net->tiny_inner[net->convs[net->ops[2].index].d.dst] = 1;
}

// Is net output t staged in a non-fp32 plan -- produced in the arena in the mode's own format and converted into the caller's fp32
// grid at the end of the forward -- because a conv reads it again inside the net, or a conv with no fp32-output form of its launch
// (shortcut, first layer) writes it?  Needs no plan: y3_net_plan marks `staged` by it, and y3_net_set_tile_bf16 refuses the
// bf16-only tile 32 on a conv whose output is not staged.
bool y3::output_staged(const y3_net *net, int t)
{
    for (const Op &o : net->ops) {
        if (o.kind != 0) continue;
        const ConvSlot &c = net->convs[o.index];
        if (c.d.src0 == t || c.d.src1 == t || c.d.residual == t) return true;
        if (c.d.dst == t && (c.d.residual >= 0 || c.first_layer)) return true;
    }
    return false;
}

namespace {

y3_status resident_rule_f32(const y3_net *, const ConvSlot &c, int)
{
    if (!(c.d.size == 3 && c.d.stride == 1 && c.d.src1 < 0 && c.d.cin == 32 && c.d.cout % 64 == 0))
        return fail(Y3_ERR_INVALID, "y3_net_set_tile: tile 33 (weight-resident) needs a 3x3 / stride-1 conv with 32 input channels and Cout %% 64 == 0");
    return Y3_OK;
}

y3_status resident_rule_bf16(const y3_net *net, const ConvSlot &c, int slot)
{
    if (!(c.d.size == 3 && c.d.stride == 1 && c.d.src1 < 0 && (c.d.cin == 32 || c.d.cin == 64) && c.d.cout % 64 == 0))
        return fail(Y3_ERR_INVALID, "y3_net_set_tile_bf16: tile 32 (weight-resident) needs a 3x3 / stride-1 conv with 32 or 64 input channels and Cout %% 64 == 0");
    // tile 32 stores bf16 only: a conv whose destination is a net output that the forward hands over as fp32 straight from the launch
    // (not read again inside the net, no shortcut: y3_net_plan does not stage it) cannot take it -- refused here, by name, instead of a
    // launch error in the forward
    if (is_output(net, c.d.dst) && !y3::output_staged(net, c.d.dst))
        return fail(Y3_ERR_INVALID, "y3_net_set_tile_bf16: tile 32 (weight-resident) stores bf16 only; conv %d writes an fp32 net output", slot);
    return Y3_OK;
}

// fp32 plans: the head kernel when the conv decodes its own tiles; else the split resolve_splits decided, the XCD order and the K order
void refine_f32(const y3_net *net, const ConvSlot &c, const y3::ConvArgs &a, y3::ConvChoice &ch)
{
    if (a.dec.boxes) { ch.kind = y3::ConvKind::HeadDecodeF32; return; }
    ch.split_k = c.split_k;
    if (c.split_k > 1) ch.kind = y3::ConvKind::SplitK;   // low-latency plan: S slices of the K walk into the lane's slabs, then the finish launch
    else if (net->xcd_mode) ch.xcd_gn = choose_xcd_gn(c, a, y3::conv_tile_info(ch.tile));
    // K order of the 3x3 convs (conv_f32.hip): chunk-major when the conv has more input channels than one chunk
    const int ck = net->k_chunk >= 0 ? net->k_chunk : default_k_chunk(c);
    if (c.d.size == 3 && c.d.src1 < 0 && ck > 0 && c.d.cin > ck && c.d.cin % ck == 0 && ck % 32 == 0) ch.k_chunk = ck;
    // Border skip: batch-minor rows over the geometry's position table (c.pos_tab: fp32 plan, 3x3, single source), for the generic tiles of
    // an unsplit launch whose images come in whole 32-row blocks; the row step of an accumulator block (one image) must fit the scalar offset
    const bool legal = c.pos_tab && ch.kind == y3::ConvKind::Mfma && ch.tile != 33 && a.B >= 32 && a.B % 32 == 0 &&
                       (long long)a.Ho * a.Wo * a.Cout * 4 * 32 < 0x7fffffffLL;
    if (legal && (net->border_skip >= 0 ? net->border_skip == 1 : default_border_skip(a))) {
        ch.pos_tab = c.pos_tab;
        // the leading tiles that hold a border position, for the balanced tile -> XCD mapping (y3_kernels.h): rows are m = j * B + b and the
        // border positions are the table's first, so every tile that begins below row pos_border * B
        const long long bm = y3::conv_tile_info(ch.tile).bm;
        if (border_balance()) ch.border_tiles = (int)std::min(((long long)c.pos_border * a.B + bm - 1) / bm, (a.M + bm - 1) / bm);
    }
}

// bf16 and fp16 plans: a head conv that decodes its own tiles needs a 256-wide tile
void refine_bf16(const y3_net *, const ConvSlot &c, const y3::ConvArgs &a, y3::ConvChoice &ch)
{
    if (c.split_k > 1 && !a.dec.boxes) {   // low-latency plan: S slices of the K walk into the lane's slabs, then the finish launch
        ch.split_k = c.split_k;
        ch.kind = y3::ConvKind::SplitK;
        return;
    }
    if (a.dec.boxes && y3::conv_bf16_tile_info(ch.tile).bn != 256) {   // a box's logits must meet in one workgroup: all 256 channels in the tile
        const bool m16 = ch.tile >= 24 && ch.tile <= 29;               // keep the MFMA shape of the plan's tile: same K grouping, same bits
        const bool big = (a.M + 255) / 256 >= 256;                     // 256x256 once it fills the chip, else 128x256 (16 waves both)
        ch.tile = m16 ? (big ? 24 : 26) : (big ? 17 : 19);
    }
}

hipError_t launch_f32(const y3::ConvArgs &a, int tile, bool, hipStream_t s) { return y3::launch_conv_f32(a, tile, s); }
hipError_t launch_f32_split(const y3::ConvArgs &a, int tile, bool, int S, void *ws, size_t n, hipStream_t s) { return y3::launch_conv_f32_split(a, tile, S, ws, n, s); }

// K tiles of 64 from which the rule splits a bf16 conv.  bf16 plans leave a conv of fewer than 32 K tiles to its one launch: in
// profiles/latency_bf16_splitk_sweep.txt every conv of 36 or 72 K tiles gains from the rule's S at every batch from 1 to 8, while the
// convs of 4 .. 18 K tiles (launches of 7 .. 15 us) lose to the finish launch and the slab traffic at some batch (the 13^2 1x1 of 16 K
// tiles: -2 us at one image, +3.5 us at eight; the 52^2 3x3 of 18 K tiles: +1.5 .. +5 us).  The sweep times one net object at every S; the
// end-to-end runs of profiles/latency_bf16.txt cannot resolve this at eight images (two net objects differ by more).  A forced S is taken
// as given.  Y3_SPLIT_MIN_K_TILES_BF16: a variant build for the record (csrc/build.py --variant OUT.so y3_net.cpp
// -DY3_SPLIT_MIN_K_TILES_BF16=0: y3_choose_split_k alone decides).
#ifndef Y3_SPLIT_MIN_K_TILES_BF16
#define Y3_SPLIT_MIN_K_TILES_BF16 32
#endif
constexpr int kSplitMinKTilesBf16 = Y3_SPLIT_MIN_K_TILES_BF16;

// fp32: tiles 10 and 11 (register-staged, BK = 32), any K, any Cout (the finish launch has a scalar form)
constexpr y3::SplitForm F32_SPLIT = {
    y3::conv_split_tile, launch_f32_split, 32, 0, &ConvSlot::split_req, &y3_net::low_latency, "y3_net_set_split_k", "y3_net_set_low_latency",
    [](int) { return "the conv's tile has no split form (tiles 10 and 11 have; the weight-resident tile 33 and the 32-wide tile 8 have not)"; },
    "tiles 10 and 11 have",
    "only Y3_DTYPE_F32 plans split K", 1, nullptr};
// bf16: tiles 11 and 12 (LDS-DMA, BK = 64, 32x32x16 MFMA); the finish launch stores bf16 in whole 16-byte pieces (a conv that writes an
// fp32 net output itself takes any Cout)
constexpr y3::SplitForm BF16_SPLIT = {
    y3::conv_bf16_split_tile, y3::launch_conv_bf16_split, 64, kSplitMinKTilesBf16, &ConvSlot::split_req_bf16, &y3_net::low_latency_bf16,
    "y3_net_set_split_k_bf16", "y3_net_set_low_latency_bf16",
    [](int tile) { return tile == 32 ? "the weight-resident tile 32 has no split form" : y3::conv_bf16_tile_info(tile).bk == 32
                       ? "the BK = 32 tiles (Cin = 32 layers) have no split form" : "the conv's tile has no split form (tiles 11 and 12 have)"; },
    "tiles 11 and 12 have",
    "only Y3_DTYPE_BF16 plans take a bf16 split", 8, "a split conv storing bf16 needs Cout % 8 == 0"};

// fp16: the bf16 row with the fp16 launcher, request and switch.  The floor is bf16's: the fp16 kernels are the bf16 ones instruction for
// instruction but the MFMA and the conversions of the epilogue.
constexpr y3::SplitForm F16_SPLIT = {
    y3::conv_bf16_split_tile, y3::launch_conv_f16_split, 64, kSplitMinKTilesBf16, &ConvSlot::split_req_f16, &y3_net::low_latency_f16,
    "y3_net_set_split_k_f16", "y3_net_set_low_latency_f16", BF16_SPLIT.no_form, BF16_SPLIT.tiles,
    "only Y3_DTYPE_F16 plans take an fp16 split", 8, "a split conv storing fp16 needs Cout % 8 == 0"};

// K tiles of 128 from which the rule splits an int8 conv: 36 (K >= 4608), the smallest K-tile count of
// profiles/latency_i8_splitk_sweep.txt from which every conv at or above it gains from the rule's S at every batch from 1 to 8 -- the
// 13^2 3x3 convs 512 -> 1024 (36 K tiles: 21.8 -> 16.1 us at one 416^2 image, 30.0 -> 24.9 us at eight).  Every shorter int8 conv is a
// launch of 7 .. 15 us that the finish launch and the slab traffic outweigh at some batch: the 26^2 3x3 of 18 K tiles is even at one image
// (-0.3 .. +0.3 us at S = 4) and loses 1 .. 6 us from two images on, the 52^2 3x3 of 9 K tiles and the 13^2 1x1 of 8 lose 1 .. 8 us at
// every batch.  int8 launches are about half as long as the 16-bit ones, so the finish launch weighs twice as much and the floor sits
// higher in K than the 16-bit one (32 tiles of 64).  A forced S is taken as given.  Y3_SPLIT_MIN_K_TILES_I8: a variant build for the
// record, as Y3_SPLIT_MIN_K_TILES_BF16 above (the sweep file was taken with 0, so that its "rule" column is y3_choose_split_k alone).
#ifndef Y3_SPLIT_MIN_K_TILES_I8
#define Y3_SPLIT_MIN_K_TILES_I8 36
#endif
constexpr int kSplitMinKTilesI8 = Y3_SPLIT_MIN_K_TILES_I8;

// int8: tiles 11 and 12 (LDS-DMA, BK = 128 channels, 32x32x32 MFMA); the slabs hold raw i32 sums and the finish launch stores int8 in whole
// 16-byte pieces of 16 channels (a conv that writes an fp32 net output itself takes any Cout).  Acts on the int8 convs of an int8 plan only:
// the fp16 convs before the cut stay unsplit under every switch (resolve_splits).
constexpr y3::SplitForm I8_SPLIT = {
    y3::conv_i8_split_tile, y3::launch_conv_i8_split, 128, kSplitMinKTilesI8, &ConvSlot::split_req_i8, &y3_net::low_latency_i8,
    "y3_net_set_split_k_i8", "y3_net_set_low_latency_i8",
    [](int) { return "the conv's tile has no split form (tiles 11 and 12 have)"; },
    "tiles 11 and 12 have",
    "only Y3_DTYPE_I8 plans take an int8 split", 16, "a split conv storing int8 needs Cout % 16 == 0"};

constexpr y3::ConvFamily F32_FAMILY = {
    y3::TILE_COUNT, y3::conv_tile_info, y3::conv_tile_built, &ConvSlot::tile, &ConvSlot::cout_pad,
    "y3_net_set_tile: bad argument", "y3_net_set_tile: tile id %d is retired (the timing ablations of rounds 1-2; y3_tile_built)",
    "y3_net_set_tile: tile does not divide Cout", 33, resident_rule_f32,
    &ConvSlot::w_dev, 4, choose_tile, launch_f32, refine_f32, y3::launch_conv_stem_f32, &ConvSlot::w0stem_dev, &ConvSlot::scale_dev, &y3_net::stem_mode,
    &F32_SPLIT, y3::launch_conv_tiny_stem_f32, &ConvSlot::w1tiny_dev};
constexpr y3::ConvFamily BF16_FAMILY = {
    y3::BF16_TILE_COUNT, y3::conv_bf16_tile_info, y3::conv_bf16_tile_built, &ConvSlot::tile_bf16, &ConvSlot::cout_pad,
    "y3_net_set_tile_bf16: bad argument",
    "y3_net_set_tile_bf16: tile id %d is retired (20: the pipelined tile of round 2; 33..36: tap-row reuse and the four-wave tile of round 4; y3_tile_built)",
    "y3_net_set_tile_bf16: tile does not fit this conv", 32, resident_rule_bf16,
    &ConvSlot::wbf_dev, 2, choose_tile_bf16, y3::launch_conv_bf16, refine_bf16, y3::launch_conv_stem_bf16, &ConvSlot::w0raw_dev, &ConvSlot::scale_dev,
    &y3_net::stem_mode, &BF16_SPLIT, y3::launch_conv_tiny_stem_bf16, &ConvSlot::w1tiny_bf_dev};
// fp16 plans: the bf16 family's tile table, forced-tile field, chooser and refine rule; fp16 weights and launchers; the fused stem and the
// split form behind switches of their own (y3_net_set_stem_fusion_f16, y3_net_set_low_latency_f16 / _split_k_f16), off by default
constexpr y3::ConvFamily F16_FAMILY = {
    y3::BF16_TILE_COUNT, y3::conv_bf16_tile_info, y3::conv_bf16_tile_built, &ConvSlot::tile_bf16, &ConvSlot::cout_pad,
    BF16_FAMILY.bad, BF16_FAMILY.retired, BF16_FAMILY.misfit, 32, resident_rule_bf16,
    &ConvSlot::wf16_dev, 2, choose_tile_bf16, y3::launch_conv_f16, refine_bf16, y3::launch_conv_stem_f16, &ConvSlot::w0norm_dev, &ConvSlot::scale0norm_dev,
    &y3_net::stem_mode_f16, &F16_SPLIT, y3::launch_conv_tiny_stem_f16, &ConvSlot::w1tiny_f16_dev};
constexpr y3::ConvFamily X3_FAMILY = {
    y3::X3_TILE_COUNT, y3::conv_x3_tile_info, y3::conv_x3_tile_built, &ConvSlot::tile_x3, &ConvSlot::cout_pad64,
    "y3_net_set_tile_x3: bad argument", "y3_net_set_tile_x3: bad argument", "y3_net_set_tile_x3: tile does not fit this conv", -1, nullptr,
    &ConvSlot::wx3_dev, 6, choose_tile_x3, y3::launch_conv_f32x3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
constexpr y3::ConvFamily X2_FAMILY = {
    y3::X3_TILE_COUNT, y3::conv_x3_tile_info, y3::conv_x2_tile_built, &ConvSlot::tile_x2, &ConvSlot::cout_pad64,
    "y3_net_set_tile_x2: bad argument", "y3_net_set_tile_x2: tile does not fit this conv", "y3_net_set_tile_x2: tile does not fit this conv", -1, nullptr,
    &ConvSlot::wx2_dev, 4, choose_tile_x2, y3::launch_conv_f32x2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

// int8 plans (Y3_DTYPE_I8): the convs from the cut on (y3_plan.cpp, resolve_i8).  The bf16 family's tile ids and forced-tile field (a
// forced tile without an int8 form, or one that does not fit, leaves the conv to the chooser), the bf16 refine rule, int8 weights over Cout
// padded to 64; the fused stem is the fp16 plans' (it runs before the cut, behind y3_net_set_stem_fusion_f16); the split form behind
// switches of its own (y3_net_set_low_latency_i8 / _split_k_i8), off by default.
constexpr y3::ConvFamily I8_FAMILY = {
    y3::BF16_TILE_COUNT, y3::conv_i8_tile_info, y3::conv_i8_tile_built, &ConvSlot::tile_bf16, &ConvSlot::cout_pad64,
    BF16_FAMILY.bad, BF16_FAMILY.retired, BF16_FAMILY.misfit, -1, nullptr,
    &ConvSlot::wi8_dev, 1, choose_tile_i8, y3::launch_conv_i8, refine_bf16, y3::launch_conv_stem_f16, &ConvSlot::w0norm_dev, &ConvSlot::scale0norm_dev,
    &y3_net::stem_mode_f16, &I8_SPLIT, nullptr, nullptr};

// "forced tile, else the family's chooser": the tile part of the launch decision.  (A forced tile was checked by its setter against the
// family it was forced for; an int8 plan shares the bf16 field, so the check is made again here.)
int family_tile(const y3::ConvFamily &f, const ConvSlot &c, long long M, long long M_plan, bool arena_out)
{
    const int t = c.*f.tile;
    return t >= 0 && f.built(t) && fits(f.info(t), c, c.*f.cout_pad) ? t : f.choose(c, M, M_plan, arena_out);
}

}  // namespace

const y3::ConvFamily *y3::conv_family(int dtype)
{
    switch (dtype) {
        case Y3_DTYPE_F32: return &F32_FAMILY;
        case Y3_DTYPE_BF16: return &BF16_FAMILY;
        case Y3_DTYPE_F32X3: return &X3_FAMILY;
        case Y3_DTYPE_F32X2: return &X2_FAMILY;
        case Y3_DTYPE_F16: return &F16_FAMILY;
        case Y3_DTYPE_I8: return &I8_FAMILY;
        default: return nullptr;
    }
}

// Which kernel, with which tile, K order, XCD order and split, conv op oi launches for the rows of `a`.  Everything that asks this --
// the enqueue path, resolve_splits, the stamp and profile entry points -- asks it here.  Two rules hold throughout: the MFMA SHAPE
// follows the planned rows and the tile SIZE the rows of the call (choose_tile_bf16), and a split follows the plan alone
// (resolve_splits), so within one plan an image's bits depend neither on its batch nor on its lane.
y3::ConvChoice y3::choose_conv(const y3_net *net, int oi, const ConvArgs &a)
{
    const ConvSlot &c = net->convs[net->ops[oi].index];
    ConvChoice ch{ConvKind::Mfma, -1, 0, 0, 1, nullptr, -1};
    if (net->tiny_stem_fused && oi == 0) ch.kind = ConvKind::InTinyStem;
    else if (net->tiny_stem_fused && oi == 2) ch.kind = ConvKind::TinyStem;
    else if ((net->stem_fused && oi == 0) || (net->stem_conv2 && oi == 2)) ch.kind = ConvKind::InStem;
    else if (net->stem_fused && oi == 1) ch.kind = ConvKind::Stem;
    else if (c.first_layer) ch.kind = ConvKind::First;
    if (ch.kind != ConvKind::Mfma) return ch;
    const ConvFamily &f = family_of_conv(net, net->ops[oi].index);   // an int8 plan: fp16 before the cut, int8 from it on
    ch.tile = family_tile(f, c, a.M, (long long)net->max_batch * a.Ho * a.Wo, net->out_slot[c.d.dst] < 0);
    // tile -1: the mode has no tile for this conv.  y3_net_plan refuses such a net (conv_without_tile), so no planned net gets here; the
    // launchers answer a tile id out of range with hipErrorInvalidValue, and no refine rule is asked about a tile that does not exist
    if (ch.tile >= 0 && f.refine) f.refine(net, c, a, ch);
    return ch;
}

y3::ConvChoice y3::choose_conv_planned(const y3_net *net, int oi)
{
    const ConvSlot &c = net->convs[net->ops[oi].index];
    ConvArgs a{};
    a.Ho = net->height / c.d.out_div;
    a.Wo = net->width / c.d.out_div;
    a.M = net->max_batch * a.Ho * a.Wo;
    a.CoutPad = c.*family_of_conv(net, net->ops[oi].index).cout_pad;
    return choose_conv(net, oi, a);
}

int y3::conv_without_tile(const y3_net *net)
{
    for (int slot = 0; slot < (int)net->convs.size(); ++slot) {
        const ConvSlot &c = net->convs[slot];
        if (c.first_layer) continue;   // the direct Cin = 3 kernel (or the fused stem) in every mode
        if (net->tiny_stem_fused && slot == net->ops[2].index) continue;   // runs inside the fused tiny stem launch: it never asks a tile table
        const long long M = (long long)net->max_batch * (net->height / c.d.out_div) * (net->width / c.d.out_div);
        // whether a tile fits depends on the conv's widths alone, never on the rows: the planned batch answers for every call
        if (family_tile(family_of_conv(net, slot), c, M, M, net->out_slot[c.d.dst] < 0) < 0) return slot;
    }
    return -1;
}

int y3::conv_op(const y3_net *net, int slot)
{
    for (int oi = 0; oi < (int)net->ops.size(); ++oi)
        if (net->ops[oi].kind == 0 && net->ops[oi].index == slot) return oi;
    return -1;
}

// The one body of y3_net_set_tile / _bf16 / _x3 / _x2: a built id that fits the conv (-1: back to the tuning table / the heuristic)
static y3_status set_forced_tile(const y3::ConvFamily &f, y3_net *net, int slot, int tile)
{
    if (!net || slot < 0 || slot >= (int)net->convs.size() || tile >= f.count) return fail(Y3_ERR_INVALID, "%s", f.bad);
    ConvSlot &c = net->convs[slot];
    if (tile >= 0) {
        if (!f.built(tile)) return fail(Y3_ERR_INVALID, f.retired, tile);
        if (c.first_layer || !fits(f.info(tile), c, c.*f.cout_pad)) return fail(Y3_ERR_INVALID, "%s", f.misfit);
        if (tile == f.resident)
            if (y3_status st = f.resident_rule(net, c, slot); st != Y3_OK) return st;
    }
    c.*f.tile = tile;
    return Y3_OK;
}

// ---- split-K (low-latency fp32, bf16, fp16 and int8 plans) --------------------------------------------------------------------------------
// Can conv `slot` ever run split in the mode of `f` (which has a split form)?  From the graph and the forced tile alone (no plan needed):
// not the first layer, not a detection head (y3_net_detect runs the heads through conv_head.hip / decodes them in the launch, and the
// composed route must stay bit-identical to it), only on the tiles the split form is built for, and with a Cout the mode's finish launch
// can store.  why: the refusal's text.
static const char *const kNoTile = "no tile of this mode divides the conv's widths";   // compared by address in set_split_k
static bool split_eligible(const y3::ConvFamily &f, const y3_net *net, int slot, const char **why)
{
    const y3::SplitForm &sf = *f.split;
    const ConvSlot &c = net->convs[slot];
    const char *w = nullptr;
    // the conv's smallest tile; arena_out as the plan will have it (a conv writing an fp32 net output itself never takes bf16's tile 32)
    const bool arena_out = !is_output(net, c.d.dst) || y3::output_staged(net, c.d.dst);
    const int tile = c.first_layer ? -1 : family_tile(f, c, 1, 1, arena_out);
    if (c.first_layer) w = "the first layer (Cin = 3) is never split";
    else if (net->nclasses > 0 && is_output(net, c.d.dst)) w = "a detection-head conv is never split (y3_net_detect decodes it in its own launch)";
    else if (tile < 0) w = kNoTile;
    else if (!sf.tile(tile)) w = sf.no_form(tile);
    else if (c.d.cout % sf.cout_mult && arena_out) w = sf.bad_cout;
    if (why) *why = w;
    return !w;
}

// Decide ConvSlot::split_k of every conv and size the slab workspace.  Runs at the end of y3_net_plan_hw and again from every
// setter that changes an input of the decision on a planned net; never from the enqueue path.  Inputs: the conv's shape, its tile at
// the planned batch, max_batch, n_cus, the caller's request -- never the rows of a call, so within one plan an image's bits do not
// depend on its batch or position (the rule choose_tile_bf16 states for the MFMA shape).
y3_status y3::resolve_splits(y3_net *net)
{
    if (!net->height) return Y3_OK;
    size_t lane_bytes = 0;
    for (int oi = 0; oi < (int)net->ops.size(); ++oi) {
        if (net->ops[oi].kind != 0) continue;
        const int slot = net->ops[oi].index;
        ConvSlot &c = net->convs[slot];
        c.split_k = 1;
        // an int8 plan is mixed: its convs before the cut launch what an fp16 plan launches and stay unsplit under every switch (their K
        // is at most 9 tiles of 64, below the 16-bit floor); from the cut on the int8 family decides
        if (net->dtype == Y3_DTYPE_I8 && !conv_is_i8(net, slot)) continue;
        const ConvFamily &f = family_of_conv(net, slot);
        const int cout_pad = c.*f.cout_pad;
        // a mode with a split form splits by its own request and switch; the rule and its inputs are the same for all
        if (!f.split || !split_eligible(f, net, slot, nullptr)) continue;
        const SplitForm &sf = *f.split;
        const int req = c.*sf.req;
        if (req == 1 || (req < 0 && !(net->*sf.low_latency))) continue;
        const ConvChoice ch = choose_conv_planned(net, oi);   // the split in force is 1 here: the unsplit launch at the planned rows
        if (ch.kind != ConvKind::Mfma) continue;               // runs as, or inside, the fused stem launch
        if (!sf.tile(ch.tile)) continue;                       // the tile at the planned rows has no split form (bf16: 8 instead of 11 / 12)
        const long long M = (long long)net->max_batch * (net->height / c.d.out_div) * (net->width / c.d.out_div);
        const TileInfo t = f.info(ch.tile);
        const long long tiles = ((M + t.bm - 1) / t.bm) * (cout_pad / t.bn);
        const size_t slab = split_slab_bytes(t, M, cout_pad);
        const int kt = c.K / sf.bk;
        if (req < 0 && kt < sf.min_k_tiles) continue;          // the mode's floor (kSplitMinKTilesBf16 says why); a forced S is taken as given
        int S = req > 1 ? req : y3_choose_split_k(tiles, kt, net->n_cus, (long long)slab);
        if (S > kt) S = kt;
        if (S < 2 || slab > 0x7fffffffull) continue;
        c.split_k = S;
        lane_bytes = std::max(lane_bytes, (size_t)S * slab);
    }
    if (lane_bytes > net->split_ws_lane || (lane_bytes && net->lanes > net->split_ws_lanes)) {
        if (net->split_ws) (void)hipFree(net->split_ws);
        net->split_ws = nullptr;
        net->split_ws_lane = 0;
        net->split_ws_lanes = 0;
        lane_bytes = (lane_bytes + 255) & ~(size_t)255;
        hipError_t e = hipMalloc(&net->split_ws, lane_bytes * net->lanes);
        if (e != hipSuccess) {
            for (ConvSlot &c : net->convs) c.split_k = 1;
            return fail(Y3_ERR_OOM, "split-K workspace: hipMalloc(%zu) failed: %s", lane_bytes * net->lanes, hipGetErrorString(e));
        }
        net->split_ws_lane = lane_bytes;
        net->split_ws_lanes = net->lanes;
    }
    return Y3_OK;
}

// ... from a setter: nothing to decide before the first plan; afterwards on the net's device (the workspace may grow)
static y3_status resolve_splits_of_setter(y3_net *net)
{
    if (!net->height) return Y3_OK;
    Y3_ENTER_DEVICE(net);
    return y3::resolve_splits(net);
}

// The one body of y3_net_set_low_latency / _bf16 / _f16 / _i8.  was_set: the flag that records the call (fp32: the Y3_LOW_LATENCY override then stays out)
static y3_status set_low_latency(const y3::ConvFamily &f, y3_net *net, int on, bool y3_net::*was_set = nullptr)
{
    if (!net || on < 0 || on > 1) return fail(Y3_ERR_INVALID, "%s: argument must be 0 or 1", f.split->set_switch);
    net->*f.split->low_latency = on != 0;
    if (was_set) net->*was_set = true;
    return resolve_splits_of_setter(net);
}

// The one body of y3_net_set_split_k / _bf16 / _f16 / _i8: the request of the mode of `f`; a forced S only where the conv can take it
static y3_status set_split_k(const y3::ConvFamily &f, y3_net *net, int slot, int S)
{
    const y3::SplitForm &sf = *f.split;
    if (!net || slot < 0 || slot >= (int)net->convs.size() || S < -1 || S == 0 || S > 16)
        return fail(Y3_ERR_INVALID, "%s: conv slot out of range, or S not -1, 1 or 2..16", sf.set_split);
    ConvSlot &c = net->convs[slot];
    if (S > 1) {
        const char *why = nullptr;
        // a conv of the fused tiny stem first: its 32 -> 32 conv has no 16-bit tile, and the refusal should name the stem, not the tile table
        if (const int oi = y3::conv_op(net, slot); net->height && net->tiny_stem_fused && (oi == 0 || oi == 2))
            return fail(Y3_ERR_INVALID, "%s: conv %d runs inside the fused tiny stem kernel (y3_net_set_tiny_stem_fusion), which is never split", sf.set_split, slot);
        // (a conv that runs in another family in this plan -- another mode's plan, an int8 plan's convs before the cut, whose Cin the int8
        // tiles need not divide -- and has no tile in f for that reason is told so by the two checks below)
        if (!split_eligible(f, net, slot, &why) && !(why == kNoTile && net->height && &y3::family_of_conv(net, slot) != &f))
            return fail(Y3_ERR_INVALID, "%s: conv %d: %s", sf.set_split, slot, why);
        if (net->height && &y3::family_of(net) != &f) return fail(Y3_ERR_INVALID, "%s: conv %d: %s", sf.set_split, slot, sf.other_plan);
        if (net->height && &y3::family_of_conv(net, slot) != &f)   // an int8 plan's convs before the cut
            return fail(Y3_ERR_INVALID, "%s: conv %d runs in fp16 in this plan (it lies before the int8 cut, conv %d), and the fp16 convs of an int8 plan are never split",
                        sf.set_split, slot, net->i8_first_conv);
        if (const int oi = y3::conv_op(net, slot); net->height && oi >= 0) {
            const y3::ConvChoice ch = y3::choose_conv_planned(net, oi);   // .tile: the conv's tile at the planned rows, split or not
            if (ch.kind == y3::ConvKind::Stem || ch.kind == y3::ConvKind::InStem)
                return fail(Y3_ERR_INVALID, "%s: conv %d runs inside the fused stem kernel, which is never split", sf.set_split, slot);
            if (!sf.tile(ch.tile))
                return fail(Y3_ERR_INVALID, "%s: conv %d: its tile at the planned rows (%d) has no split form (%s)", sf.set_split, slot, ch.tile, sf.tiles);
        }
        if (S > c.K / sf.bk) return fail(Y3_ERR_INVALID, "%s: conv %d has %d K tiles, fewer than S = %d", sf.set_split, slot, c.K / sf.bk, S);
    }
    c.*sf.req = S;
    return resolve_splits_of_setter(net);
}

// y3_net_get_split_k / _bf16 / _f16 / _i8: the split in force when the net is planned in the mode of `f`, 1 otherwise
static int split_in_force(const y3::ConvFamily &f, const y3_net *net, int slot)
{
    if (!net || slot < 0 || slot >= (int)net->convs.size() || !net->height || &y3::family_of(net) != &f) return 1;
    return net->convs[slot].split_k;
}

extern "C" {

int y3_version(void) { return 100; }

const char *y3_last_error(void) { return g_err; }

int y3_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int y3_tile_built(int dtype, int tile)
{
    const y3::ConvFamily *f = y3::conv_family(dtype);
    return (f && f->built(tile)) ? 1 : 0;
}

int y3_choose_tile(int dtype, int size, int stride, int cin, int c0, int cout, long long M, long long M_plan, int arena_out)
{
    const y3::ConvFamily *f = y3::conv_family(dtype);
    // the shapes y3_net_create accepts for a conv that launches a tile (not the Cin = 3 first layer)
    if (!f || !(size == 1 || size == 3) || !(stride == 1 || (stride == 2 && size == 3)) || cin <= 0 || cin % 32 || cout <= 0 || M <= 0 || M_plan <= 0)
        return -2;
    if (c0 >= 0 && (size != 1 || c0 == 0 || c0 >= cin || c0 % 32)) return -2;
    ConvSlot c;   // as y3_net_create fills it; no forced tile, so family_tile asks the mode's chooser
    c.d.size = size;
    c.d.stride = stride;
    c.d.cin = cin;
    c.d.cout = cout;
    c.d.c0 = c0 >= 0 ? c0 : cin;
    c.d.src1 = c0 >= 0 ? 1 : -1;
    c.d.residual = -1;
    c.cout_pad = (cout + 31) / 32 * 32;
    c.cout_pad64 = (cout + 63) / 64 * 64;
    c.K = size * size * cin;
    return family_tile(*f, c, M, M_plan, arena_out != 0);
}

y3_status y3_net_create_heads(const y3_tensor_desc *tensors, int n_tensors, const int32_t *op_kinds, int n_ops,
                              const y3_conv_desc *convs, int n_convs, const y3_aux_desc *aux, int n_aux, int input_tensor,
                              const int32_t *outputs, int n_outputs, int nclasses, y3_net **out)
try {
    if (!tensors || !op_kinds || !convs || !outputs || !out || n_tensors <= 0 || n_ops <= 0 || n_convs < 0 || n_aux < 0)
        return fail(Y3_ERR_INVALID, "y3_net_create: null, empty or negative-count argument");
    if (n_outputs != 2 && n_outputs != 3) return fail(Y3_ERR_INVALID, "y3_net_create_heads: a net has 2 or 3 outputs (got %d)", n_outputs);
    if (y3::test_fail_alloc()) throw std::bad_alloc();   // tests only: the allocation below failing
    std::unique_ptr<y3_net> net(new y3_net());           // released to the caller on success only: no path leaks it, thrown ones included
    if (hipGetDevice(&net->device) != hipSuccess) return fail(Y3_ERR_NODEVICE, "y3_net_create: no HIP device");
    net->tensors.assign(tensors, tensors + n_tensors);
    net->aux.assign(aux, aux + (aux ? n_aux : 0));
    net->convs.resize(n_convs);
    auto bad_t = [&](int t) { return t < 0 || t >= n_tensors; };
    for (int i = 0; i < n_convs; ++i) {
        ConvSlot &c = net->convs[i];
        c.d = convs[i];
        const y3_conv_desc &d = c.d;
        int err = 0;
        if (bad_t(d.src0) || bad_t(d.dst) || (d.src1 >= 0 && bad_t(d.src1)) || (d.residual >= 0 && bad_t(d.residual))) err = 1;
        if (!(d.size == 1 || d.size == 3) || !(d.stride == 1 || (d.stride == 2 && d.size == 3))) err = 2;
        if (d.src1 >= 0 && (d.size != 1 || d.c0 % 32 || (d.cin - d.c0) % 32 || d.c0 <= 0 || d.c0 >= d.cin)) err = 3;
        if (d.src1 < 0 && (d.c0 != d.cin || d.src0_upsample)) err = 4;
        c.first_layer = (d.cin == 3);
        if (c.first_layer && !(d.size == 3 && d.stride == 1 && d.cout == 32 && d.residual < 0 && d.src1 < 0)) err = 5;
        if (!c.first_layer && d.cin % 32) err = 6;
        if (d.cout <= 0 || d.out_div != d.in_div * d.stride) err = err ? err : 7;
        if (err) {
            return fail(Y3_ERR_INVALID, "y3_net_create: conv %d unsupported or inconsistent (check %d)", i, err);
        }
        c.cout_pad = (d.cout + 31) / 32 * 32;
        c.cout_pad64 = (d.cout + 63) / 64 * 64;
        c.K = d.size * d.size * d.cin;
    }
    int ci = 0, ai = 0;
    for (int i = 0; i < n_ops; ++i) {
        if (op_kinds[i] == 0) {
            if (ci >= n_convs) { return fail(Y3_ERR_INVALID, "y3_net_create: more conv ops than descriptors"); }
            net->ops.push_back({0, ci++});
        } else {
            if (ai >= n_aux) { return fail(Y3_ERR_INVALID, "y3_net_create: more aux ops than descriptors"); }
            net->ops.push_back({1, ai++});
        }
    }
    if (bad_t(input_tensor)) { return fail(Y3_ERR_INVALID, "y3_net_create: bad input tensor"); }
    net->input_tensor = input_tensor;
    for (const y3_aux_desc &x : net->aux) {
        if (x.kind != Y3_AUX_MAXPOOL2X2_S2 && x.kind != Y3_AUX_MAXPOOL2X2_S1) continue;
        const int up = x.kind == Y3_AUX_MAXPOOL2X2_S2 ? 2 : 1;
        if (bad_t(x.src0) || bad_t(x.dst) || tensors[x.src0].channels % 32 || tensors[x.dst].channels != tensors[x.src0].channels ||
            tensors[x.dst].div != tensors[x.src0].div * up)
            return fail(Y3_ERR_INVALID, "y3_net_create: max-pool op (kind %d) needs a source of Cin %% 32 == 0 channels and a destination of "
                                        "the same width at %s", x.kind, up == 2 ? "twice the source's div" : "the source's div");
        net->has_pool = true;
    }
    net->n_heads = n_outputs;
    for (int i = 0; i < n_outputs; ++i) {
        // nclasses == 0: raw feature outputs (layer tests); otherwise the yolo head layout is enforced
        if (bad_t(outputs[i]) || (nclasses > 0 && tensors[outputs[i]].channels != 3 * (5 + nclasses))) {
            return fail(Y3_ERR_INVALID, "y3_net_create: output %d must have 3*(5+nclasses) channels", i);
        }
        net->outputs[i] = outputs[i];
    }
    net->nclasses = nclasses;
    net->tdev.assign(n_tensors, nullptr);
    net->tbytes.assign(n_tensors, 0);
    net->tblock.assign(n_tensors, 0);
    net->out_slot.assign(n_tensors, -1);
    *out = net.release();
    return Y3_OK;
}
Y3_CATCH("y3_net_create_heads")

y3_status y3_net_create(const y3_tensor_desc *tensors, int n_tensors, const int32_t *op_kinds, int n_ops,
                        const y3_conv_desc *convs, int n_convs, const y3_aux_desc *aux, int n_aux, int input_tensor,
                        const int32_t outputs[3], int nclasses, y3_net **out)
try {
    return y3_net_create_heads(tensors, n_tensors, op_kinds, n_ops, convs, n_convs, aux, n_aux, input_tensor, outputs, 3, nclasses, out);
}
Y3_CATCH("y3_net_create")

int y3_net_heads(const y3_net *net) { return net ? net->n_heads : 0; }

void y3_net_destroy(y3_net *net)
{
    if (!net) return;
    y3::free_plan(net);
    if (net->fork_ev) {
        (void)hipEventDestroy(net->fork_ev);
        for (int i = 0; i < Y3_MAX_LANES; ++i) {
            (void)hipStreamDestroy(net->lane_stream[i]);
            (void)hipEventDestroy(net->join_ev[i]);
        }
    }
    for (ConvSlot &c : net->convs)
        for (void *p : {c.w_dev, (void *)c.w0stem_dev, (void *)c.w0raw_dev, (void *)c.w0norm_dev, (void *)c.scale0norm_dev, c.wbf_dev, c.wf16_dev, c.wx3_dev, c.wx2_dev, (void *)c.scale_x2_dev, (void *)c.scale_dev, (void *)c.shift_dev, c.wi8_dev, (void *)c.sc_i8_dev, (void *)c.w0tiny_dev, c.w1tiny_dev, c.w1tiny_bf_dev, c.w1tiny_f16_dev})
            if (p) (void)hipFree(p);
    delete net;
}

y3_status y3_net_set_conv_weights(y3_net *net, int slot, const float *w, const float *gamma, const float *beta,
                                  const float *mean, const float *var, const float *bias, float eps)
try {
    if (!net || slot < 0 || slot >= (int)net->convs.size() || !w)
        return fail(Y3_ERR_INVALID, "y3_net_set_conv_weights: bad slot or null weights");
    ConvSlot &c = net->convs[slot];
    const y3_conv_desc &d = c.d;
    if (d.bn ? !(gamma && beta && mean && var) : !bias)
        return fail(Y3_ERR_INVALID, "y3_net_set_conv_weights: conv %d needs %s", slot, d.bn ? "gamma/beta/mean/var" : "bias");
    const int K = c.K, CP = c.cout_pad, CP64 = c.cout_pad64;
    std::vector<float> scale(CP64, 1.0f), shift(CP64, 0.0f);
    for (int n = 0; n < d.cout; ++n) {
        if (d.bn) {
            // BatchNormalization inference: y = x*scale + (beta - mean*scale), scale = gamma*rsqrt(var+eps)
            const float inv = 1.0f / sqrtf(var[n] + eps);
            scale[n] = inv * gamma[n];
            shift[n] = beta[n] - mean[n] * scale[n];
        } else {
            shift[n] = bias[n];
        }
    }
    Y3_ENTER_DEVICE(net);
    // every format is packed whatever the plan's dtype: one net can be re-planned in another mode
    if (c.first_layer) {
        // HWIO as is (the Cin = 3 direct kernels); the fused stem kernel's 28 rows with the BN scale folded in (fp32) and without (bf16)
        HIP_TRY(upload(c.w_dev, std::vector<float>(w, w + (size_t)K * d.cout)));
        HIP_TRY(upload(c.w0stem_dev, pack_stem28(w, K, d.cout, scale.data())));
        HIP_TRY(upload(c.w0raw_dev, pack_stem28(w, K, d.cout, nullptr)));
        // ... and normalised per output channel by a power of two, with the scale that undoes it (fp16)
        std::vector<int> exps;
        HIP_TRY(upload(c.w0norm_dev, pack_stem28_norm(w, K, d.cout, exps)));
        std::vector<float> scale_norm(scale.begin(), scale.begin() + d.cout);
        for (int n = 0; n < d.cout; ++n) scale_norm[n] = ldexpf(scale_norm[n], exps[n]);
        HIP_TRY(upload(c.scale0norm_dev, scale_norm));
        // the fused tiny stem's copy at the real width 16: the HWIO rows of output channels 0..15 (unscaled; scale_dev / shift_dev begin with
        // their scale and shift), and whether channels 16..31 are the lowering's zero pad channels
        std::vector<float> w16((size_t)K * 16);
        for (int k = 0; k < K; ++k)
            for (int n = 0; n < 16; ++n) w16[(size_t)k * 16 + n] = w[(size_t)k * d.cout + n];
        HIP_TRY(upload(c.w0tiny_dev, w16));
        c.tiny_pad_zero = true;
        for (int n = 16; n < d.cout; ++n) c.tiny_pad_zero = c.tiny_pad_zero && scale[n] == 0.0f && shift[n] == 0.0f;
    } else {
        // fp32 path: the BN scale is folded into the packed weights (one VALU multiply less per output element; VALU
        // time is matrix-pipe time for the fp32 MFMA).  The bf16 copy keeps the unscaled weights + scale in the epilogue.
        const std::vector<float> pk = pack_rows(w, K, d.cout, CP, nullptr), pk_scaled = pack_rows(w, K, d.cout, CP, scale.data());
        HIP_TRY(upload(c.w_dev, pk_scaled));
        HIP_TRY(upload(c.wbf_dev, pack_planes<1>(pk, K, d.cout, CP, [](float x, unsigned short *v) { v[0] = f32_to_bf16_rne(x); })));
        // the fp16 copy, packed like the bf16 one (unscaled, round to nearest even; |w| beyond the fp16 range becomes inf, as IEEE says)
        HIP_TRY(upload(c.wf16_dev, pack_planes<1>(pk, K, d.cout, CP, [](float x, unsigned short *v) { v[0] = f32_to_f16_rne(x); })));
        // a scaled weight outside the fp16 range: y3_net_plan(Y3_DTYPE_F32X2) refuses the net; other modes are unaffected.  The planes below are
        // normalised into [1, 2) per channel, so fp16 could represent such weights: the refusal is kept as the mode's stated contract (a channel
        // whose scaled weights reach 65504 leaves the fp16 range of its activation planes for inputs of order 1), not as a representability bound of the packing
        c.x2_ok = std::all_of(pk_scaled.begin(), pk_scaled.end(), [](float x) { return fabsf(x) < 65504.0f; });
        HIP_TRY(upload(c.wx3_dev, pack_planes<3>(pk, K, d.cout, CP64, split_bf16x3)));         // unscaled, like the bf16 copy
        // BN-scaled, like the fp32 copy, and normalised per output channel by a power of two that the epilogue puts back
        std::vector<float> pow2(CP64, 1.0f);
        HIP_TRY(upload(c.wx2_dev, pack_planes<2>(normalise_rows(pk_scaled, K, d.cout, pow2), K, d.cout, CP64, split_f16x2)));
        HIP_TRY(upload(c.scale_x2_dev, pow2));
        // the int8 copy: the raw weights quantised per output channel (BN stays in the epilogue); their scales stay on the host for the plan
        HIP_TRY(upload(c.wi8_dev, pack_i8(pk, K, d.cout, CP64, c.sw_host)));
        c.bn_scale_host = scale;
        if (d.size == 3 && d.stride == 1 && d.cin == 32 && d.cout == 32 && d.src1 < 0) {
            // the fused tiny stem's copies at the real input width 16: [144][32], row tap * 16 + c from input channels c < 16, unscaled
            std::vector<float> t32((size_t)144 * 32);
            for (int tap = 0; tap < 9; ++tap)
                for (int ch = 0; ch < 16; ++ch)
                    for (int n = 0; n < 32; ++n) t32[((size_t)tap * 16 + ch) * 32 + n] = w[((size_t)tap * 32 + ch) * 32 + n];
            std::vector<unsigned short> tb(t32.size()), th(t32.size());
            for (size_t i = 0; i < t32.size(); ++i) {
                tb[i] = f32_to_bf16_rne(t32[i]);
                th[i] = f32_to_f16_rne(t32[i]);
            }
            HIP_TRY(upload(c.w1tiny_dev, t32));
            HIP_TRY(upload(c.w1tiny_bf_dev, tb));
            HIP_TRY(upload(c.w1tiny_f16_dev, th));
        }
    }
    HIP_TRY(upload(c.scale_dev, scale));
    HIP_TRY(upload(c.shift_dev, shift));
    c.loaded = true;
    if (y3::conv_is_i8(net, slot)) return y3::upload_i8_scales(net, slot);   // a planned int8 net: this conv's epilogue scales follow its weights
    return Y3_OK;
}
Y3_CATCH("y3_net_set_conv_weights")

y3_status y3_net_set_tile(y3_net *net, int slot, int tile)
try {
    if (y3_status st = set_forced_tile(F32_FAMILY, net, slot, tile); st != Y3_OK) return st;
    return resolve_splits_of_setter(net);   // the tile is an input of the split decision
}
Y3_CATCH("y3_net_set_tile")

y3_status y3_net_set_tile_bf16(y3_net *net, int slot, int tile)
try {
    if (y3_status st = set_forced_tile(BF16_FAMILY, net, slot, tile); st != Y3_OK) return st;
    return resolve_splits_of_setter(net);   // the tile is an input of the split decision
}
Y3_CATCH("y3_net_set_tile_bf16")

y3_status y3_net_set_tile_x3(y3_net *net, int slot, int tile)
try { return set_forced_tile(X3_FAMILY, net, slot, tile); }
Y3_CATCH("y3_net_set_tile_x3")

y3_status y3_net_set_tile_x2(y3_net *net, int slot, int tile)
try { return set_forced_tile(X2_FAMILY, net, slot, tile); }
Y3_CATCH("y3_net_set_tile_x2")

y3_status y3_net_set_lanes(y3_net *net, int lanes)
try {
    if (!net || lanes < 1 || lanes > Y3_MAX_LANES) return fail(Y3_ERR_INVALID, "y3_net_set_lanes: lanes must be in [1,%d]", Y3_MAX_LANES);
    net->lanes = lanes;
    return resolve_splits_of_setter(net);   // one slab workspace per lane
}
Y3_CATCH("y3_net_set_lanes")

// The one body of y3_net_set_stem_fusion / _f16: the switch `mode` of the plans it acts on
static y3_status set_stem_fusion(const char *who, y3_net *net, int y3_net::*mode, int on)
{
    if (!net || on < 0 || on > 2) return fail(Y3_ERR_INVALID, "%s: argument must be 0, 1 or 2", who);
    net->*mode = on;
    // takes effect at once on a planned net of the switch's mode when the graph qualifies (decided again by the next y3_net_plan)
    if (net->height) y3::resolve_stem(net);
    return resolve_splits_of_setter(net);   // a conv inside the fused stem is not split
}

y3_status y3_net_set_stem_fusion(y3_net *net, int on)
try {
    const y3_status st = set_stem_fusion("y3_net_set_stem_fusion", net, &y3_net::stem_mode, on);
    if (st == Y3_OK) net->stem_mode_set = true;
    return st;
}
Y3_CATCH("y3_net_set_stem_fusion")

y3_status y3_net_set_stem_fusion_f16(y3_net *net, int on)
try { return set_stem_fusion("y3_net_set_stem_fusion_f16", net, &y3_net::stem_mode_f16, on); }
Y3_CATCH("y3_net_set_stem_fusion_f16")

y3_status y3_net_set_tiny_stem_fusion(y3_net *net, int on)
try {
    if (!net || on < 0 || on > 1) return fail(Y3_ERR_INVALID, "y3_net_set_tiny_stem_fusion: argument must be 0 or 1");
    net->tiny_stem_mode = on;   // read by the next y3_net_plan: the arena is placed by it
    return Y3_OK;
}
Y3_CATCH("y3_net_set_tiny_stem_fusion")

int y3_net_get_tiny_stem_fused(const y3_net *net) { return net && net->height && net->tiny_stem_fused ? 1 : 0; }

y3_status y3_net_set_pools_i8(y3_net *net, int on)
try {
    if (!net || on < 0 || on > 1) return fail(Y3_ERR_INVALID, "y3_net_set_pools_i8: argument must be 0 or 1");
    net->pools_i8_mode = on;   // read by the next y3_net_plan: the element size of the arena's tensors follows it
    return Y3_OK;
}
Y3_CATCH("y3_net_set_pools_i8")

int y3_net_pools_i8(const y3_net *net)
{
    if (!net || !net->height || net->dtype != Y3_DTYPE_I8) return 0;
    for (char on : net->aux_i8)
        if (on) return 1;
    return 0;
}

y3_status y3_net_set_k_chunk(y3_net *net, int channels)
try {
    if (!net || channels < -1 || (channels > 0 && channels % 32)) return fail(Y3_ERR_INVALID, "y3_net_set_k_chunk: -1, 0 or a multiple of 32 channels");
    net->k_chunk = channels;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_k_chunk")

y3_status y3_net_set_border_skip(y3_net *net, int mode)
try {
    if (!net || mode < -1 || mode > 1) return fail(Y3_ERR_INVALID, "y3_net_set_border_skip: -1 (the rule), 0 (off) or 1 (on wherever legal)");
    net->border_skip = mode;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_border_skip")

int y3_net_get_border_skip(const y3_net *net, int slot, int batch)
{
    if (!net || !net->height || slot < 0 || slot >= (int)net->convs.size() || batch <= 0 || batch > net->max_batch) return 0;
    const int oi = y3::conv_op(net, slot);
    if (oi < 0) return 0;
    const ConvSlot &c = net->convs[slot];
    int lanes = net->lanes, n = 0;
    while (lanes > 1 && batch / lanes < 1) --lanes;
    for (int l = 0; l < lanes; ++l) {   // the sub-batches of y3_net_forward; a conv of the chunked leading segment: its first chunk
        int nb = (int)((long long)batch * (l + 1) / lanes) - (int)((long long)batch * l / lanes);
        if (oi < net->early_ops && nb > net->early_step) nb = net->early_step;
        if (nb <= 0) continue;
        y3::ConvArgs a{};
        a.B = nb;
        a.Ho = net->height / c.d.out_div;
        a.Wo = net->width / c.d.out_div;
        a.M = nb * a.Ho * a.Wo;
        a.Cout = c.d.cout;
        a.CoutPad = c.*y3::family_of_conv(net, slot).cout_pad;
        n += y3::choose_conv(net, oi, a).pos_tab != nullptr;
    }
    return n;
}

y3_status y3_net_set_low_latency(y3_net *net, int on)
try { return set_low_latency(F32_FAMILY, net, on, &y3_net::low_latency_set); }
Y3_CATCH("y3_net_set_low_latency")

y3_status y3_net_set_split_k(y3_net *net, int slot, int S)
try { return set_split_k(F32_FAMILY, net, slot, S); }
Y3_CATCH("y3_net_set_split_k")

y3_status y3_net_set_low_latency_bf16(y3_net *net, int on)
try { return set_low_latency(BF16_FAMILY, net, on); }
Y3_CATCH("y3_net_set_low_latency_bf16")

y3_status y3_net_set_split_k_bf16(y3_net *net, int slot, int S)
try { return set_split_k(BF16_FAMILY, net, slot, S); }
Y3_CATCH("y3_net_set_split_k_bf16")

y3_status y3_net_set_low_latency_f16(y3_net *net, int on)
try { return set_low_latency(F16_FAMILY, net, on); }
Y3_CATCH("y3_net_set_low_latency_f16")

y3_status y3_net_set_split_k_f16(y3_net *net, int slot, int S)
try { return set_split_k(F16_FAMILY, net, slot, S); }
Y3_CATCH("y3_net_set_split_k_f16")

y3_status y3_net_set_low_latency_i8(y3_net *net, int on)
try { return set_low_latency(I8_FAMILY, net, on); }
Y3_CATCH("y3_net_set_low_latency_i8")

y3_status y3_net_set_split_k_i8(y3_net *net, int slot, int S)
try { return set_split_k(I8_FAMILY, net, slot, S); }
Y3_CATCH("y3_net_set_split_k_i8")

y3_status y3_net_set_xcd_mode(y3_net *net, int mode)
try {
    if (!net || mode < 0 || mode > 1) return fail(Y3_ERR_INVALID, "y3_net_set_xcd_mode: mode must be 0 or 1");
    net->xcd_mode = mode;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_xcd_mode")

y3_status y3_net_set_nms_mode(y3_net *net, int mode)
try {
    if (!net || (mode != Y3_NMS_AGNOSTIC && mode != Y3_NMS_PER_CLASS))
        return fail(Y3_ERR_INVALID, "y3_net_set_nms_mode: mode must be Y3_NMS_AGNOSTIC (0) or Y3_NMS_PER_CLASS (1)");
    net->nms_mode = mode;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_nms_mode")

int y3_net_get_nms_mode(const y3_net *net) { return net ? net->nms_mode : Y3_NMS_AGNOSTIC; }

y3_status y3_net_set_multi_label(y3_net *net, int on, int capacity)
try {
    if (!net || capacity < 0)
        return fail(Y3_ERR_INVALID, "y3_net_set_multi_label: null net or capacity < 0 (0: N of the plan; otherwise 1 <= capacity <= N, checked when y3_net_detect enqueues)");
    net->multi_label = on != 0;
    net->multi_label_capacity = capacity;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_multi_label")

int y3_net_get_multi_label(const y3_net *net) { return net ? net->multi_label : 0; }
int y3_net_get_multi_label_capacity(const y3_net *net) { return net ? net->multi_label_capacity : 0; }

y3_status y3_net_read_multi_label_totals(y3_net *net, int batch, int32_t *dst_dev, void *stream)
try {
    if (!net || !dst_dev || batch < 1) return fail(Y3_ERR_INVALID, "y3_net_read_multi_label_totals: bad argument");
    if (!net->height || net->nclasses <= 0 || net->multi_label_batch < 1)
        return fail(Y3_ERR_STATE, "y3_net_read_multi_label_totals: no multi-label y3_net_detect was enqueued on this plan");
    if (batch > net->max_batch) return fail(Y3_ERR_INVALID, "y3_net_read_multi_label_totals: batch %d > planned %d", batch, net->max_batch);
    const y3::DetectLayout L = y3::detect_layout(net, net->multi_label_batch);
    if (!net->det_buf || net->det_bytes < L.total)
        return fail(Y3_ERR_STATE, "y3_net_read_multi_label_totals: detect scratch not planned (y3_net_plan allocates it)");
    Y3_ENTER_DEVICE(net);
    const int have = batch < net->multi_label_batch ? batch : net->multi_label_batch;   // images that detect did not have read 0
    HIP_TRY(hipMemcpyAsync(dst_dev, static_cast<char *>(net->det_buf) + L.totals, (size_t)have * sizeof(int32_t), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    if (batch > have) HIP_TRY(hipMemsetAsync(dst_dev + have, 0, (size_t)(batch - have) * sizeof(int32_t), (hipStream_t)stream));
    return Y3_OK;
}
Y3_CATCH("y3_net_read_multi_label_totals")

y3_status y3_net_set_early_chunk(y3_net *net, int n_convs, int chunk_images)
try {
    if (!net || n_convs < 0 || chunk_images < 0) return fail(Y3_ERR_INVALID, "y3_net_set_early_chunk: bad argument");
    if (n_convs >= (int)net->convs.size()) return fail(Y3_ERR_INVALID, "y3_net_set_early_chunk: n_convs must leave at least one conv for the full batch");
    net->early_convs = (chunk_images > 0) ? n_convs : 0;
    net->early_chunk = (n_convs > 0) ? chunk_images : 0;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_early_chunk")

y3_status y3_net_keep_activations(y3_net *net, int keep)
try {
    if (!net) return fail(Y3_ERR_INVALID, "y3_net_keep_activations: null net");
    net->keep_all = keep ? 1 : 0;
    return Y3_OK;
}
Y3_CATCH("y3_net_keep_activations")

y3_status y3_net_set_act_scales(y3_net *net, const float *scales, int n_tensors)
try {
    if (!net || !scales) return fail(Y3_ERR_INVALID, "y3_net_set_act_scales: null argument");
    if (n_tensors != (int)net->tensors.size())
        return fail(Y3_ERR_INVALID, "y3_net_set_act_scales: %d scales for a net of %zu tensors", n_tensors, net->tensors.size());
    for (int t = 0; t < n_tensors; ++t)
        if (scales[t] > 0.0f && !std::isfinite(scales[t])) return fail(Y3_ERR_INVALID, "y3_net_set_act_scales: the scale of tensor %d is not finite", t);
    net->act_scale.assign(scales, scales + n_tensors);
    return Y3_OK;
}
Y3_CATCH("y3_net_set_act_scales")

float y3_net_get_act_scale(const y3_net *net, int tensor_id)
{
    if (!net || tensor_id < 0 || tensor_id >= (int)net->act_scale.size() || !(net->act_scale[tensor_id] > 0.0f)) return 0.0f;
    return net->act_scale[tensor_id];
}

int y3_net_i8_first_conv(const y3_net *net) { return (net && net->height && net->dtype == Y3_DTYPE_I8) ? net->i8_first_conv : -1; }

int y3_net_get_split_k(const y3_net *net, int slot) { return split_in_force(F32_FAMILY, net, slot); }

int y3_net_get_split_k_bf16(const y3_net *net, int slot) { return split_in_force(BF16_FAMILY, net, slot); }

int y3_net_get_split_k_f16(const y3_net *net, int slot) { return split_in_force(F16_FAMILY, net, slot); }

int y3_net_get_split_k_i8(const y3_net *net, int slot) { return split_in_force(I8_FAMILY, net, slot); }

int y3_choose_split_k(long long tiles, int k_tiles, int n_cus, long long slab_bytes_per_slice)
{
    // Below two workgroups per CU the wall time of a conv launch is one workgroup's walk through K (the 13^2 512 -> 1024 conv at
    // one image: 48 workgroups x 144 K tiles on 256 CUs), so slices multiply the workgroups until the chip holds two per CU -- but a
    // slice keeps at least kSplitMinTiles K tiles (its prologue and its slab store are paid per slice), at most kSplitMax slices
    // exist, and the slabs of one launch stay under kSplitMaxBytes (they are written and read once more by the finish launch).
    constexpr int kSplitMinTiles = 4, kSplitMax = 16;
    constexpr long long kSplitMaxBytes = 16ll << 20;
    if (tiles <= 0 || k_tiles <= 0 || n_cus <= 0 || slab_bytes_per_slice <= 0) return 1;
    const long long want = 2ll * n_cus;
    if (tiles >= want) return 1;
    long long S = (want + tiles - 1) / tiles;
    S = std::min<long long>(S, k_tiles / kSplitMinTiles);
    S = std::min<long long>(S, kSplitMax);
    S = std::min<long long>(S, kSplitMaxBytes / slab_bytes_per_slice);
    return S < 2 ? 1 : (int)S;
}

int y3_persistent_grid(int kind, long long n_tiles, int slices, int n_cus)
{
    // the launchers' own formulas (y3_kernels.h); what they refuse or never see is refused here: no tiles, more than an int of them,
    // slices on a kernel that has none
    if (n_tiles <= 0 || n_tiles > 0x7fffffffll || slices <= 0 || n_cus <= 0) return 0;
    switch (kind) {
        case Y3_PERSISTENT_TINY_STEM: return slices == 1 ? y3::persistent_stem_grid(n_tiles, y3::kTinyStemWgPerCu, n_cus) : 0;
        case Y3_PERSISTENT_STEM_F32: return slices == 1 ? y3::persistent_stem_grid(n_tiles, y3::kStemWgPerCuF32, n_cus) : 0;
        case Y3_PERSISTENT_STEM_16: return slices == 1 ? y3::persistent_stem_grid(n_tiles, y3::kStemWgPerCu16, n_cus) : 0;
        case Y3_PERSISTENT_RES_F32:
        case Y3_PERSISTENT_RES_16: return y3::persistent_res_per_slice(n_tiles, slices, n_cus) * slices;
        default: return 0;
    }
}

}  // extern "C"
