// C-ABI layer of liby3hip.so: network object (fused conv program), weight packing, activation arena,
// and the decode / NMS entry points.  See include/y3.h for the contract each function implements and
// the reference interface it replaces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <vector>

#include "../../include/y3.h"
#include "y3_kernels.h"

namespace {

// The last error of this thread: a fixed buffer, so that reporting a failure allocates nothing and cannot itself throw
// (include/y3.h: no entry point throws or aborts -- not even while it reports that the host ran out of memory).
thread_local char g_err[512] = "";

}  // namespace

namespace y3 {
// record the message as this thread's last error and return `code` (here and in the other translation units: comm.cpp)
int fail_msg(int code, const char *fmt, ...) noexcept
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// The exception barrier of the C ABI.  Every extern "C" entry point that can reach an allocation (std::vector, new, std::string)
// is a function-try-block ending in Y3_CATCH: a C++ exception becomes a status + message instead of crossing the boundary and
// terminating the host process (a ctypes / cgo / JNI caller has no handler for it).
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

// Test hook (tests/test_abi.py): Y3_TEST_FAIL_ALLOC=1 makes the object allocations of y3_net_create / y3_comm_init_rank fail the
// way operator new does; read on every call so that a test can switch it on and off inside one process.
bool test_fail_alloc() noexcept
{
    const char *e = getenv("Y3_TEST_FAIL_ALLOC");
    return e && e[0] == '1';
}

// include/y3.h, Y3_IMAGE_LETTERBOX.  Every operation in fp32 (this file is compiled with -ffp-contract=off), nearbyintf in the
// default rounding mode (half to even): bit for bit what core/utils.letterbox_geometry computes with np.float32 and np.rint.
LetterboxGeom letterbox_geom(int h, int w, int Hc, int Wc)
{
    const float scale = std::min((float)Hc / (float)h, (float)Wc / (float)w);
    LetterboxGeom g;
    g.sh = std::max(1, (int)nearbyintf(scale * (float)h));
    g.sw = std::max(1, (int)nearbyintf(scale * (float)w));
    g.top = (Hc - g.sh) >> 1;      // floor, also where the difference is negative (refused by letterbox_geom_fits)
    g.left = (Wc - g.sw) >> 1;
    return g;
}
}  // namespace y3

#define Y3_CATCH(who) catch (...) { return y3::on_exception(who); }

namespace {

constexpr auto fail = y3::fail_msg;

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? Y3_ERR_OOM : Y3_ERR_HIP, "%s: %s", #expr,     \
                        hipGetErrorString(e_));                                                   \
    } while (0)

// Enter the net's device for the duration of a call and give the caller its own current device back on every return path (a
// process driving several GPUs -- PyTorch with nets on different devices -- must not find its current device changed).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev); else if (err == hipSuccess) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define Y3_ENTER_DEVICE(net_)                                                                      \
    DeviceGuard dev_guard_((net_)->device);                                                        \
    if (dev_guard_.err != hipSuccess) return fail(Y3_ERR_HIP, "hipSetDevice(%d): %s", (net_)->device, hipGetErrorString(dev_guard_.err))

struct ConvSlot {
    y3_conv_desc d{};
    bool loaded = false;
    bool first_layer = false;  // Cin == 3 direct kernel
    int cout_pad = 0;
    int K = 0;
    int tile = -1;             // -1: choose by heuristic at plan time
    int split_req = -1;        // y3_net_set_split_k: -1 the heuristic (low-latency plans only), 1 off, 2..16 forced
    int split_k = 1;           // K slices in force, decided by resolve_splits from plan-time quantities only (1: the unsplit launch)
    int tile_bf16 = -1;
    int tile_x3 = -1;
    int cout_pad64 = 0;        // Cout rounded up to 64 (the three-plane kernel has no 32-wide N tile)
    void *wx3_dev = nullptr;   // packed [CoutPad64][3 planes][K] bf16 (hi, mid, lo of the fp32 weights)
    int tile_x2 = -1;
    bool x2_ok = true;         // false: a BN-scaled weight is outside the fp16 range, the two-plane mode cannot be planned
    void *wx2_dev = nullptr;   // packed [CoutPad64][2 planes][K] fp16 (h, l' = (w - h) * 2^11 of the BN-scaled weights)
    float *w_dev = nullptr;    // packed [CoutPad][K] (or HWIO for the first layer)
    float *w0stem_dev = nullptr;   // first layer only: [28][Cout] = HWIO rows x BN scale, row 27 zero (fused stem kernel, fp32)
    float *w0raw_dev = nullptr;    // first layer only: the same without the scale (fused stem kernel, bf16 mode)
    void *wbf_dev = nullptr;   // same, bf16 (not for the first layer)
    float *scale_dev = nullptr;
    float *shift_dev = nullptr;
};

struct Op {
    int kind;  // 0 conv, 1 aux
    int index;
};

constexpr int Y3_MAX_LANES = 4;
constexpr int Y3_MAX_OUTPUT_BOXES = 1024;   // upper bound of max_output_size (y3_nms_padded) the detect scratch is sized for

}  // namespace

struct y3_net {
    int device = 0;
    int n_cus = 0;                 // compute units of `device`, read once by y3_net_plan (grids of the persistent kernels)
    std::vector<y3_tensor_desc> tensors;
    std::vector<Op> ops;
    std::vector<ConvSlot> convs;
    std::vector<y3_aux_desc> aux;
    int input_tensor = 0;
    int outputs[3] = {0, 0, 0};
    int nclasses = 0;
    // plan
    int max_batch = 0, height = 0, width = 0, dtype = Y3_DTYPE_F32;   // the planned canvas: height x width (0: no plan)
    int keep_all = 0;              // 1: no buffer reuse, every intermediate stays readable after a forward
    int lanes = 1;                 // sub-batches run concurrently on forked streams (y3_net_set_lanes)
    int early_convs = 0;           // y3_net_set_early_chunk: the first early_convs convs run early_chunk images at a time
    int early_chunk = 0;
    int early_ops = 0;             // (at plan time) number of leading ops that form the chunked segment
    std::vector<char> dense;       // tensor written by the chunked segment: own block, image i at i * image_bytes
    // (non-fp32 modes) output tensors that another op reads, or that a residual / first-layer conv writes: produced in
    // the arena in the mode's own format and converted into the caller's fp32 buffer at the end of the forward
    std::vector<char> staged;
    // y3_net_detect scratch (grids, decoded boxes / classes / scores, selected indices, NMS workspace): allocated by
    // y3_net_plan for max_batch images and Y3_MAX_OUTPUT_BOXES rows, so y3_net_detect itself only enqueues work
    void *det_buf = nullptr;
    size_t det_bytes = 0;
    int stem_mode = 1;             // y3_net_set_stem_fusion: 1 = conv0 + conv1 (+ the 1x1 after them) as one kernel when the graph allows it; 2 = conv0 + conv1 only
    bool stem_mode_set = false;    // y3_net_set_stem_fusion was called (the Y3_STEM_MODE tool override then stays out)
    bool stem_fused = false;       // (at plan time) the first two convs run as the fused stem kernel
    bool stem_conv2 = false;       // ... and the 1x1 conv that follows them (64 -> 32) runs inside it as well (fp32 and bf16 plans)
    int xcd_mode = 1;              // y3_net_set_xcd_mode: 0 contiguous tile runs per XCD, 1 XCD-blocked order chosen per conv
    bool low_latency_set = false;  // y3_net_set_low_latency was called (the Y3_LOW_LATENCY tool override then stays out)
    bool low_latency = false;      // y3_net_set_low_latency: every eligible fp32 conv takes y3_choose_split_k
    void *split_ws = nullptr;      // split-K slabs: split_ws_lanes regions of split_ws_lane bytes, one per lane (lanes run concurrently)
    size_t split_ws_lane = 0;
    int split_ws_lanes = 0;
    int k_chunk = -1;              // y3_net_set_k_chunk: fp32 3x3 convs walk K chunk-major, this many input channels per chunk; 0 tap-major; -1 per-conv default
    hipEvent_t fork_ev = nullptr;
    hipStream_t lane_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t join_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<void *> tdev;      // arena pointer per tensor (nullptr: not materialised / external)
    std::vector<size_t> tbytes;    // bytes at max_batch
    std::vector<size_t> tblock;    // size of the arena block the tensor lives in
    std::vector<void *> blocks;    // distinct hipMalloc'ed blocks
};

namespace {

int rows(const y3_net *n, int t) { return n->height / n->tensors[t].div; }
int cols(const y3_net *n, int t) { return n->width / n->tensors[t].div; }

void free_plan(y3_net *n)
{
    if (n->det_buf) (void)hipFree(n->det_buf);
    n->det_buf = nullptr;
    n->det_bytes = 0;
    if (n->split_ws) (void)hipFree(n->split_ws);
    n->split_ws = nullptr;
    n->split_ws_lane = 0;
    n->split_ws_lanes = 0;
    for (void *p : n->blocks) (void)hipFree(p);
    n->blocks.clear();
    n->tdev.assign(n->tensors.size(), nullptr);
}

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

// three bf16 planes: x = hi + mid + lo exactly
void split_bf16x3(float x, unsigned short v[3])
{
    v[0] = f32_to_bf16_rne(x);
    const float r1 = x - bf16_to_f32(v[0]);
    v[1] = f32_to_bf16_rne(r1);
    v[2] = f32_to_bf16_rne(r1 - bf16_to_f32(v[1]));
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

// The first candidate tile that fits the conv and gives at least `want` workgroups for M rows over `cout_pad` channels; the last
// candidate when none does.
template <size_t N>
int first_reaching(const int (&cand)[N], y3::TileInfo (*info)(int), const ConvSlot &c, int cout_pad, long long M, long long want)
{
    for (int t : cand) {
        const y3::TileInfo s = info(t);
        if (fits(s, c, cout_pad) && ((M + s.bm - 1) / s.bm) * (cout_pad / s.bn) >= want) return t;
    }
    return cand[N - 1];
}

int choose_tile_x2(const ConvSlot &c, long long M)
{
    // widest tile that still gives every CU at least two workgroups
    static constexpr int wide[] = {4, 8, 0, 3, 2}, narrow[] = {1, 2};
    if (c.cout_pad64 % 128 == 0) return first_reaching(wide, y3::conv_x3_tile_info, c, c.cout_pad64, M, 512);
    return first_reaching(narrow, y3::conv_x3_tile_info, c, c.cout_pad64, M, 512);
}

int choose_tile_x3(const ConvSlot &c, long long M)
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
    static constexpr int bk32[] = {5, 6},    // BK = 32 (Cin = 32 layers, Cout = 64)
                         n128[] = {8, 12, 11},   // LDS-DMA variants: 128x128, 64x128, 64x64
                         n64[] = {10, 11}, n32[] = {4};
    if (c.d.cin % 64) return first_reaching(bk32, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512);
    if (c.cout_pad % 128 == 0) return first_reaching(n128, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512);
    if (c.cout_pad % 64 == 0) return first_reaching(n64, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512);
    return first_reaching(n32, y3::conv_bf16_tile_info, c, c.cout_pad, M, 512);
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

int choose_tile(const ConvSlot &c, long long M)
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

static bool is_output(const y3_net *net, int t) { return t == net->outputs[0] || t == net->outputs[1] || t == net->outputs[2]; }

// The first two ops are conv0 (3x3/1, 3 -> 32) and conv1 (3x3/2, 32 -> 64, no shortcut, single source) reading it, nobody
// else reads conv0's output, and the plan is fp32 with every intermediate reusable: the pair runs as csrc/conv_stem.hip.
static bool stem_applicable(const y3_net *net)
{
    if ((net->dtype != Y3_DTYPE_F32 && net->dtype != Y3_DTYPE_BF16) || net->keep_all || net->height % 32 || net->width % 32 || net->early_ops > 0)
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
static bool stem_conv2_applicable(const y3_net *net)
{
    if ((net->dtype != Y3_DTYPE_F32 && net->dtype != Y3_DTYPE_BF16) || net->ops.size() < 3 || net->ops[2].kind != 0) return false;
    const y3_conv_desc &b = net->convs[net->ops[1].index].d, &c = net->convs[net->ops[2].index].d;
    if (c.size != 1 || c.stride != 1 || c.cin != 64 || c.cout != 32 || c.residual >= 0 || c.src1 >= 0 || c.src0 != b.dst) return false;
    return !is_output(net, c.dst);
}

// ---- split-K (low-latency fp32 plans) --------------------------------------------------------------------------------------
// Can conv `slot` ever run split?  From the graph and the forced tile alone (no plan needed): not the first layer, not the
// weight-resident tile 33, not a detection head (y3_net_detect runs the heads through conv_head.hip, and the composed route
// must stay bit-identical to it), and only on the two tiles the split form is built for.  why: the refusal's text.
static bool split_eligible(const y3_net *net, int slot, const char **why)
{
    const ConvSlot &c = net->convs[slot];
    const char *w = nullptr;
    if (c.first_layer) w = "the first layer (Cin = 3) is never split";
    else if (net->nclasses > 0 && is_output(net, c.d.dst)) w = "a detection-head conv is never split (y3_net_detect decodes it in its own kernel)";
    else if (c.tile >= 0 ? !y3::conv_split_tile(c.tile) : !y3::conv_split_tile(choose_tile(c, 1)))
        w = "the conv's tile has no split form (tiles 10 and 11 have; the weight-resident tile 33 and the 32-wide tile 8 have not)";
    if (why) *why = w;
    return !w;
}

// does conv op oi run inside the fused stem launch (or as it)?
static bool in_fused_stem(const y3_net *net, int oi) { return (net->stem_fused && oi < 2) || (net->stem_conv2 && oi == 2); }

// Decide ConvSlot::split_k of every conv and size the slab workspace.  Runs at the end of y3_net_plan_hw and again from every
// setter that changes an input of the decision on a planned net; never from the enqueue path.  Inputs: the conv's shape, its tile at
// the planned batch, max_batch, n_cus, the caller's request -- never the rows of a call, so within one plan an image's bits do not
// depend on its batch or position (the rule choose_tile_bf16 states for the MFMA shape).
static y3_status resolve_splits(y3_net *net)
{
    if (!net->height) return Y3_OK;
    size_t lane_bytes = 0;
    for (int oi = 0; oi < (int)net->ops.size(); ++oi) {
        if (net->ops[oi].kind != 0) continue;
        const int slot = net->ops[oi].index;
        ConvSlot &c = net->convs[slot];
        c.split_k = 1;
        if (net->dtype != Y3_DTYPE_F32 || in_fused_stem(net, oi) || !split_eligible(net, slot, nullptr)) continue;
        if (c.split_req == 1 || (c.split_req < 0 && !net->low_latency)) continue;
        const long long M = (long long)net->max_batch * (net->height / c.d.out_div) * (net->width / c.d.out_div);
        const int tile = c.tile >= 0 ? c.tile : choose_tile(c, M);
        const y3::TileInfo t = y3::conv_tile_info(tile);
        const long long tiles = ((M + t.bm - 1) / t.bm) * (c.cout_pad / t.bn);
        const size_t slab = y3::conv_split_slab_bytes(tile, M, c.cout_pad);
        const int kt = c.K / t.bk;
        int S = c.split_req > 1 ? c.split_req : y3_choose_split_k(tiles, kt, net->n_cus, (long long)slab);
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
    return resolve_splits(net);
}

// Is net output t staged in a non-fp32 plan -- produced in the arena in the mode's own format and converted into the caller's fp32
// grid at the end of the forward -- because a conv reads it again inside the net, or a conv with no fp32-output form of its launch
// (shortcut, first layer) writes it?  Needs no plan: y3_net_plan marks `staged` by it, and y3_net_set_tile_bf16 refuses the
// bf16-only tile 32 on a conv whose output is not staged.
static bool output_staged(const y3_net *net, int t)
{
    for (const Op &o : net->ops) {
        if (o.kind != 0) continue;
        const ConvSlot &c = net->convs[o.index];
        if (c.d.src0 == t || c.d.src1 == t || c.d.residual == t) return true;
        if (c.d.dst == t && (c.d.residual >= 0 || c.first_layer)) return true;
    }
    return false;
}

// bytes per element of an arena tensor: fp32, bf16, three bf16 planes, or two fp16 planes (4 bytes as well)
static size_t arena_elem_bytes(int dtype) { return dtype == Y3_DTYPE_BF16 ? 2 : dtype == Y3_DTYPE_F32X3 ? 6 : 4; }

// One conv family per plan mode (Y3_DTYPE_*): its tile table (y3_tile_built), the tile a caller forced on a conv and the texts with which
// its setter refuses one (y3_net_set_tile*).
struct ConvFamily {
    int count;                                     // tile ids are [0, count)
    y3::TileInfo (*info)(int);
    bool (*built)(int);
    int ConvSlot::*tile;                           // forced tile, -1: the chooser's
    int ConvSlot::*cout_pad;                       // padded Cout of the mode's packed weights
    const char *bad, *retired, *misfit;            // refusals: bad argument, retired id (format: the id), tile does not fit the conv
    int resident;                                  // id of the weight-resident kernel, -1: none
    y3_status (*resident_rule)(const y3_net *, const ConvSlot &, int slot);   // its own shape rule
};
// ... and what the two plane-split modes (three bf16 planes, two fp16 planes per value) differ in at launch time
struct PlaneSplit : ConvFamily {
    void *ConvSlot::*w;     // packed weights
    int planes;
    int (*choose)(const ConvSlot &, long long);
    hipError_t (*launch)(const y3::ConvArgs &, int, bool, hipStream_t);
};

static y3_status resident_rule_f32(const y3_net *, const ConvSlot &c, int)
{
    if (!(c.d.size == 3 && c.d.stride == 1 && c.d.src1 < 0 && c.d.cin == 32 && c.d.cout % 64 == 0))
        return fail(Y3_ERR_INVALID, "y3_net_set_tile: tile 33 (weight-resident) needs a 3x3 / stride-1 conv with 32 input channels and Cout %% 64 == 0");
    return Y3_OK;
}

static y3_status resident_rule_bf16(const y3_net *net, const ConvSlot &c, int slot)
{
    if (!(c.d.size == 3 && c.d.stride == 1 && c.d.src1 < 0 && (c.d.cin == 32 || c.d.cin == 64) && c.d.cout % 64 == 0))
        return fail(Y3_ERR_INVALID, "y3_net_set_tile_bf16: tile 32 (weight-resident) needs a 3x3 / stride-1 conv with 32 or 64 input channels and Cout %% 64 == 0");
    // tile 32 stores bf16 only: a conv whose destination is a net output that the forward hands over as fp32 straight from the launch
    // (not read again inside the net, no shortcut: y3_net_plan does not stage it) cannot take it -- refused here, by name, instead of a
    // launch error in the forward
    if (is_output(net, c.d.dst) && !output_staged(net, c.d.dst))
        return fail(Y3_ERR_INVALID, "y3_net_set_tile_bf16: tile 32 (weight-resident) stores bf16 only; conv %d writes an fp32 net output", slot);
    return Y3_OK;
}

static constexpr ConvFamily F32_FAMILY = {
    y3::TILE_COUNT, y3::conv_tile_info, y3::conv_tile_built, &ConvSlot::tile, &ConvSlot::cout_pad,
    "y3_net_set_tile: bad argument", "y3_net_set_tile: tile id %d is retired (the timing ablations of rounds 1-2; y3_tile_built)",
    "y3_net_set_tile: tile does not divide Cout", 33, resident_rule_f32};
static constexpr ConvFamily BF16_FAMILY = {
    y3::BF16_TILE_COUNT, y3::conv_bf16_tile_info, y3::conv_bf16_tile_built, &ConvSlot::tile_bf16, &ConvSlot::cout_pad,
    "y3_net_set_tile_bf16: bad argument",
    "y3_net_set_tile_bf16: tile id %d is retired (20: the pipelined tile of round 2; 33..36: tap-row reuse and the four-wave tile of round 4; y3_tile_built)",
    "y3_net_set_tile_bf16: tile does not fit this conv", 32, resident_rule_bf16};
static constexpr PlaneSplit X3_SPLIT = {
    {y3::X3_TILE_COUNT, y3::conv_x3_tile_info, y3::conv_x3_tile_built, &ConvSlot::tile_x3, &ConvSlot::cout_pad64,
     "y3_net_set_tile_x3: bad argument", "y3_net_set_tile_x3: bad argument", "y3_net_set_tile_x3: tile does not fit this conv", -1, nullptr},
    &ConvSlot::wx3_dev, 3, choose_tile_x3, y3::launch_conv_f32x3};
static constexpr PlaneSplit X2_SPLIT = {
    {y3::X3_TILE_COUNT, y3::conv_x3_tile_info, y3::conv_x2_tile_built, &ConvSlot::tile_x2, &ConvSlot::cout_pad64,
     "y3_net_set_tile_x2: bad argument", "y3_net_set_tile_x2: tile does not fit this conv", "y3_net_set_tile_x2: tile does not fit this conv", -1, nullptr},
    &ConvSlot::wx2_dev, 2, choose_tile_x2, y3::launch_conv_f32x2};

static const ConvFamily *conv_family(int dtype)
{
    switch (dtype) {
        case Y3_DTYPE_F32: return &F32_FAMILY;
        case Y3_DTYPE_BF16: return &BF16_FAMILY;
        case Y3_DTYPE_F32X3: return &X3_SPLIT;
        case Y3_DTYPE_F32X2: return &X2_SPLIT;
        default: return nullptr;
    }
}

// The one body of y3_net_set_tile / _bf16 / _x3 / _x2: a built id that fits the conv (-1: back to the tuning table / the heuristic)
static y3_status set_forced_tile(const ConvFamily &f, y3_net *net, int slot, int tile)
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
    const ConvFamily *f = conv_family(dtype);
    return (f && f->built(tile)) ? 1 : 0;
}

y3_status y3_net_create(const y3_tensor_desc *tensors, int n_tensors, const int32_t *op_kinds, int n_ops,
                        const y3_conv_desc *convs, int n_convs, const y3_aux_desc *aux, int n_aux, int input_tensor,
                        const int32_t outputs[3], int nclasses, y3_net **out)
try {
    if (!tensors || !op_kinds || !convs || !outputs || !out || n_tensors <= 0 || n_ops <= 0 || n_convs < 0 || n_aux < 0)
        return fail(Y3_ERR_INVALID, "y3_net_create: null, empty or negative-count argument");
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
    for (int i = 0; i < 3; ++i) {
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
    *out = net.release();
    return Y3_OK;
}
Y3_CATCH("y3_net_create")

void y3_net_destroy(y3_net *net)
{
    if (!net) return;
    free_plan(net);
    if (net->fork_ev) {
        (void)hipEventDestroy(net->fork_ev);
        for (int i = 0; i < Y3_MAX_LANES; ++i) {
            (void)hipStreamDestroy(net->lane_stream[i]);
            (void)hipEventDestroy(net->join_ev[i]);
        }
    }
    for (ConvSlot &c : net->convs)
        for (void *p : {(void *)c.w_dev, (void *)c.w0stem_dev, (void *)c.w0raw_dev, c.wbf_dev, c.wx3_dev, c.wx2_dev, (void *)c.scale_dev, (void *)c.shift_dev})
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
    } else {
        // fp32 path: the BN scale is folded into the packed weights (one VALU multiply less per output element; VALU
        // time is matrix-pipe time for the fp32 MFMA).  The bf16 copy keeps the unscaled weights + scale in the epilogue.
        const std::vector<float> pk = pack_rows(w, K, d.cout, CP, nullptr), pk_scaled = pack_rows(w, K, d.cout, CP, scale.data());
        HIP_TRY(upload(c.w_dev, pk_scaled));
        HIP_TRY(upload(c.wbf_dev, pack_planes<1>(pk, K, d.cout, CP, [](float x, unsigned short *v) { v[0] = f32_to_bf16_rne(x); })));
        // a scaled weight outside the fp16 range: y3_net_plan(Y3_DTYPE_F32X2) refuses the net; other modes are unaffected
        c.x2_ok = std::all_of(pk_scaled.begin(), pk_scaled.end(), [](float x) { return fabsf(x) < 65504.0f; });
        HIP_TRY(upload(c.wx3_dev, pack_planes<3>(pk, K, d.cout, CP64, split_bf16x3)));         // unscaled, like the bf16 copy
        HIP_TRY(upload(c.wx2_dev, pack_planes<2>(pk_scaled, K, d.cout, CP64, split_f16x2)));   // BN-scaled, like the fp32 copy
    }
    HIP_TRY(upload(c.scale_dev, scale));
    HIP_TRY(upload(c.shift_dev, shift));
    c.loaded = true;
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
    return set_forced_tile(BF16_FAMILY, net, slot, tile);
}
Y3_CATCH("y3_net_set_tile_bf16")

y3_status y3_net_set_tile_x3(y3_net *net, int slot, int tile)
try {
    return set_forced_tile(X3_SPLIT, net, slot, tile);
}
Y3_CATCH("y3_net_set_tile_x3")

y3_status y3_net_set_tile_x2(y3_net *net, int slot, int tile)
try {
    return set_forced_tile(X2_SPLIT, net, slot, tile);
}
Y3_CATCH("y3_net_set_tile_x2")

y3_status y3_net_set_lanes(y3_net *net, int lanes)
try {
    if (!net || lanes < 1 || lanes > Y3_MAX_LANES) return fail(Y3_ERR_INVALID, "y3_net_set_lanes: lanes must be in [1,%d]", Y3_MAX_LANES);
    net->lanes = lanes;
    return resolve_splits_of_setter(net);   // one slab workspace per lane
}
Y3_CATCH("y3_net_set_lanes")

y3_status y3_net_set_stem_fusion(y3_net *net, int on)
try {
    if (!net || on < 0 || on > 2) return fail(Y3_ERR_INVALID, "y3_net_set_stem_fusion: argument must be 0, 1 or 2");
    net->stem_mode = on;
    net->stem_mode_set = true;
    // takes effect at once on a planned net when the graph qualifies (decided again by the next y3_net_plan)
    if (net->height) {
        net->stem_fused = on && stem_applicable(net);
        net->stem_conv2 = net->stem_fused && on == 1 && stem_conv2_applicable(net);
    }
    return resolve_splits_of_setter(net);   // a conv inside the fused stem is not split
}
Y3_CATCH("y3_net_set_stem_fusion")

y3_status y3_net_set_k_chunk(y3_net *net, int channels)
try {
    if (!net || channels < -1 || (channels > 0 && channels % 32)) return fail(Y3_ERR_INVALID, "y3_net_set_k_chunk: -1, 0 or a multiple of 32 channels");
    net->k_chunk = channels;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_k_chunk")

y3_status y3_net_set_low_latency(y3_net *net, int on)
try {
    if (!net || on < 0 || on > 1) return fail(Y3_ERR_INVALID, "y3_net_set_low_latency: argument must be 0 or 1");
    net->low_latency = on != 0;
    net->low_latency_set = true;
    return resolve_splits_of_setter(net);
}
Y3_CATCH("y3_net_set_low_latency")

y3_status y3_net_set_split_k(y3_net *net, int slot, int S)
try {
    if (!net || slot < 0 || slot >= (int)net->convs.size() || S < -1 || S == 0 || S > 16)
        return fail(Y3_ERR_INVALID, "y3_net_set_split_k: conv slot out of range, or S not -1, 1 or 2..16");
    ConvSlot &c = net->convs[slot];
    if (S > 1) {
        const char *why = nullptr;
        if (!split_eligible(net, slot, &why)) return fail(Y3_ERR_INVALID, "y3_net_set_split_k: conv %d: %s", slot, why);
        if (net->height && net->dtype != Y3_DTYPE_F32) return fail(Y3_ERR_INVALID, "y3_net_set_split_k: conv %d: only Y3_DTYPE_F32 plans split K", slot);
        for (int oi = 0; oi < 3 && oi < (int)net->ops.size() && net->height; ++oi)
            if (net->ops[oi].kind == 0 && net->ops[oi].index == slot && in_fused_stem(net, oi))
                return fail(Y3_ERR_INVALID, "y3_net_set_split_k: conv %d runs inside the fused stem kernel, which is never split", slot);
        if (S > c.K / 32) return fail(Y3_ERR_INVALID, "y3_net_set_split_k: conv %d has %d K tiles, fewer than S = %d", slot, c.K / 32, S);
    }
    c.split_req = S;
    return resolve_splits_of_setter(net);
}
Y3_CATCH("y3_net_set_split_k")

y3_status y3_net_set_xcd_mode(y3_net *net, int mode)
try {
    if (!net || mode < 0 || mode > 1) return fail(Y3_ERR_INVALID, "y3_net_set_xcd_mode: mode must be 0 or 1");
    net->xcd_mode = mode;
    return Y3_OK;
}
Y3_CATCH("y3_net_set_xcd_mode")

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

static void detect_layout(const y3_net *net, int batch, size_t off[9], size_t *n_boxes, int32_t gs[3][2], size_t gelems[3]);

// forked streams / events of the concurrent sub-batches: created at plan time so that a forward enqueues work only
static y3_status ensure_lanes(y3_net *net)
{
    if (net->fork_ev) return Y3_OK;
    HIP_TRY(hipEventCreateWithFlags(&net->fork_ev, hipEventDisableTiming));
    for (int i = 0; i < Y3_MAX_LANES; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&net->lane_stream[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&net->join_ev[i], hipEventDisableTiming));
    }
    return Y3_OK;
}

// Arena blocks for the plan's tensors from their liveness [first, last] over the op list
static y3_status place_tensors(y3_net *net, const std::vector<int> &first, const std::vector<int> &last)
{
    const int nt = (int)net->tensors.size();
    struct Blk { void *p; size_t bytes; int free_at; };
    std::vector<Blk> pool;
    // allocate in order of first definition; the image batch and the head grids are caller-owned
    std::vector<int> order;
    for (int t = 0; t < nt; ++t) {
        const bool external = t == net->input_tensor || (is_output(net, t) && !net->staged[t]);
        if (first[t] >= 0 && !external) order.push_back(t);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    for (int t : order) {
        const int until = (net->keep_all || net->dense[t]) ? (int)net->ops.size() + 1 : last[t];
        int pick = -1;
        for (int k = 0; k < (int)pool.size() && !net->dense[t]; ++k)
            if (pool[k].free_at < first[t] && pool[k].bytes >= net->tbytes[t] &&
                (pick < 0 || pool[k].bytes < pool[pick].bytes))
                pick = k;
        if (pick < 0) {
            void *p = nullptr;
            hipError_t e = hipMalloc(&p, net->tbytes[t] + 4096);
            if (e != hipSuccess) {
                free_plan(net);
                return fail(Y3_ERR_OOM, "y3_net_plan: hipMalloc(%zu) failed: %s", net->tbytes[t], hipGetErrorString(e));
            }
            net->blocks.push_back(p);
            pool.push_back({p, net->tbytes[t], until});
            pick = (int)pool.size() - 1;
        }
        pool[pick].free_at = until;
        net->tdev[t] = pool[pick].p;
        net->tblock[t] = pool[pick].bytes;
    }
    return Y3_OK;
}

y3_status y3_net_plan_hw(y3_net *net, int max_batch, int height, int width, int dtype)
try {
    if (!net || max_batch <= 0 || height <= 0 || width <= 0) return fail(Y3_ERR_INVALID, "y3_net_plan: bad argument");
    if (dtype != Y3_DTYPE_F32 && dtype != Y3_DTYPE_BF16 && dtype != Y3_DTYPE_F32X3 && dtype != Y3_DTYPE_F32X2)
        return fail(Y3_ERR_INVALID, "y3_net_plan: unknown dtype %d", dtype);
    for (const y3_tensor_desc &t : net->tensors)
        if (t.div <= 0 || height % t.div || width % t.div) {
            if (height == width) return fail(Y3_ERR_INVALID, "y3_net_plan: image_size %d not divisible by %d", height, t.div);   // the square call's text, as ever
            return fail(Y3_ERR_INVALID, "y3_net_plan_hw: image size %d x %d (height x width) not divisible by %d", height, width, t.div);
        }
    if (dtype == Y3_DTYPE_F32X2)
        for (size_t i = 0; i < net->convs.size(); ++i)
            if (net->convs[i].loaded && !net->convs[i].x2_ok)
                return fail(Y3_ERR_INVALID, "y3_net_plan: conv %zu has a BN-scaled weight outside the fp16 range (|w| >= 65504); "
                                            "the two-plane mode cannot represent it, use Y3_DTYPE_F32 or Y3_DTYPE_F32X3", i);
    Y3_ENTER_DEVICE(net);
    if (net->n_cus <= 0) {   // once per net: the launch path itself makes no device query
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, net->device));
        net->n_cus = cus > 0 ? cus : 256;
    }
    free_plan(net);
    net->max_batch = max_batch;
    net->height = height;
    net->width = width;
    net->dtype = dtype;
    const int nt = (int)net->tensors.size();
    // liveness over the op list; tensors with equal lifetime class share blocks (first-fit free list)
    std::vector<int> first(nt, -1), last(nt, -1);
    auto touch = [&](int t, int i) {
        if (t < 0) return;
        if (first[t] < 0) first[t] = i;
        last[t] = i;
    };
    for (int i = 0; i < (int)net->ops.size(); ++i) {
        const Op &o = net->ops[i];
        if (o.kind == 0) {
            const y3_conv_desc &d = net->convs[o.index].d;
            touch(d.src0, i); touch(d.src1, i); touch(d.residual, i); touch(d.dst, i);
        } else {
            const y3_aux_desc &a = net->aux[o.index];
            touch(a.src0, i); touch(a.src1, i); touch(a.dst, i);
        }
    }
    net->staged.assign(nt, 0);
    if (dtype != Y3_DTYPE_F32)
        for (int k = 0; k < 3; ++k)
            if (output_staged(net, net->outputs[k])) {
                net->staged[net->outputs[k]] = 1;
                last[net->outputs[k]] = (int)net->ops.size();        // alive until the final conversion
            }
    // chunked leading segment: every op before the (early_convs)-th conv; tensors it writes get blocks of their own,
    // laid out densely by image, because they are rewritten chunk after chunk while earlier chunks' results are still live
    net->early_ops = 0;
    if (net->early_convs > 0 && net->early_chunk > 0) {
        int seen = 0;
        for (int i = 0; i < (int)net->ops.size(); ++i) {
            if (net->ops[i].kind == 0 && seen++ == net->early_convs) break;
            net->early_ops = i + 1;
        }
        if (net->early_ops >= (int)net->ops.size()) net->early_ops = 0;
    }
    net->dense.assign(nt, 0);
    for (int t = 0; t < nt; ++t) net->dense[t] = (first[t] >= 0 && first[t] < net->early_ops) ? 1 : 0;
    for (int t = 0; t < nt; ++t) {
        net->tbytes[t] = (size_t)max_batch * rows(net, t) * cols(net, t) * net->tensors[t].channels * arena_elem_bytes(dtype);
        if (net->tbytes[t] >= 0xFFFFFFF0ull && first[t] >= 0)
            return fail(Y3_ERR_INVALID, "y3_net_plan: tensor %d is %zu bytes; 32-bit buffer offsets need < 4 GiB, lower max_batch", t, net->tbytes[t]);
    }
    if (y3_status st = place_tensors(net, first, last); st != Y3_OK) return st;
    if (y3_status st = ensure_lanes(net); st != Y3_OK) return st;
    {   // Y3_STEM_MODE (tools: same-process-tree A/B of the stem forms) overrides the default, not an explicit setter call
        static const int env = [] { const char *e = getenv("Y3_STEM_MODE"); return e ? atoi(e) : -1; }();
        if (env >= 0 && env <= 2 && !net->stem_mode_set) net->stem_mode = env;
    }
    net->stem_fused = net->stem_mode && stem_applicable(net);
    net->stem_conv2 = net->stem_fused && net->stem_mode == 1 && stem_conv2_applicable(net);
    {   // Y3_LOW_LATENCY (tools/ab_libs.py: a low-latency plan in a child process that knows nothing of it) overrides the default, not the setter
        static const int env = [] { const char *e = getenv("Y3_LOW_LATENCY"); return e ? atoi(e) : -1; }();
        if ((env == 0 || env == 1) && !net->low_latency_set) net->low_latency = env == 1;
    }
    if (net->nclasses > 0) {   // scratch of y3_net_detect: no allocation inside the stream-ordered call
        size_t off[9], n_boxes, gelems[3];
        int32_t gs[3][2];
        detect_layout(net, max_batch, off, &n_boxes, gs, gelems);
        hipError_t e = hipMalloc(&net->det_buf, off[8]);
        if (e != hipSuccess) {
            free_plan(net);
            return fail(Y3_ERR_OOM, "y3_net_plan: hipMalloc(%zu) for the detect scratch failed: %s", off[8], hipGetErrorString(e));
        }
        net->det_bytes = off[8];
    }
    if (y3_status st = resolve_splits(net); st != Y3_OK) {
        free_plan(net);
        return st;
    }
    return Y3_OK;
}
Y3_CATCH("y3_net_plan_hw")

y3_status y3_net_plan(y3_net *net, int max_batch, int image_size, int dtype)
try {
    return y3_net_plan_hw(net, max_batch, image_size, image_size, dtype);
}
Y3_CATCH("y3_net_plan")

// byte offsets of the y3_net_detect scratch for `batch` images (and the total in [8])
static void detect_layout(const y3_net *net, int batch, size_t off[9], size_t *n_boxes, int32_t gs[3][2], size_t gelems[3])
{
    const size_t per = (size_t)3 * (5 + net->nclasses);
    size_t n = 0;
    for (int i = 0; i < 3; ++i) {
        gs[i][0] = rows(net, net->outputs[i]);
        gs[i][1] = cols(net, net->outputs[i]);
        gelems[i] = (size_t)batch * gs[i][0] * gs[i][1] * per;
        n += (size_t)3 * gs[i][0] * gs[i][1];
    }
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    off[0] = 0;                                              // grid 0
    off[1] = off[0] + up(gelems[0] * 4);                     // grid 1
    off[2] = off[1] + up(gelems[1] * 4);                     // grid 2
    off[3] = off[2] + up(gelems[2] * 4);                     // boxes
    off[4] = off[3] + up((size_t)batch * n * 16);            // class indices (i64)
    off[5] = off[4] + up((size_t)batch * n * 8);             // scores
    off[6] = off[5] + up((size_t)batch * n * 4);             // selected indices
    off[7] = off[6] + up((size_t)batch * Y3_MAX_OUTPUT_BOXES * 4);   // NMS workspace
    off[8] = off[7] + y3::nms_workspace_bytes(batch, (int)n);
    *n_boxes = n;
}

int y3_net_get_split_k(const y3_net *net, int slot)
{
    if (!net || slot < 0 || slot >= (int)net->convs.size() || !net->height) return 1;
    return net->convs[slot].split_k;
}

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

double y3_net_flops_per_image(const y3_net *net)
{
    if (!net || !net->height) return 0.0;
    double tot = 0;
    for (const ConvSlot &c : net->convs) {
        const double ho = net->height / c.d.out_div, wo = net->width / c.d.out_div;
        tot += 2.0 * c.d.size * c.d.size * c.d.cin * c.d.cout * ho * wo;
    }
    return tot;
}

// One call's forward: everything that belongs to the call rather than the net.  Built on the stack by each entry point that
// runs the conv program; the net itself is read-only while a forward is enqueued.
struct Forward {
    const float *images;
    float *const *grids;                     // [3] caller's fp32 head grids
    int batch;
    hipStream_t stream;
    int lanes;                               // concurrent sub-batches this call may use (the net's y3_net_set_lanes, or 1)
    const y3::DecodeHead *heads = nullptr;   // [3] in output order: the head convs decode their own tiles into these buffers
                                             // (per scale: first box index, grid size, anchors) instead of writing grids
    unsigned long long *clk = nullptr;       // y3_net_measure_sclk*: device buffer the stamped launch(es) write
    int clk_conv = -1;                       // ... which conv (-2: every conv, 8 words each at clk + 8 conv)
    float *ms_out = nullptr;                 // y3_net_profile_convs: milliseconds per conv slot (n_ms entries)
    int n_ms = 0;
};

// argument checks shared by the entry points that run the conv program; `heads`: the call needs detection heads
static y3_status check_forward_args(const y3_net *net, bool args_ok, int batch, bool heads, const char *who)
{
    if (!net || !args_ok || batch <= 0) return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    if (heads && net->nclasses <= 0) return fail(Y3_ERR_STATE, "%s: the net was created without detection heads (nclasses = 0)", who);
    if (!net->height) return fail(Y3_ERR_STATE, "%s: call y3_net_plan first", who);
    if (batch > net->max_batch) return fail(Y3_ERR_INVALID, "%s: batch %d > planned %d", who, batch, net->max_batch);
    return Y3_OK;
}

// The part of a forward one run() step enqueues: images [b0, b0 + nb) of the batch, as lane `lane`, on stream s
struct Slice {
    const y3_net *net;
    const Forward &f;
    int b0, nb, lane;
    hipStream_t s;

    size_t img_elems(int t) const { return (size_t)rows(net, t) * cols(net, t) * net->tensors[t].channels; }
    // a net output written straight into the caller's fp32 grid (not staged)
    bool caller_grid(int t) const { return is_output(net, t) && !net->staged[t]; }
    // element size: head grids are always fp32; the image batch is fp32 when the Cin = 3 first-layer kernel reads it
    // (a model whose input feeds an MFMA conv directly hands bf16 in bf16 mode); everything else follows the plan
    size_t elem_bytes(int t) const
    {
        if (caller_grid(t)) return 4;
        if (t == net->input_tensor) return net->tensors[t].channels != 3 ? arena_elem_bytes(net->dtype) : 4;
        return arena_elem_bytes(net->dtype);
    }
    size_t bytes(int t) const { return (size_t)nb * img_elems(t) * elem_bytes(t); }

    void *ptr(int t) const
    {
        if (t < 0) return nullptr;
        char *base = nullptr;
        if (t == net->input_tensor) base = reinterpret_cast<char *>(const_cast<float *>(f.images));
        for (int i = 0; i < 3 && !base; ++i)
            if (t == net->outputs[i] && !net->staged[t]) base = reinterpret_cast<char *>(f.grids[i]);
        if (base) return base + (size_t)b0 * img_elems(t) * elem_bytes(t);
        // arena tensors share blocks with other (dead) tensors of different per-image size: give every lane its
        // own 1/lanes region of the block so that concurrent sub-batches never alias
        char *blk = static_cast<char *>(net->tdev[t]);
        if (!blk) return nullptr;
        if (net->dense[t]) return blk + (size_t)b0 * img_elems(t) * elem_bytes(t);
        // lane regions start at the lane's first image (scaled to the block size), 256-B aligned; blocks carry 4 KiB of slack
        const size_t off = ((size_t)((double)net->tblock[t] * b0 / f.batch) + 255) & ~(size_t)255;
        return blk + (lane ? off : 0);
    }

    // ConvArgs of conv slot `conv`; *head: which output it decodes in place (fused decode; its grid is then not written), else -1
    y3::ConvArgs conv_args(int conv, int *head) const
    {
        const ConvSlot &c = net->convs[conv];
        const y3_conv_desc &d = c.d;
        y3::ConvArgs a{};
        a.src0 = ptr(d.src0);
        a.src1 = ptr(d.src1);
        a.wpk = c.w_dev;
        a.scale = c.scale_dev;
        a.shift = c.shift_dev;
        a.residual = ptr(d.residual);
        a.dst = ptr(d.dst);
        a.B = nb;
        a.H = net->height / d.in_div;
        a.W = net->width / d.in_div;
        a.Ho = net->height / d.out_div;
        a.Wo = net->width / d.out_div;
        a.Cin = d.cin;
        a.C0 = d.c0;
        a.Cout = d.cout;
        a.CoutPad = c.cout_pad;
        a.ksize = d.size;
        a.stride = d.stride;
        a.pad = (d.size == 3) ? 1 : 0;
        a.up0 = d.src0_upsample;
        a.leaky = d.leaky;
        a.M = nb * a.Ho * a.Wo;
        a.K = c.K;
        a.src0_bytes = (unsigned)bytes(d.src0);
        a.src1_bytes = d.src1 >= 0 ? (unsigned)bytes(d.src1) : 0;
        a.w_bytes = (unsigned)((size_t)c.cout_pad * c.K * sizeof(float));
        a.dst_bytes = (unsigned)bytes(d.dst);
        a.n_cus = net->n_cus;
        a.device = net->device;
        a.clk_stamps = !f.clk ? nullptr : f.clk_conv == conv ? f.clk : f.clk_conv == -2 ? f.clk + 8 * conv : nullptr;   // fp32 MFMA kernel and stem only
        *head = -1;
        if (f.heads)
            for (int k = 0; k < 3; ++k)
                if (d.dst == net->outputs[k] && !net->staged[d.dst]) *head = k;
        if (*head >= 0) {
            a.dec = f.heads[*head];
            a.dec.boxes += (size_t)b0 * a.dec.N * 4;
            a.dec.cls += (size_t)b0 * a.dec.N;
            a.dec.scores += (size_t)b0 * a.dec.N;
            a.dst = nullptr;
            a.dst_bytes = 0;
        }
        return a;
    }

    // the fused stem launch (op 1) from conv1's own args: conv0 (op 0) and, with stem_conv2, the 1x1 of op 2 run inside it
    y3_status launch_stem(const y3::ConvArgs &a1) const
    {
        const bool bf = net->dtype == Y3_DTYPE_BF16;
        const ConvSlot &c0 = net->convs[net->ops[0].index], &c1 = net->convs[net->ops[1].index];
        y3::StemArgs sa{};
        sa.img = static_cast<const float *>(ptr(c0.d.src0));
        sa.w0 = bf ? c0.w0raw_dev : c0.w0stem_dev;
        sa.scale0 = c0.scale_dev;
        sa.shift0 = c0.shift_dev;
        sa.w1 = bf ? c1.wbf_dev : static_cast<const void *>(c1.w_dev);
        sa.scale1 = c1.scale_dev;
        sa.shift1 = c1.shift_dev;
        sa.dst = a1.dst;
        sa.B = nb;
        sa.H = net->height;
        sa.W = net->width;
        sa.leaky0 = c0.d.leaky;
        sa.leaky1 = c1.d.leaky;
        sa.img_bytes = (unsigned)bytes(c0.d.src0);
        sa.dst_bytes = a1.dst_bytes;
        sa.device = net->device;
        sa.n_cus = net->n_cus;
        sa.clk_stamps = a1.clk_stamps;
        if (net->stem_conv2) {
            const ConvSlot &c2 = net->convs[net->ops[2].index];
            sa.w2 = bf ? c2.wbf_dev : static_cast<const void *>(c2.w_dev);
            sa.scale2 = c2.scale_dev;
            sa.shift2 = c2.shift_dev;
            sa.dst2 = ptr(c2.d.dst);
            sa.leaky2 = c2.d.leaky;
            sa.dst2_bytes = (unsigned)bytes(c2.d.dst);
            if (!sa.dst2) return fail(Y3_ERR_STATE, "conv %d: tensor not planned", net->ops[2].index);
        }
        hipError_t e = bf ? y3::launch_conv_stem_bf16(sa, s) : y3::launch_conv_stem_f32(sa, s);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "conv %d launch: %s", net->ops[1].index, hipGetErrorString(e));
        return Y3_OK;
    }

    // pick and launch the kernel of conv op oi (args from conv_args, adjusted here per mode)
    y3_status launch_conv(int oi, y3::ConvArgs &a, int head) const
    {
        if (net->stem_fused && oi == 1) return launch_stem(a);
        const int conv = net->ops[oi].index;
        const ConvSlot &c = net->convs[conv];
        const y3_conv_desc &d = c.d;
        const bool bf = net->dtype == Y3_DTYPE_BF16;
        const PlaneSplit *split = net->dtype == Y3_DTYPE_F32X3 ? &X3_SPLIT : net->dtype == Y3_DTYPE_F32X2 ? &X2_SPLIT : nullptr;
        const bool out_f32 = caller_grid(d.dst);   // bf16 / plane-split plans: the launch stores the fp32 grid itself
        hipError_t e;
        if (c.first_layer) {
            if (net->dtype != Y3_DTYPE_F32 && out_f32) return fail(Y3_ERR_INVALID, "conv %d: first layer cannot be a head in this mode", conv);
            e = y3::launch_conv_first(a, c.w_dev, net->dtype, s);
        } else if (split) {
            a.wpk = c.*split->w;
            a.CoutPad = c.cout_pad64;
            a.w_bytes = (unsigned)((size_t)c.cout_pad64 * split->planes * c.K * 2);
            if (d.residual >= 0 && out_f32) return fail(Y3_ERR_INVALID, "conv %d: residual on a head output is not supported in this mode", conv);
            e = split->launch(a, c.*split->tile >= 0 ? c.*split->tile : split->choose(c, a.M), out_f32, s);
        } else if (bf) {
            a.wpk = c.wbf_dev;
            a.w_bytes = (unsigned)((size_t)c.cout_pad * c.K * 2);
            if (d.residual >= 0 && out_f32) return fail(Y3_ERR_INVALID, "conv %d: residual on a head output is not supported in bf16 mode", conv);
            int tile = c.tile_bf16 >= 0 ? c.tile_bf16 : choose_tile_bf16(c, a.M, (long long)net->max_batch * a.Ho * a.Wo, !out_f32);
            if (head >= 0 && y3::conv_bf16_tile_info(tile).bn != 256) {   // a box's logits must meet in one workgroup: all 256 channels in the tile
                const bool m16 = tile >= 24 && tile <= 29;                // keep the MFMA shape of the plan's tile: same K grouping, same bits
                const bool big = (a.M + 255) / 256 >= 256;                // 256x256 once it fills the chip, else 128x256 (16 waves both)
                tile = m16 ? (big ? 24 : 26) : (big ? 17 : 19);
            }
            e = y3::launch_conv_bf16(a, tile, out_f32, s);
        } else if (head >= 0) {
            e = y3::launch_conv_head_decode_f32(a, s);
        } else {
            const int tile = c.tile >= 0 ? c.tile : choose_tile(c, a.M);
            if (net->xcd_mode && c.split_k <= 1) a.xcd_gn = choose_xcd_gn(c, a, y3::conv_tile_info(tile));
            {   // K order of the 3x3 convs (conv_f32.hip): chunk-major when the conv has more input channels than one chunk
                const int ck = net->k_chunk >= 0 ? net->k_chunk : default_k_chunk(c);
                if (d.size == 3 && d.src1 < 0 && ck > 0 && d.cin > ck && d.cin % ck == 0 && ck % 32 == 0) a.k_chunk = ck;
            }
            if (c.split_k > 1) {   // low-latency plan: S slices of the K walk into this lane's slabs, then the finish launch
                if (lane >= net->split_ws_lanes) return fail(Y3_ERR_STATE, "conv %d: no split-K workspace for lane %d", conv, lane);
                e = y3::launch_conv_f32_split(a, tile, c.split_k, static_cast<char *>(net->split_ws) + (size_t)lane * net->split_ws_lane,
                                              net->split_ws_lane, s);
            } else {
                e = y3::launch_conv_f32(a, tile, s);
            }
        }
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "conv %d launch: %s", conv, hipGetErrorString(e));
        return Y3_OK;
    }

    y3_status run_aux(int index) const
    {
        if (net->dtype != Y3_DTYPE_F32) return fail(Y3_ERR_INVALID, "stand-alone add/upsample/concat ops are fp32 only");
        const y3_aux_desc &x = net->aux[index];
        auto p = [&](int t) { return static_cast<float *>(ptr(t)); };
        const int sh = rows(net, x.dst), sw = cols(net, x.dst);
        const int C = net->tensors[x.dst].channels;
        hipError_t e = hipSuccess;
        if (x.kind == Y3_AUX_ADD)
            e = y3::launch_add(p(x.src0), p(x.src1), p(x.dst), (size_t)nb * sh * sw * C, s);
        else if (x.kind == Y3_AUX_UPSAMPLE2X)
            e = y3::launch_upsample2x(p(x.src0), nb, sh / 2, sw / 2, C, p(x.dst), s);
        else if (x.kind == Y3_AUX_CONCAT)
            e = y3::launch_concat(p(x.src0), net->tensors[x.src0].channels, p(x.src1), net->tensors[x.src1].channels, (size_t)nb * sh * sw, p(x.dst), s);
        else
            return fail(Y3_ERR_INVALID, "unknown aux op kind %d", x.kind);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "aux op %d launch: %s", index, hipGetErrorString(e));
        return Y3_OK;
    }

    // Enqueue ops [op_begin, op_end) of the op list; the segment that ends the list also converts the staged outputs to fp32.
    y3_status run(int op_begin, int op_end) const
    {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if (f.ms_out) {
            HIP_TRY(hipEventCreate(&ev0));
            HIP_TRY(hipEventCreate(&ev1));
        }
        for (int oi = op_begin; oi < op_end; ++oi) {
            const Op &o = net->ops[oi];
            if (o.kind != 0) {
                if (y3_status st = run_aux(o.index); st != Y3_OK) return st;
                continue;
            }
            int head;
            y3::ConvArgs a = conv_args(o.index, &head);
            if (!a.src0 || (!a.dst && head < 0)) return fail(Y3_ERR_STATE, "conv %d: tensor not planned", o.index);
            if ((net->stem_fused && oi == 0) || (net->stem_conv2 && oi == 2)) {   // runs inside conv1's launch (fused stem)
                if (f.ms_out && o.index < f.n_ms) f.ms_out[o.index] = 0.0f;
                continue;
            }
            if (f.ms_out) HIP_TRY(hipEventRecord(ev0, s));
            if (y3_status st = launch_conv(oi, a, head); st != Y3_OK) return st;
            if (f.ms_out) {
                HIP_TRY(hipEventRecord(ev1, s));
                HIP_TRY(hipEventSynchronize(ev1));
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
                if (o.index < f.n_ms) f.ms_out[o.index] = ms;
            }
        }
        for (int k = 0; k < 3 && op_end == (int)net->ops.size(); ++k) {
            const int t = net->outputs[k];
            if (!net->staged[t]) continue;
            const size_t npix = (size_t)nb * rows(net, t) * cols(net, t);
            hipError_t e = y3::launch_to_f32(net->dtype, ptr(t), f.grids[k] + (size_t)b0 * img_elems(t), npix, net->tensors[t].channels, s);
            if (e != hipSuccess) return fail(Y3_ERR_HIP, "output %d conversion: %s", k, hipGetErrorString(e));
        }
        if (f.ms_out) {
            (void)hipEventDestroy(ev0);
            (void)hipEventDestroy(ev1);
        }
        return Y3_OK;
    }
};

static y3_status run(const y3_net *net, const Forward &f)
{
    if (y3_status st = check_forward_args(net, f.images && f.grids, f.batch, false, "y3_net_forward"); st != Y3_OK) return st;
    for (size_t i = 0; i < net->convs.size(); ++i)
        if (!net->convs[i].loaded) return fail(Y3_ERR_STATE, "y3_net_forward: conv %zu has no weights", i);
    if (net->dtype == Y3_DTYPE_F32X2)
        for (size_t i = 0; i < net->convs.size(); ++i)
            if (!net->convs[i].x2_ok) return fail(Y3_ERR_INVALID, "y3_net_forward: conv %zu has a weight outside the fp16 range of the two-plane mode", i);
    for (int i = 0; i < 3; ++i)
        if (!f.grids[i] || ((uintptr_t)f.grids[i] & 15)) return fail(Y3_ERR_INVALID, "y3_net_forward: grid %d null or not 16-byte aligned", i);
    if ((uintptr_t)f.images & 3) return fail(Y3_ERR_INVALID, "y3_net_forward: images not 4-byte aligned");
    Y3_ENTER_DEVICE(net);   // launches go to the net's device whatever the caller's current one is; restored on return
    const hipStream_t s = f.stream;
    const int batch = f.batch;
    // Images are independent, so the batch can run as `lanes` sub-batches on forked streams: while one sub-batch's
    // conv kernel drains (its last workgroups leave CUs under-occupied), the other sub-batch's kernel fills them.
    int lanes = f.lanes;
    while (lanes > 1 && batch / lanes < 1) --lanes;
    // leading segment in chunks small enough for their activations to stay in the 256 MB Infinity Cache between the
    // conv that writes them and the one that reads them, then the rest of the op list on the whole (sub-)batch
    const int k_early = f.ms_out ? 0 : net->early_ops;
    auto run_lane = [&](int b0, int nb, hipStream_t st, int lane) -> y3_status {
        if (k_early > 0) {
            for (int c0 = 0; c0 < nb; c0 += net->early_chunk) {
                const int cn = nb - c0 < net->early_chunk ? nb - c0 : net->early_chunk;
                y3_status r = Slice{net, f, b0 + c0, cn, lane, st}.run(0, k_early);
                if (r != Y3_OK) return r;
            }
        }
        return Slice{net, f, b0, nb, lane, st}.run(k_early, (int)net->ops.size());
    };
    if (lanes == 1) return run_lane(0, batch, s, 0);
    if (!net->fork_ev) return fail(Y3_ERR_STATE, "y3_net_forward: no lane streams (y3_net_plan creates them)");
    HIP_TRY(hipEventRecord(net->fork_ev, s));
    // equal sub-batches (measured with tools/lanes_sweep.py: weighted 2:3 / 3:4:5 splits were 2-3 % slower)
    int start[Y3_MAX_LANES + 1];
    for (int l = 0; l <= lanes; ++l) start[l] = (int)((long long)batch * l / lanes);
    // lane 0 runs on the caller's stream itself: its first kernel needs no cross-queue signal to start, and the join waits for the other lanes only
    // (fp32 eager step 31.324 -> 31.218 ms, +0.3 %, every round of three; bf16 graph replay unchanged: profiles/r05_ab_lane0_on_caller_stream.txt)
    hipStream_t ls[Y3_MAX_LANES];
    for (int l = 0; l < Y3_MAX_LANES; ++l) ls[l] = l == 0 ? s : net->lane_stream[l];
    for (int l = 0; l < lanes; ++l)
        if (start[l + 1] > start[l] && ls[l] != s) HIP_TRY(hipStreamWaitEvent(ls[l], net->fork_ev, 0));
    if (k_early > 0) {
        for (int l = 0; l < lanes; ++l) {
            const int nb = start[l + 1] - start[l];
            if (nb <= 0) continue;
            y3_status st = run_lane(start[l], nb, ls[l], l);
            if (st != Y3_OK) return st;
        }
    } else {
        // op-major enqueue: op k of every lane before op k+1 of any.  Enqueued lane by lane, an eager forward gives lane 0 a
        // head start of one whole forward's worth of host launch time (0.3 ms; 0.9 ms under a profiler: the per-queue timeline of
        // tools/timeline_dump.py shows lane 0 four kernels ahead), and a start offset between the lanes only costs
        // (profiles/r03_ab_lane_stagger.txt).  A captured forward replays with both branches released at once either way.
        const int n_ops = (int)net->ops.size();
        // (A start offset between the lanes was measured again in round 5 for the fp32 plan -- lane 1 released 1 / 2 / 4 ops behind lane 0: at most
        // +0.28 %, inside the process-to-process spread, profiles/r05_ab_f32_lane_stagger.txt; not kept.)
        for (int oi = 0; oi < n_ops; ++oi)
            for (int l = 0; l < lanes; ++l) {
                const int nb = start[l + 1] - start[l];
                if (nb <= 0) continue;
                y3_status st = Slice{net, f, start[l], nb, l, ls[l]}.run(oi, oi + 1);
                if (st != Y3_OK) return st;
            }
    }
    for (int l = 0; l < lanes; ++l) {
        if (start[l + 1] <= start[l]) continue;
        if (ls[l] == s) continue;
        HIP_TRY(hipEventRecord(net->join_ev[l], ls[l]));
        HIP_TRY(hipStreamWaitEvent(s, net->join_ev[l], 0));
    }
    return Y3_OK;
}

y3_status y3_net_forward(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], void *stream)
try {
    return run(net, {images_dev, grids_dev, batch, (hipStream_t)stream, net ? net->lanes : 1});
}
Y3_CATCH("y3_net_forward")

y3_status y3_net_profile_convs(y3_net *net, const float *images_dev, int batch, float *ms_out, int n, void *stream)
try {
    if (!net || !ms_out) return fail(Y3_ERR_INVALID, "y3_net_profile_convs: bad argument");
    // head grids go to scratch owned by this call
    if (!net->height || batch <= 0) return fail(Y3_ERR_STATE, "y3_net_profile_convs: call y3_net_plan first (and batch > 0)");
    Y3_ENTER_DEVICE(net);
    float *g[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        const int t = net->outputs[i];
        hipError_t e = hipMalloc(&g[i], (size_t)batch * rows(net, t) * cols(net, t) * net->tensors[net->outputs[i]].channels * sizeof(float));
        if (e != hipSuccess) {
            for (int k = 0; k < i; ++k) (void)hipFree(g[k]);
            return fail(Y3_ERR_OOM, "y3_net_profile_convs: hipMalloc: %s", hipGetErrorString(e));
        }
    }
    Forward f{images_dev, g, batch, (hipStream_t)stream, 1};   // one lane: each launch is timed on its own
    f.ms_out = ms_out;
    f.n_ms = n;
    y3_status st = run(net, f);
    (void)hipStreamSynchronize((hipStream_t)stream);
    for (int i = 0; i < 3; ++i) (void)hipFree(g[i]);
    return st;
}
Y3_CATCH("y3_net_profile_convs")

namespace {
// can conv slot i of this plan carry the clock stamps?  The fp32 MFMA kernel (fp32 plans) and the fused stem kernel do.
bool conv_carries_stamps(const y3_net *net, size_t i)
{
    const ConvSlot &c = net->convs[i];
    const bool stem = net->stem_fused && net->ops.size() > 1 && net->ops[1].kind == 0 && net->ops[1].index == (int)i;
    if (stem) return true;
    if (net->stem_fused && (i == (size_t)net->ops[0].index || (net->stem_conv2 && net->ops.size() > 2 && i == (size_t)net->ops[2].index)))
        return false;    // runs inside the stem launch
    return net->dtype == Y3_DTYPE_F32 && !c.first_layer && c.split_k <= 1;   // a split launch carries no stamps
}
// pick >= 0: that conv, *mhz_out one value; pick == -2: every conv that carries stamps, mhz_out / start_us / end_us arrays of
// convs.size() entries (0 where a conv left no stamps; times relative to the earliest stamp, from s_memrealtime)
y3_status measure_sclk_arrays(const y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                              int pick, float *mhz_out, double *start_us, double *end_us, void *stream)
{
    Y3_ENTER_DEVICE(net);
    const size_t nconv = net->convs.size();
    const size_t words = pick == -2 ? 8 * nconv : 8;   // per conv: memtime, realtime at entry; the same after the epilogue; realtime at the entry of workgroup 0
    std::vector<unsigned long long> host(words, 0ull);
    unsigned long long *buf = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&buf), words * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(buf, 0, words * sizeof(unsigned long long), (hipStream_t)stream);
    // the chip's clock follows the load of the last milliseconds: stamp the LAST of `forwards` back-to-back forwards
    y3_status st = Y3_OK;
    // one lane: one launch of a stamped conv (concurrent sub-batches would each stamp the same words)
    Forward f{images_dev, grids_dev, batch, (hipStream_t)stream, 1};
    for (int i = 0; i < forwards && st == Y3_OK && e == hipSuccess; ++i) {
        f.clk = (i == forwards - 1) ? buf : nullptr;
        f.clk_conv = (i == forwards - 1) ? pick : -1;
        st = run(net, f);
    }
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(host.data(), buf, words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (st != Y3_OK) return st;
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_net_measure_sclk: %s", hipGetErrorString(e));
    if (pick >= 0) {
        const double ticks = (double)(host[2] - host[0]), real = (double)(host[3] - host[1]);
        if (!(real > 0.0) || !(ticks > 0.0)) return fail(Y3_ERR_STATE, "y3_net_measure_sclk: conv %d left no stamps", pick);
        *mhz_out = (float)(ticks / real * 100.0);   // s_memrealtime counts at 100 MHz
        return Y3_OK;
    }
    // start = entry of the launch's FIRST workgroup (word 4; the stem kernel stamps in workgroup 0 throughout: word 1),
    // end = after the epilogue of the clock-stamped workgroup (a middle one; the stem: workgroup 0, resident to the end)
    auto first = [&](size_t c) { return host[8 * c + 4] ? host[8 * c + 4] : host[8 * c + 1]; };
    unsigned long long t0 = ~0ull;
    for (size_t c = 0; c < nconv; ++c)
        if (host[8 * c + 3] > host[8 * c + 1] && first(c) < t0) t0 = first(c);
    int stamped = 0;
    for (size_t c = 0; c < nconv; ++c) {
        const double ticks = (double)(host[8 * c + 2] - host[8 * c]), real = (double)(host[8 * c + 3] - host[8 * c + 1]);
        const bool ok = host[8 * c + 3] > host[8 * c + 1] && host[8 * c + 2] > host[8 * c];
        mhz_out[c] = ok ? (float)(ticks / real * 100.0) : 0.0f;
        if (start_us) start_us[c] = ok ? (double)(first(c) - t0) / 100.0 : 0.0;
        if (end_us) end_us[c] = ok ? (double)(host[8 * c + 3] - t0) / 100.0 : 0.0;
        stamped += ok;
    }
    if (!stamped) return fail(Y3_ERR_STATE, "y3_net_measure_sclk_all: no launch of this plan left clock stamps (fp32 plan or fused stem needed)");
    return Y3_OK;
}
}  // namespace

y3_status y3_net_measure_sclk_conv(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                                   int conv, float *mhz_out, void *stream)
try {
    if (!net || !mhz_out || forwards < 1 || conv < 0 || conv >= (int)net->convs.size())
        return fail(Y3_ERR_INVALID, "y3_net_measure_sclk_conv: bad argument");
    if (!conv_carries_stamps(net, (size_t)conv))
        return fail(Y3_ERR_STATE, "y3_net_measure_sclk_conv: the launch of conv %d carries no clock stamps in this plan", conv);
    return measure_sclk_arrays(net, images_dev, batch, grids_dev, forwards, conv, mhz_out, nullptr, nullptr, stream);
}
Y3_CATCH("y3_net_measure_sclk_conv")

y3_status y3_net_measure_sclk(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                              float *mhz_out, void *stream)
try {
    if (!net || !mhz_out || forwards < 1) return fail(Y3_ERR_INVALID, "y3_net_measure_sclk: bad argument");
    // the launch that carries the stamps: the conv with the most FLOPs among those whose kernel has them -- the fp32 MFMA
    // kernel (fp32 plans; a steady-state workgroup of a ~0.8 ms launch) or the fused stem kernel (fp32 and bf16 plans)
    int pick = -1;
    double best = 0;
    for (size_t i = 0; i < net->convs.size(); ++i) {
        const ConvSlot &c = net->convs[i];
        if (!conv_carries_stamps(net, i)) continue;
        const double ho = net->height / c.d.out_div, wo = net->width / c.d.out_div;   // 0 without a plan
        const double fl = 2.0 * c.d.size * c.d.size * c.d.cin * c.d.cout * ho * wo;
        if (fl > best) { best = fl; pick = (int)i; }
    }
    if (pick < 0) return fail(Y3_ERR_STATE, "y3_net_measure_sclk: no launch of this plan carries clock stamps (fp32 plan or fused stem needed)");
    return measure_sclk_arrays(net, images_dev, batch, grids_dev, forwards, pick, mhz_out, nullptr, nullptr, stream);
}
Y3_CATCH("y3_net_measure_sclk")

y3_status y3_net_measure_sclk_all(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                                  float *mhz_out, double *start_us, double *end_us, void *stream)
try {
    if (!net || !mhz_out || forwards < 1) return fail(Y3_ERR_INVALID, "y3_net_measure_sclk_all: bad argument");
    return measure_sclk_arrays(net, images_dev, batch, grids_dev, forwards, -2, mhz_out, start_us, end_us, stream);
}
Y3_CATCH("y3_net_measure_sclk_all")

y3_status y3_net_read_tensor(y3_net *net, int t, int batch, float *dst_dev, size_t *n_elems, void *stream)
try {
    if (!net || t < 0 || t >= (int)net->tensors.size() || !net->height)
        return fail(Y3_ERR_INVALID, "y3_net_read_tensor: bad argument");
    const size_t npix = (size_t)batch * rows(net, t) * cols(net, t);
    const size_t n = npix * net->tensors[t].channels;
    if (n_elems) *n_elems = n;
    if (!dst_dev) return Y3_OK;
    if (!net->tdev[t]) return fail(Y3_ERR_STATE, "y3_net_read_tensor: tensor %d is not held in the arena", t);
    Y3_ENTER_DEVICE(net);   // the conversion kernels / the copy below read the net's arena: enqueue them on its device
    hipError_t e = y3::launch_to_f32(net->dtype, net->tdev[t], dst_dev, npix, net->tensors[t].channels, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_net_read_tensor: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_net_read_tensor")

// ------------------------------------------------------------------------------------------ image input
namespace {
// is_uint8 / y3_image_desc.mode: 0, 1 or 2, with or without Y3_IMAGE_LETTERBOX
bool image_mode_ok(int mode) { return (mode & ~Y3_IMAGE_LETTERBOX) >= 0 && (mode & ~Y3_IMAGE_LETTERBOX) <= 2; }
// the geometry of one image: the whole canvas without the flag
y3::LetterboxGeom image_geom(int mode, int h, int w, int Hc, int Wc)
{
    return (mode & Y3_IMAGE_LETTERBOX) ? y3::letterbox_geom(h, w, Hc, Wc) : y3::LetterboxGeom{Hc, Wc, 0, 0};
}
}  // namespace

// The square entry points (y3_preprocess_image, ...) are their _hw counterparts with canvas_h == canvas_w; `who` names the
// entry point the caller used in the messages.
static y3_status preprocess_image_hw(const char *who, const void *image_dev, int is_uint8, int height, int width, int channels,
                                     float *batch_dev, int slot, int Hc, int Wc, void *stream)
{
    if (!image_dev || !batch_dev || height <= 0 || width <= 0 || channels < 3 || channels > 4 || slot < 0 ||
        Hc <= 0 || Wc <= 0 || !image_mode_ok(is_uint8) || ((is_uint8 & ~Y3_IMAGE_LETTERBOX) == 0 && ((uintptr_t)image_dev & 3)))
        return fail(Y3_ERR_INVALID, "%s: bad argument (channels must be 3 or 4)", who);
    const y3::LetterboxGeom g = image_geom(is_uint8, height, width, Hc, Wc);
    if (!y3::letterbox_geom_fits(g, Hc, Wc))
        return fail(Y3_ERR_INVALID, "%s: letterbox of %d x %d (%d x %d at %d, %d) does not fit %d x %d", who, height, width,
                    g.sh, g.sw, g.top, g.left, Hc, Wc);
    float *dst = batch_dev + (size_t)slot * Hc * Wc * 3;
    hipError_t e = y3::launch_resize(image_dev, is_uint8, height, width, channels, dst, Hc, Wc, g, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}

y3_status y3_preprocess_image_hw(const void *image_dev, int is_uint8, int height, int width, int channels,
                                 float *batch_dev, int slot, int canvas_h, int canvas_w, void *stream)
try {
    return preprocess_image_hw("y3_preprocess_image_hw", image_dev, is_uint8, height, width, channels, batch_dev, slot, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_preprocess_image_hw")

y3_status y3_preprocess_image(const void *image_dev, int is_uint8, int height, int width, int channels,
                              float *batch_dev, int slot, int image_size, void *stream)
try {
    return preprocess_image_hw("y3_preprocess_image", image_dev, is_uint8, height, width, channels, batch_dev, slot, image_size, image_size, stream);
}
Y3_CATCH("y3_preprocess_image")

static y3_status preprocess_batch_hw(const char *who, const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host,
                                     int n_images, float *batch_dev, int first_slot, int Hc, int Wc, void *stream)
{
    if (!pixels_dev || !descs_host || !batch_dev || n_images < 1 || first_slot < 0 || Hc <= 0 || Wc <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument (null pointer, n_images < 1, first_slot < 0 or image_size <= 0)", who);
    // every check before the first launch: a bad image late in the list must not leave the batch half written
    for (int i = 0; i < n_images; ++i) {
        const y3_image_desc &d = descs_host[i];
        if (d.channels < 3 || d.channels > 4)
            return fail(Y3_ERR_INVALID, "%s: image %d: channels must be 3 or 4 (got %d)", who, i, d.channels);
        if (!image_mode_ok(d.mode))
            return fail(Y3_ERR_INVALID, "%s: image %d: mode must be 0, 1 or 2, optionally | Y3_IMAGE_LETTERBOX (got %d)", who, i, d.mode);
        if (d.height < 1 || d.width < 1)
            return fail(Y3_ERR_INVALID, "%s: image %d: height and width must be at least 1 (got %d x %d)", who, i,
                        d.height, d.width);
        const bool f32 = (d.mode & ~Y3_IMAGE_LETTERBOX) == 0;
        if (f32 && ((d.offset & 3) || ((uintptr_t)pixels_dev & 3)))
            return fail(Y3_ERR_INVALID, "%s: image %d: float32 pixels must be 4-byte aligned (offset %llu)", who, i,
                        (unsigned long long)d.offset);
        // height, width < 2^31 and channels * elemsize <= 16: the product stays below 2^66, so take it in 128 bits
        const unsigned __int128 bytes = (unsigned __int128)d.height * (unsigned __int128)d.width * (unsigned)(d.channels * (f32 ? 4 : 1));
        if ((unsigned __int128)d.offset + bytes > (unsigned __int128)pixels_bytes)
            return fail(Y3_ERR_INVALID, "%s: image %d: %d x %d x %d at offset %llu runs past the %zu-byte pixel blob", who, i,
                        d.height, d.width, d.channels, (unsigned long long)d.offset, pixels_bytes);
        const y3::LetterboxGeom g = image_geom(d.mode, d.height, d.width, Hc, Wc);
        if (!y3::letterbox_geom_fits(g, Hc, Wc))
            return fail(Y3_ERR_INVALID, "%s: image %d: letterbox of %d x %d (%d x %d at %d, %d) does not fit %d x %d", who, i,
                        d.height, d.width, g.sh, g.sw, g.top, g.left, Hc, Wc);
    }
    const size_t per_image = (size_t)Hc * Wc * 3;
    for (int i0 = 0; i0 < n_images; i0 += y3::kPreprocessTableImages) {
        const int n = std::min(y3::kPreprocessTableImages, n_images - i0);
        y3::LetterboxGeom geoms[y3::kPreprocessTableImages];     // on the stack: the call allocates nothing
        for (int i = 0; i < n; ++i) geoms[i] = image_geom(descs_host[i0 + i].mode, descs_host[i0 + i].height, descs_host[i0 + i].width, Hc, Wc);
        hipError_t e = y3::launch_preprocess_batch(pixels_dev, descs_host + i0, geoms, n, batch_dev + ((size_t)first_slot + i0) * per_image,
                                                   Hc, Wc, (hipStream_t)stream);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    }
    return Y3_OK;
}

y3_status y3_preprocess_batch_hw(const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host, int n_images,
                                 float *batch_dev, int first_slot, int canvas_h, int canvas_w, void *stream)
try {
    return preprocess_batch_hw("y3_preprocess_batch_hw", pixels_dev, pixels_bytes, descs_host, n_images, batch_dev, first_slot, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_preprocess_batch_hw")

y3_status y3_preprocess_batch(const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host, int n_images,
                              float *batch_dev, int first_slot, int image_size, void *stream)
try {
    return preprocess_batch_hw("y3_preprocess_batch", pixels_dev, pixels_bytes, descs_host, n_images, batch_dev, first_slot, image_size, image_size, stream);
}
Y3_CATCH("y3_preprocess_batch")

static y3_status letterbox_geometry_hw(const char *who, const y3_image_desc *descs_host, int n_images, int Hc, int Wc, int32_t *geoms_out_host)
{
    if (!descs_host || !geoms_out_host || n_images < 1 || Hc <= 0 || Wc <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument (null pointer, n_images < 1 or image_size <= 0)", who);
    for (int i = 0; i < n_images; ++i) {
        const y3_image_desc &d = descs_host[i];
        if (!image_mode_ok(d.mode))
            return fail(Y3_ERR_INVALID, "%s: image %d: mode must be 0, 1 or 2, optionally | Y3_IMAGE_LETTERBOX (got %d)", who, i, d.mode);
        if (d.height < 1 || d.width < 1)
            return fail(Y3_ERR_INVALID, "%s: image %d: height and width must be at least 1 (got %d x %d)", who, i,
                        d.height, d.width);
    }
    static_assert(sizeof(y3::LetterboxGeom) == 4 * sizeof(int32_t), "a geometry is four int32");
    for (int i = 0; i < n_images; ++i) {
        const y3::LetterboxGeom g = image_geom(descs_host[i].mode, descs_host[i].height, descs_host[i].width, Hc, Wc);
        memcpy(geoms_out_host + (size_t)i * 4, &g, sizeof(g));
    }
    return Y3_OK;
}

y3_status y3_letterbox_geometry_hw(const y3_image_desc *descs_host, int n_images, int canvas_h, int canvas_w, int32_t *geoms_out_host)
try {
    return letterbox_geometry_hw("y3_letterbox_geometry_hw", descs_host, n_images, canvas_h, canvas_w, geoms_out_host);
}
Y3_CATCH("y3_letterbox_geometry_hw")

y3_status y3_letterbox_geometry(const y3_image_desc *descs_host, int n_images, int image_size, int32_t *geoms_out_host)
try {
    return letterbox_geometry_hw("y3_letterbox_geometry", descs_host, n_images, image_size, image_size, geoms_out_host);
}
Y3_CATCH("y3_letterbox_geometry")

static y3_status unletterbox_hw(const char *who, void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                int max_boxes, int Hc, int Wc, void *stream)
{
    if (!packed_dev || !num_valid_dev || !geoms_host || batch < 1 || Hc <= 0 || Wc <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument (null pointer, batch < 1 or image_size <= 0)", who);
    if (max_boxes <= 0 || max_boxes > Y3_MAX_OUTPUT_BOXES)
        return fail(Y3_ERR_INVALID, "%s: max_boxes must be in [1,%d]", who, Y3_MAX_OUTPUT_BOXES);
    // every check before the first launch: the rows are rewritten in place
    for (int i = 0; i < batch; ++i) {
        y3::LetterboxGeom g;
        memcpy(&g, geoms_host + (size_t)i * 4, sizeof(g));
        if (!y3::letterbox_geom_fits(g, Hc, Wc))
            return fail(Y3_ERR_INVALID, "%s: image %d: geometry %d x %d at (%d, %d) does not lie inside %d x %d", who, i,
                        g.sh, g.sw, g.top, g.left, Hc, Wc);
    }
    unsigned *packed = static_cast<unsigned *>(packed_dev);
    for (int i0 = 0; i0 < batch; i0 += y3::kUnletterboxTableImages) {
        const int n = std::min(y3::kUnletterboxTableImages, batch - i0);
        y3::LetterboxGeom geoms[y3::kUnletterboxTableImages];
        memcpy(geoms, geoms_host + (size_t)i0 * 4, (size_t)n * sizeof(y3::LetterboxGeom));
        hipError_t e = y3::launch_unletterbox(packed + (size_t)i0 * max_boxes * 7, num_valid_dev + i0, geoms, n, max_boxes, Hc, Wc,
                                              (hipStream_t)stream);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    }
    return Y3_OK;
}

y3_status y3_unletterbox_detections_hw(void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                       int max_boxes, int canvas_h, int canvas_w, void *stream)
try {
    return unletterbox_hw("y3_unletterbox_detections_hw", packed_dev, num_valid_dev, geoms_host, batch, max_boxes, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_unletterbox_detections_hw")

y3_status y3_unletterbox_detections(void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                    int max_boxes, int image_size, void *stream)
try {
    return unletterbox_hw("y3_unletterbox_detections", packed_dev, num_valid_dev, geoms_host, batch, max_boxes, image_size, image_size, stream);
}
Y3_CATCH("y3_unletterbox_detections")

y3_status y3_evaluate_detections(const void *packed_dev, const int32_t *num_valid_dev, int batch, int max_boxes,
                                 const float *gt_boxes_dev, const int32_t *gt_classes_dev, const int32_t *gt_count_dev, int max_gt,
                                 int nclasses, float iou_threshold, const float *score_thresholds_host, int n_thresholds,
                                 int one_class, int64_t *counters_dev, void *stream)
try {
    if (!packed_dev || !num_valid_dev || !gt_boxes_dev || !gt_classes_dev || !gt_count_dev || !score_thresholds_host || !counters_dev)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: null pointer");
    if (batch < 1) return fail(Y3_ERR_INVALID, "y3_evaluate_detections: batch must be at least 1 (got %d)", batch);
    if (max_boxes < 1 || max_boxes > y3::kEvalMaxBoxes)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: max_boxes must be in [1,%d] (got %d)", y3::kEvalMaxBoxes, max_boxes);
    if (max_gt < 1 || max_gt > y3::kEvalMaxGt)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: max_gt must be in [1,%d] (got %d)", y3::kEvalMaxGt, max_gt);
    if (nclasses < 1 || nclasses > y3::kEvalMaxClasses)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: nclasses must be in [1,%d] (got %d)", y3::kEvalMaxClasses, nclasses);
    if (n_thresholds < 1 || n_thresholds > y3::kEvalMaxThresholds)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: n_thresholds must be in [1,%d] (got %d)", y3::kEvalMaxThresholds, n_thresholds);
    if (((uintptr_t)packed_dev & 3) || ((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)counters_dev & 7))
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: packed / gt_boxes not 4-byte or counters not 8-byte aligned");
    y3::EvalThresholds thr{};
    for (int t = 0; t < n_thresholds; ++t) thr.s[t] = score_thresholds_host[t];
    hipError_t e = y3::launch_evaluate(packed_dev, num_valid_dev, batch, max_boxes, gt_boxes_dev, gt_classes_dev, gt_count_dev, max_gt,
                                       nclasses, iou_threshold, thr, n_thresholds, one_class != 0, counters_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_evaluate_detections launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_evaluate_detections")

// ------------------------------------------------------------------------------------------ validation loss
namespace {
// The checks and the by-value geometry the two loss entries share: grid sizes, first decode row per scale, anchors.
y3_status loss_geometry(const char *who, const int32_t *grid_sizes, const float *anchors_host, int batch, int max_gt, int nclasses,
                        y3::LossGeom *geo)
{
    if (!grid_sizes || !anchors_host) return fail(Y3_ERR_INVALID, "%s: null pointer", who);
    if (batch < 1) return fail(Y3_ERR_INVALID, "%s: batch must be at least 1 (got %d)", who, batch);
    if (max_gt < 1 || max_gt > y3::kEvalMaxGt) return fail(Y3_ERR_INVALID, "%s: max_gt must be in [1,%d] (got %d)", who, y3::kEvalMaxGt, max_gt);
    if (nclasses < 1 || nclasses > y3::kEvalMaxClasses)
        return fail(Y3_ERR_INVALID, "%s: nclasses must be in [1,%d] (got %d)", who, y3::kEvalMaxClasses, nclasses);
    int off = 0;
    for (int s = 0; s < 3; ++s) {
        if (grid_sizes[s] < 1 || grid_sizes[s] > y3::kLossMaxGrid)
            return fail(Y3_ERR_INVALID, "%s: grid_sizes[%d] must be in [1,%d] (got %d)", who, s, y3::kLossMaxGrid, grid_sizes[s]);
        geo->g[s] = grid_sizes[s];
        geo->off[s] = off;
        off += 3 * grid_sizes[s] * grid_sizes[s];
        for (int a = 0; a < 3; ++a) {
            geo->anchors[s][a][0] = anchors_host[(s * 3 + a) * 2 + 0];
            geo->anchors[s][a][1] = anchors_host[(s * 3 + a) * 2 + 1];
        }
    }
    return Y3_OK;
}
}  // namespace

y3_status y3_yolo_assign_targets(const float *gt_boxes_dev, const int32_t *gt_classes_dev, const int32_t *gt_count_dev, int batch,
                                 int max_gt, int nclasses, const int32_t grid_sizes[3], const float *anchors_host,
                                 int32_t *cells_dev, void *stream)
try {
    if (!gt_boxes_dev || !gt_classes_dev || !gt_count_dev || !cells_dev)
        return fail(Y3_ERR_INVALID, "y3_yolo_assign_targets: null pointer");
    y3::LossGeom geo{};
    y3_status st = loss_geometry("y3_yolo_assign_targets", grid_sizes, anchors_host, batch, max_gt, nclasses, &geo);
    if (st != Y3_OK) return st;
    if (((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)gt_classes_dev & 3) || ((uintptr_t)gt_count_dev & 3) || ((uintptr_t)cells_dev & 3))
        return fail(Y3_ERR_INVALID, "y3_yolo_assign_targets: a device pointer is not 4-byte aligned");
    hipError_t e = y3::launch_assign_targets(gt_boxes_dev, gt_classes_dev, gt_count_dev, batch, max_gt, nclasses, geo, cells_dev,
                                             (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_yolo_assign_targets launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_yolo_assign_targets")

y3_status y3_yolo_loss(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                       const float *anchors_host, const float *gt_boxes_dev, const int32_t *gt_classes_dev,
                       const int32_t *cells_dev, int max_gt, double *loss_dev, void *stream)
try {
    if (!grids_dev || !gt_boxes_dev || !gt_classes_dev || !cells_dev || !loss_dev)
        return fail(Y3_ERR_INVALID, "y3_yolo_loss: null pointer");
    y3::LossGeom geo{};
    y3_status st = loss_geometry("y3_yolo_loss", grid_sizes, anchors_host, batch, max_gt, nclasses, &geo);
    if (st != Y3_OK) return st;
    y3::LossGrids grids{};
    for (int s = 0; s < 3; ++s) {
        if (!grids_dev[s] || ((uintptr_t)grids_dev[s] & 3))
            return fail(Y3_ERR_INVALID, "y3_yolo_loss: grid %d null or not 4-byte aligned", s);
        grids.p[s] = grids_dev[s];
    }
    if (((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)gt_classes_dev & 3) || ((uintptr_t)cells_dev & 3) || ((uintptr_t)loss_dev & 7))
        return fail(Y3_ERR_INVALID, "y3_yolo_loss: gt_boxes / gt_classes / cells not 4-byte or loss not 8-byte aligned");
    hipError_t e = y3::launch_yolo_loss(grids, geo, batch, nclasses, gt_boxes_dev, gt_classes_dev, cells_dev, max_gt, loss_dev,
                                        (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_yolo_loss launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_yolo_loss")

// ------------------------------------------------------------------------------------------ TFRecord checksum
uint32_t y3_crc32c(const void *data_host, size_t nbytes)
{
    // slicing-by-8 over the reflected Castagnoli polynomial
    static uint32_t T[8][256];
    static bool ready = [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
        return true;
    }();
    (void)ready;
    const unsigned char *p = static_cast<const unsigned char *>(data_host);
    uint32_t c = 0xFFFFFFFFu;
    while (nbytes >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^ T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^ T[3][hi & 0xFF] ^
            T[2][(hi >> 8) & 0xFF] ^ T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
        p += 8;
        nbytes -= 8;
    }
    while (nbytes--) c = (c >> 8) ^ T[0][(c ^ *p++) & 0xFF];
    return c ^ 0xFFFFFFFFu;
}

// ------------------------------------------------------------------------------------------ decode
// gs: grid_hw[3][2] = {gh, gw} per scale (the square entry points hand {g, g})
static y3_status decode_common(const float *const grids[3], const int32_t (*gs)[2], int batch, int nc,
                               const float *anchors, float *bboxes, float *conf, float *probs, int64_t *cls,
                               float *scores, void *stream, const char *who)
{
    if (!grids || !gs || !anchors || !bboxes || batch <= 0 || nc <= 0) return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    y3::DecodeArgs a{};
    int off = 0;
    for (int s = 0; s < 3; ++s) {
        if (!grids[s] || gs[s][0] <= 0 || gs[s][1] <= 0 || ((uintptr_t)grids[s] & 15))
            return fail(Y3_ERR_INVALID, "%s: grid %d null, empty or not 16-byte aligned", who, s);
        a.grid[s] = grids[s];
        a.gh[s] = gs[s][0];
        a.gw[s] = gs[s][1];
        a.off[s] = off;
        off += gs[s][0] * gs[s][1] * 3;
        for (int k = 0; k < 3; ++k) {
            a.anchors[s][k][0] = anchors[(s * 3 + k) * 2 + 0];
            a.anchors[s][k][1] = anchors[(s * 3 + k) * 2 + 1];
        }
    }
    if ((uintptr_t)bboxes & 15) return fail(Y3_ERR_INVALID, "%s: bboxes not 16-byte aligned", who);
    a.B = batch;
    a.N = off;
    a.nc = nc;
    hipError_t e = y3::launch_decode(a, bboxes, conf, probs, cls, scores, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}

// The square entry points are the _hw ones with {g, g}; `who` names the entry point the caller used in the messages.
static y3_status yolo_decode_hw(const char *who, const float *const grids_dev[3], const int32_t (*grid_hw)[2], int batch, int nclasses,
                                const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
{
    if (!conf_dev || !probs_dev) return fail(Y3_ERR_INVALID, "%s: null output", who);
    return decode_common(grids_dev, grid_hw, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, nullptr, nullptr, stream, who);
}

static y3_status yolo_decode_scores_hw(const char *who, const float *const grids_dev[3], const int32_t (*grid_hw)[2], int batch, int nclasses,
                                       const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev, float *scores_dev, void *stream)
{
    if (!class_idx_dev || !scores_dev) return fail(Y3_ERR_INVALID, "%s: null output", who);
    return decode_common(grids_dev, grid_hw, batch, nclasses, anchors_host, bboxes_dev, nullptr, nullptr, class_idx_dev, scores_dev, stream, who);
}

y3_status y3_yolo_decode_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                            const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
try {
    return yolo_decode_hw("y3_yolo_decode_hw", grids_dev, grid_hw, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, stream);
}
Y3_CATCH("y3_yolo_decode_hw")

y3_status y3_yolo_decode_scores_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                                   const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev,
                                   float *scores_dev, void *stream)
try {
    return yolo_decode_scores_hw("y3_yolo_decode_scores_hw", grids_dev, grid_hw, batch, nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
}
Y3_CATCH("y3_yolo_decode_scores_hw")

y3_status y3_yolo_decode(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                         const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
try {
    if (!conf_dev || !probs_dev) return fail(Y3_ERR_INVALID, "y3_yolo_decode: null output");
    if (!grid_sizes) return fail(Y3_ERR_INVALID, "y3_yolo_decode: bad argument");
    const int32_t hw[3][2] = {{grid_sizes[0], grid_sizes[0]}, {grid_sizes[1], grid_sizes[1]}, {grid_sizes[2], grid_sizes[2]}};
    return yolo_decode_hw("y3_yolo_decode", grids_dev, hw, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, stream);
}
Y3_CATCH("y3_yolo_decode")

y3_status y3_yolo_decode_scores(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                                const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev,
                                float *scores_dev, void *stream)
try {
    if (!class_idx_dev || !scores_dev) return fail(Y3_ERR_INVALID, "y3_yolo_decode_scores: null output");
    if (!grid_sizes) return fail(Y3_ERR_INVALID, "y3_yolo_decode_scores: bad argument");
    const int32_t hw[3][2] = {{grid_sizes[0], grid_sizes[0]}, {grid_sizes[1], grid_sizes[1]}, {grid_sizes[2], grid_sizes[2]}};
    return yolo_decode_scores_hw("y3_yolo_decode_scores", grids_dev, hw, batch, nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
}
Y3_CATCH("y3_yolo_decode_scores")

y3_status y3_class_scores(const float *conf_dev, const float *probs_dev, int batch, int n, int nclasses,
                          int64_t *class_idx_dev, float *scores_dev, void *stream)
try {
    if (!conf_dev || !probs_dev || !class_idx_dev || !scores_dev || batch <= 0 || n <= 0 || nclasses <= 0)
        return fail(Y3_ERR_INVALID, "y3_class_scores: bad argument");
    hipError_t e = y3::launch_class_scores(conf_dev, probs_dev, (size_t)batch * n, nclasses, class_idx_dev, scores_dev,
                                           (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_class_scores launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_class_scores")

// ------------------------------------------------------------------------------------------ forward + decode
namespace {
// Can the three heads decode in place?  Each output must come from a 1x1 / stride-1 single-source conv without shortcut whose
// 3 * (5 + nc) channels fit one 256-wide tile, written straight to the caller-visible grid (not staged), in an fp32 or bf16
// plan.  Y3_FUSE_DECODE=0 (tools: A/B against the composed route) switches the fusion off.
bool heads_can_decode(const y3_net *net)
{
    static const bool off = [] { const char *e = getenv("Y3_FUSE_DECODE"); return e && e[0] == '0'; }();
    if (off || net->nclasses <= 0 || (net->dtype != Y3_DTYPE_F32 && net->dtype != Y3_DTYPE_BF16)) return false;
    if (net->keep_all || net->early_ops > 0 || 3 * (5 + net->nclasses) > 256) return false;
    for (int k = 0; k < 3; ++k) {
        const int t = net->outputs[k];
        if (net->staged[t]) return false;
        int producers = 0;
        for (const ConvSlot &c : net->convs) {
            if (c.d.dst != t) continue;
            ++producers;
            if (c.first_layer || c.d.size != 1 || c.d.stride != 1 || c.d.src1 >= 0 || c.d.residual >= 0 || c.d.cin % 64 ||
                c.d.cout != 3 * (5 + net->nclasses) || c.cout_pad != 256)
                return false;
        }
        if (producers != 1) return false;
        // the fused route does not write the grid: nobody inside the net may read it (fp32 plans never stage an output, so a
        // consumer would read the caller's buffer -- on this route uninitialised scratch)
        for (const ConvSlot &c : net->convs)
            if (c.d.src0 == t || c.d.src1 == t || c.d.residual == t) return false;
        for (const y3_aux_desc &x : net->aux)
            if (x.dst == t || x.src0 == t || x.src1 == t) return false;
    }
    return true;
}
}  // namespace

y3_status y3_net_forward_decode(y3_net *net, const float *images_dev, int batch, const float *anchors_host, float *bboxes_dev,
                                int64_t *class_idx_dev, float *scores_dev, void *stream)
try {
    y3_status st = check_forward_args(net, images_dev && anchors_host && bboxes_dev && class_idx_dev && scores_dev, batch, true,
                                      "y3_net_forward_decode");
    if (st != Y3_OK) return st;
    if ((uintptr_t)bboxes_dev & 15) return fail(Y3_ERR_INVALID, "y3_net_forward_decode: bboxes not 16-byte aligned");
    Y3_ENTER_DEVICE(net);
    int32_t gs[3][2];
    size_t gelems[3], n = 0, off[9];
    detect_layout(net, batch, off, &n, gs, gelems);
    if (!net->det_buf || net->det_bytes < off[8])
        return fail(Y3_ERR_STATE, "y3_net_forward_decode: detect scratch not planned (y3_net_plan allocates it)");
    char *b = static_cast<char *>(net->det_buf);
    float *grids[3] = {reinterpret_cast<float *>(b + off[0]), reinterpret_cast<float *>(b + off[1]), reinterpret_cast<float *>(b + off[2])};
    Forward f{images_dev, grids, batch, (hipStream_t)stream, net->lanes};
    if (!heads_can_decode(net)) {   // composed route: grids into the scratch, then the stand-alone decode
        if ((st = run(net, f)) != Y3_OK) return st;
        return yolo_decode_scores_hw("y3_yolo_decode_scores", grids, gs, batch, net->nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
    }
    y3::DecodeHead heads[3];
    int first = 0;
    for (int k = 0; k < 3; ++k) {
        heads[k].boxes = bboxes_dev;
        heads[k].cls = class_idx_dev;
        heads[k].scores = scores_dev;
        heads[k].gh = gs[k][0];
        heads[k].gw = gs[k][1];
        heads[k].off = first;
        heads[k].N = (int)n;
        heads[k].nc = net->nclasses;
        for (int a = 0; a < 3; ++a) {
            heads[k].anchors[a][0] = anchors_host[(k * 3 + a) * 2 + 0];
            heads[k].anchors[a][1] = anchors_host[(k * 3 + a) * 2 + 1];
        }
        first += gs[k][0] * gs[k][1] * 3;
    }
    f.heads = heads;
    return run(net, f);
}
Y3_CATCH("y3_net_forward_decode")

// ------------------------------------------------------------------------------------------ nms
// ------------------------------------------------------------------------------------------ whole pipeline
y3_status y3_net_detect(y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes,
                        float iou_threshold, float score_threshold, void *packed_dev, int32_t *num_valid_dev,
                        void *stream)
try {
    y3_status st = check_forward_args(net, images_dev && anchors_host && packed_dev && num_valid_dev, batch, true, "y3_net_detect");
    if (st != Y3_OK) return st;
    if (max_boxes <= 0 || max_boxes > Y3_MAX_OUTPUT_BOXES)
        return fail(Y3_ERR_INVALID, "y3_net_detect: max_boxes must be in [1,%d]", Y3_MAX_OUTPUT_BOXES);
    Y3_ENTER_DEVICE(net);   // the decode / NMS / pack launches below go to the net's device; the caller's current device is restored on return
    int32_t gs[3][2];
    size_t gelems[3], n = 0, off[9];
    detect_layout(net, batch, off, &n, gs, gelems);
    if (!net->det_buf || net->det_bytes < off[8])
        return fail(Y3_ERR_STATE, "y3_net_detect: detect scratch not planned (y3_net_plan allocates it)");
    const size_t o_box = off[3], o_cls = off[4], o_score = off[5];
    const size_t o_sel = off[6], o_ws = off[7];
    const size_t ws_bytes = y3::nms_workspace_bytes(batch, (int)n);
    char *b = static_cast<char *>(net->det_buf);
    float *boxes = reinterpret_cast<float *>(b + o_box), *scores = reinterpret_cast<float *>(b + o_score);
    int64_t *cls = reinterpret_cast<int64_t *>(b + o_cls);
    int32_t *sel = reinterpret_cast<int32_t *>(b + o_sel);
    // conv program with the head convs decoding their own tiles (grids neither written nor read back) where the graph allows it.
    // (Round 5 ran NMS + pack per lane, on each lane's stream behind its last conv: bit-identical and 0.2 % slower under graph replay -- the NMS
    // workgroups take CUs from the other lane's last convs; profiles/r05_ab_bf16_lane_nms.txt.  Batch-wide launches behind the join again.)
    st = y3_net_forward_decode(net, images_dev, batch, anchors_host, boxes, cls, scores, stream);
    if (st != Y3_OK) return st;
    st = y3_nms_padded(boxes, scores, batch, (int)n, max_boxes, iou_threshold, score_threshold, sel, num_valid_dev,
                       b + o_ws, ws_bytes, stream);
    if (st != Y3_OK) return st;
    return y3_pack_detections(boxes, cls, scores, sel, num_valid_dev, batch, (int)n, max_boxes, packed_dev, stream);
}
Y3_CATCH("y3_net_detect")

size_t y3_nms_workspace_bytes(int batch, int n) { return (batch > 0 && n > 0) ? y3::nms_workspace_bytes(batch, n) : 0; }

y3_status y3_nms_padded(const float *bboxes_dev, const float *scores_dev, int batch, int n, int max_output_size,
                        float iou_threshold, float score_threshold, int32_t *selected_idx_dev,
                        int32_t *num_valid_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
try {
    if (!bboxes_dev || !scores_dev || !selected_idx_dev || !num_valid_dev || batch <= 0 || n <= 0)
        return fail(Y3_ERR_INVALID, "y3_nms_padded: bad argument");
    if (max_output_size <= 0 || max_output_size > 1024)
        return fail(Y3_ERR_INVALID, "y3_nms_padded: max_output_size must be in [1,1024]");
    if ((uintptr_t)bboxes_dev & 15) return fail(Y3_ERR_INVALID, "y3_nms_padded: bboxes not 16-byte aligned");
    if (!(iou_threshold > 0.0f) && score_threshold < 0.0f)
        return fail(Y3_ERR_INVALID, "y3_nms_padded: iou_threshold <= 0 together with score_threshold < 0 is not supported");
    if (!workspace_dev || workspace_bytes < y3::nms_workspace_bytes(batch, n))
        return fail(Y3_ERR_INVALID, "y3_nms_padded: workspace too small (need %zu bytes)", y3::nms_workspace_bytes(batch, n));
    hipError_t e = y3::launch_nms(bboxes_dev, scores_dev, batch, n, max_output_size, iou_threshold, score_threshold,
                                  selected_idx_dev, num_valid_dev, workspace_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_nms_padded launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_nms_padded")

y3_status y3_pack_detections(const float *bboxes_dev, const int64_t *class_idx_dev, const float *scores_dev,
                             const int32_t *selected_idx_dev, const int32_t *num_valid_dev, int batch, int n,
                             int max_out, void *packed_dev, void *stream)
try {
    if (!bboxes_dev || !class_idx_dev || !scores_dev || !selected_idx_dev || !num_valid_dev || !packed_dev ||
        batch <= 0 || n <= 0 || max_out <= 0)
        return fail(Y3_ERR_INVALID, "y3_pack_detections: bad argument");
    hipError_t e = y3::launch_pack(bboxes_dev, class_idx_dev, scores_dev, selected_idx_dev, num_valid_dev, batch, n,
                                   max_out, packed_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_pack_detections launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_pack_detections")

}  // extern "C"
