// Fused stem of YOLOv3-tiny on gfx950: conv0 (3x3 / 1, 3 -> 16, BN, LeakyReLU), max-pool 2x2 / 2, conv1 (3x3 / 1, 16 -> 32, BN, LeakyReLU),
// max-pool 2x2 / 2 in ONE kernel (reference: config/models/yolov3_tiny/backbone.yaml layers 1-4 through core/parse_model.py:27-52 and
// :78-99).  The image batch [B,H,W,3] fp32 comes in, pool 1's tensor [B,H/4,W/4,32] goes out in the plan's format; conv0's tensor
// (H x W x 16), pool 0's (H/2 x W/2 x 16) and conv1's (H/2 x W/2 x 32) never reach memory.  The kernel works at the real widths 16 and
// K = 144: the zero pad channels with which the unfused plan stores 16 channels as 32 are neither computed nor stored, and the 32 -> 32 conv
// they make of conv1 -- for which the 16-bit tile tables have no tile -- does not exist here.
//
// One workgroup of four waves walks tiles of TH x TW = 4 x 8 pool-1 pixels (persistent: tile += gridDim.x; H and W are multiples of 32, so
// H/4 and W/4 are multiples of 8 and no tile is partial -- the stores are guarded all the same).  Per tile:
//   phase 1  conv0 + pool 0 for the 10 x 18 pooled positions that the tile's 8 x 16 conv1 pixels read (one pixel of halo), from a 22 x 38 x 3
//            image patch in LDS.  Plain fp32 FMA, not the matrix cores: wave w computes output channels 4w .. 4w + 3 (its weights come
//            from LDS, one address per wave: broadcast reads), a lane one pooled position = the 2 x 2 conv0 pixels under it from the 4 x 4 x 3 image values it
//            loads once (432 FMAs on 48 loaded values).  y = acc * scale + shift, leaky, ONE rounding to the plan's format (where the unfused
//            pipeline stores conv0), then the max of the four in y3_maxpool2x2's order; the four conv0 values never leave registers.  A
//            pooled position outside the image is conv1's zero padding: written as an exact 0, never computed.  conv0's own zero padding is
//            the zeros of the image patch.  Recompute: 720 conv0 pixels per 512 consumed = 1.41 x a layer of 2.7 % of the network's FLOPs.
//   phase 2  conv1 as an implicit GEMM 128 pixels x 32 channels x K = 144 with the A operand read from the pooled patch in LDS and the B
//            operand (all of conv1's weights) resident in registers (16-bit; 36 per lane) or in LDS (fp32): wave w takes conv1 rows 2w, 2w + 1 of the tile.  fp32: 72
//            v_mfma_f32_32x32x2_f32; 16-bit: 9 v_mfma_f32_32x32x16_bf16 / _f16, one tap of 16 channels each, N = 32 exactly.  GEMM row
//            m = 4 * window + 2 dy + dx, so the four conv1 pixels of a pool-1 window are accumulator elements 4i .. 4i + 3 of ONE lane:
//            y = acc * scale + shift, leaky, one rounding to the plan's format, and pool 1 is three compares in registers.  The lane stores
//            its four windows' values of channel n (32 lanes = one pixel's 32 channels, contiguous).
// Both pools compare values and keep the winner's bits, after BN and leaky (a BN scale may be negative or zero); there is no running maximum
// with a start value.  Rounding is monotone, so the maximum of the rounded values is what the unfused op order stores.
//
// LDS (fp32: 41,712 B; 16-bit: 17,520 B per workgroup; launch bound 256 threads x 2 per SIMD; see profiles/tiny_stem_resources.txt):
//   patch  180 positions x 16 channels: 64 B (fp32) / 32 B (16-bit) per position, position (py, px) at index py * 18 + px, its 16-B chunk c
//          stored at chunk c ^ ((px >> 1) & 3) (fp32, four chunks) / c ^ ((px >> 1) & 1) (16-bit, two).  Phase 2 reads it with ds_read_b128:
//          lane fr of a half-wave reads position (2w + dy + u, 2 win + dx + v), win = fr >> 2; within each of the instruction's 16-lane
//          groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) the sixteen (position, chunk) pairs then fall into sixteen
//          different 4-bank columns for every tap, wave and chunk: conflict free (checked exhaustively over taps, waves, chunks and groups).
//          Phase 1 writes one ds_write_b128 (fp32) / ds_write_b64 (16-bit) per lane and position.
//   img    22 x 38 x 3 floats, [row][column][channel].  Phase 1 reads a lane's 4 x 12 floats as 24 ds_read_b64 (addresses are multiples of
//          24 B); lanes along a pooled row are 6 floats apart, so the 32 lanes of a ds_read_b64 group cover the 64 banks once (a lane group
//          that wraps to the next pooled row may meet a 2-way conflict).
//   w0     conv0's weights, 27 x 16 floats.
//   w1     fp32 form only: conv1's weights [32 rows n][144], chunk kc of row n at (kc & ~3) | ((kc & 3) ^ ((n >> 2) & 3)): the sixteen lanes
//          of a ds_read_b128 group read rows whose (n & 3, (n >> 2) & 3) pairs are all different: conflict free.
// The next tile's image patch is fetched into registers before phase 2 and staged behind it.
// Scratch use is zero.  Summation order per output element -- conv0: one accumulator, taps (u, v) row-major, channel c inside, the order of
// conv_first.hip; conv1: one accumulator, taps row-major, inside a tap the MFMA's own order (fp32: channels 8h + j, j = 0 .. 7, the two lane
// halves h alternating inside each instruction) -- is the same for every pixel, image, batch size and lane.  Offsets into the image batch and
// the output are size_t.  The kernel only enqueues: it runs per lane slice and inside a captured graph.
#include <type_traits>

#include "conv_common.h"

namespace y3 {

namespace tstem {
constexpr int TH = 4, TW = 8;                     // pool-1 pixels per tile
constexpr int PH = 2 * TH + 2, PW = 2 * TW + 2;   // pooled patch (conv1's input with halo): 10 x 18
constexpr int IH = 2 * PH + 2, IW = 2 * PW + 2;   // image patch: 22 x 38
constexpr int C0 = 16, C1 = 32;
constexpr int NPOS = PH * PW;                     // 180
constexpr int IMG_F = IH * IW * 3;                // 2508 floats
constexpr int NT = 256;
constexpr int ROUNDS = (NPOS + 63) / 64;          // 3: pooled positions per lane in phase 1
constexpr int IMG_PER_THREAD = (IMG_F + NT - 1) / NT;   // 10
constexpr int WG_PER_CU = kTinyStemWgPerCu;       // persistent workgroups per CU the grid is sized for (4; y3_kernels.h)
struct F32 {};                                    // element tag of the fp32 form (the 16-bit forms: Bf16Elem, F16Elem)
template <class E> constexpr int elem_bytes() { return std::is_same_v<E, F32> ? 4 : 2; }
constexpr int W0_F = 27 * C0;                     // conv0's weights: 432 floats
constexpr int K1 = 9 * C0;                        // 144
constexpr int W1_F = C1 * K1;                     // conv1's weights in LDS, the fp32 form only: 4608 floats
template <class E> constexpr int lds_bytes() { return NPOS * C0 * elem_bytes<E>() + (IMG_F + W0_F + (std::is_same_v<E, F32> ? W1_F : 0)) * 4; }

// the value as the plan's format holds it
template <class E> __device__ __forceinline__ float round_to(float v)
{
    if constexpr (std::is_same_v<E, F32>) return v;
    else return (float)(typename E::elem)v;
}
// the larger of two values, the first on a tie (max_word of maxpool.hip)
__device__ __forceinline__ float max_keep(float a, float b) { return b > a ? b : a; }
// 2x2 window {a c / d e} = {(y0, x0) (y0, x1) / (y1, x0) (y1, x1)} in maxpool2x2_kernel's order
__device__ __forceinline__ float pool4(float a, float c, float d, float e) { return max_keep(max_keep(a, c), max_keep(d, e)); }
}  // namespace tstem

template <class E>
__device__ __forceinline__ void conv_tiny_stem_body(const TinyStemArgs &p)
{
    using namespace tstem;
    constexpr bool IS32 = std::is_same_v<E, F32>;
    constexpr int EB = elem_bytes<E>();
    constexpr int POS_B = C0 * EB;                // bytes per pooled position: 64 / 32
    constexpr int PATCH_B = NPOS * POS_B;
    extern __shared__ __attribute__((aligned(16))) unsigned char tiny_smem[];
    char *lds = reinterpret_cast<char *>(tiny_smem);
    float *imgs = reinterpret_cast<float *>(tiny_smem + PATCH_B);
    float *w0s = imgs + IMG_F;                    // conv0's weights [27][16]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;

    // ---- once per workgroup ----
    // conv0's weights into LDS; this wave reads its four output channels of row k at w0 + 16 k, one address for the whole wave (a broadcast)
    for (int i = tid; i < W0_F; i += NT) w0s[i] = p.w0[i];
    const float *w0 = w0s + 4 * wave;
    float sc0[4], sh0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sc0[j] = p.scale0[4 * wave + j];
        sh0[j] = p.shift0[4 * wave + j];
    }
    // conv1's B operand in registers: lane (n = fr, half fh) holds w1[tap * 16 + 8 fh + j][n], j = 0 .. 7, of every tap
    typename std::conditional_t<IS32, Bf16Elem, E>::frag wh[IS32 ? 1 : 9];
    float *w1s = w0s + W0_F;                      // fp32 form: conv1's weights in LDS (72 registers per lane would not leave two waves per SIMD)
    int bw[2] = {0, 0};                           // ... and the byte addresses of this lane's two chunks of a tap, without the tap's immediate
    if constexpr (IS32) {
        // [n][144], the 16-B chunk kc (four channels of a tap; four chunks per tap) of row n stored at (kc & ~3) | ((kc & 3) ^ ((n >> 2) & 3))
        const float *w1 = static_cast<const float *>(p.w1);
        for (int g = tid; g < W1_F; g += NT) {
            const int k = g / C1, n = g - k * C1;   // consecutive threads read consecutive n of one row k of [144][32]
            const int kc = k >> 2;
            w1s[n * K1 + ((kc & ~3) | ((kc & 3) ^ ((n >> 2) & 3))) * 4 + (k & 3)] = w1[g];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
            bw[i] = static_cast<int>(reinterpret_cast<char *>(w1s) - lds) + fr * (K1 * 4) + (((2 * fh + i) ^ ((fr >> 2) & 3)) << 4);
    } else {
        const unsigned short *w1 = static_cast<const unsigned short *>(p.w1);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) wh[t][j] = __builtin_bit_cast(typename E::elem, w1[(t * C0 + 8 * fh + j) * C1 + fr]);
    }
    const float sc1 = p.scale1[fr], sh1 = p.shift1[fr];

    // phase 2, per lane: GEMM row fr = 4 win + 2 dy + dx -> conv1 pixel (2 wave + dy, 2 win + dx) of the tile; tap (u, v) reads patch
    // position (2 wave + dy + u, 2 win + dx + v), whose swizzle key is ((2 win + dx + v) >> 1) = win + ((dx + v) >> 1)
    const int win = fr >> 2, dy = (fr >> 1) & 1, dx = fr & 1;
    const int abase = ((2 * wave + dy) * PW + 2 * win + dx) * POS_B;
    int a2[3][IS32 ? 2 : 1];                      // [v][chunk of the lane's two (fp32)]: byte address without the tap's immediate
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const int key = win + ((dx + v) >> 1);
        if constexpr (IS32) {
            a2[v][0] = abase + (((2 * fh) ^ (key & 3)) << 4);
            a2[v][1] = abase + (((2 * fh + 1) ^ (key & 3)) << 4);
        } else {
            a2[v][0] = abase + ((fh ^ (key & 1)) << 4);
        }
    }

    const int H = p.H, W = p.W, Hp = p.H >> 1, Wp = p.W >> 1, Ho = p.H >> 2, Wo = p.W >> 2;
    const int tiles_per_img = p.tiles_y * p.tiles_x;

    // image patch of a tile: element i of the 22 x 38 x 3 patch <- image (iy0 + i / 114, ix0 + (i % 114) / 3, channel); positions outside
    // the image are 0 (conv0's 'same' padding)
    float rimg[IMG_PER_THREAD];
    auto img_fetch = [&](int tile) {
        const int b = tile / tiles_per_img, t2 = tile - b * tiles_per_img;
        const int ty = t2 / p.tiles_x, tx = t2 - ty * p.tiles_x;
        const int iy0 = 4 * TH * ty - 3, ix0 = 4 * TW * tx - 3;
#pragma unroll
        for (int i = 0; i < IMG_PER_THREAD; ++i) {
            const int e = tid + i * NT;
            const int iy = e / (IW * 3), rem = e - iy * (IW * 3);
            const int ix = rem / 3, c = rem - ix * 3;
            const int gy = iy0 + iy, gx = ix0 + ix;
            const bool ok = e < IMG_F && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
            rimg[i] = ok ? p.img[(((size_t)b * H + gy) * W + gx) * 3 + c] : 0.0f;
        }
    };
    auto img_stage = [&]() {
#pragma unroll
        for (int i = 0; i < IMG_PER_THREAD; ++i)
            if (tid + i * NT < IMG_F) imgs[tid + i * NT] = rimg[i];
    };

    int tile = blockIdx.x;
    if (tile < p.n_tiles) {
        img_fetch(tile);
        img_stage();
    }
    __syncthreads();

    for (; tile < p.n_tiles; tile += gridDim.x) {
        const int b = tile / tiles_per_img, t2 = tile - b * tiles_per_img;
        const int ty = t2 / p.tiles_x, tx = t2 - ty * p.tiles_x;

        // ================= phase 1: conv0 + pool 0 into the pooled patch =================
#pragma unroll 1
        for (int r = 0; r < ROUNDS; ++r) {
            // pooled position pos = lane + 64 r -> (py, px) (the lanes past 180 in the last round compute position 0 and store nothing);
            // the image patch offset of its window's first value; the patch byte address of this wave's four channels
            const int pos = lane + 64 * r;
            const int pc = pos < NPOS ? pos : 0;
            const int py = pc / PW, px = pc - py * PW;
            const float *xp = imgs + (2 * py * IW + 2 * px) * 3;
            int wadr;
            if constexpr (IS32) wadr = pc * POS_B + ((wave ^ ((px >> 1) & 3)) << 4);
            else wadr = pc * POS_B + (((wave >> 1) ^ ((px >> 1) & 1)) << 4) + (wave & 1) * 8;
            float x[4][12];                        // the window's 4 x 4 pixels x 3 channels
#pragma unroll
            for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const f32x2 t = *reinterpret_cast<const f32x2 *>(xp + yy * IW * 3 + 2 * k);
                    x[yy][2 * k] = t[0];
                    x[yy][2 * k + 1] = t[1];
                }
            float acc[4][4];                       // [conv0 pixel q = 2 dy + dx of the window][channel]
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[q][j] = 0.0f;
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int v = 0; v < 3; ++v)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const f32x4 wv = *reinterpret_cast<const f32x4 *>(w0 + ((u * 3 + v) * 3 + c) * C0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float xv = x[(q >> 1) + u][((q & 1) + v) * 3 + c];
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[q][j] = __builtin_fmaf(xv, wv[j], acc[q][j]);
                        }
                    }
            // pooled position in pool 0's grid: outside it the position is conv1's zero padding
            const int gy = 2 * TH * ty - 1 + py, gx = 2 * TW * tx - 1 + px;
            const bool inside = (unsigned)gy < (unsigned)Hp && (unsigned)gx < (unsigned)Wp;
            float pooled[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float y[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = acc[q][j] * sc0[j] + sh0[j];
                    if (p.leaky0) v = fmaxf(v, 0.1f * v);
                    y[q] = round_to<E>(v);
                }
                pooled[j] = inside ? pool4(y[0], y[1], y[2], y[3]) : 0.0f;
            }
            if (pos < NPOS) {
                if constexpr (IS32) {
                    *reinterpret_cast<f32x4 *>(lds + wadr) = f32x4{pooled[0], pooled[1], pooled[2], pooled[3]};
                } else {
                    const unsigned lo = (unsigned)E::bits(pooled[0]) | ((unsigned)E::bits(pooled[1]) << 16);
                    const unsigned hi = (unsigned)E::bits(pooled[2]) | ((unsigned)E::bits(pooled[3]) << 16);
                    *reinterpret_cast<uint2 *>(lds + wadr) = uint2{lo, hi};
                }
            }
        }
        __syncthreads();   // pooled patch complete; the image patch is free

        // the next tile's image patch: in flight during phase 2, staged before the closing barrier
        const int next = tile + gridDim.x;
        if (next < p.n_tiles) img_fetch(next);

        // ================= phase 2: conv1 from the pooled patch =================
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int imm = (u * PW + v) * POS_B;
                const int t = u * 3 + v;
                if constexpr (IS32) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const f32x4 fa = *reinterpret_cast<const f32x4 *>(lds + a2[v][i] + imm);
                        const f32x4 fb = *reinterpret_cast<const f32x4 *>(lds + bw[i] + t * 64);
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[k], fb[k], acc, 0, 0, 0);
                    }
                } else {
                    using frag = typename E::frag;
                    const frag fa = *reinterpret_cast<const frag *>(lds + a2[v][0] + imm);
                    acc = E::mfma32(fa, wh[t], acc);
                }
            }

        // ---- epilogue + pool 1: elements 4 i .. 4 i + 3 of this lane are the 2 x 2 window 2 i + fh of pool-1 row `wave`, channel fr ----
        {
            const int oy = ty * TH + wave;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float y[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = acc[4 * i + q] * sc1 + sh1;
                    if (p.leaky1) v = fmaxf(v, 0.1f * v);
                    y[q] = round_to<E>(v);
                }
                const float m = pool4(y[0], y[1], y[2], y[3]);
                const int ox = tx * TW + 2 * i + fh;
                const size_t off = (((size_t)b * Ho + oy) * Wo + ox) * C1 + fr;
                if (oy < Ho && ox < Wo) {
                    if constexpr (IS32) static_cast<float *>(p.dst)[off] = m;
                    else static_cast<unsigned short *>(p.dst)[off] = E::bits(m);
                }
            }
        }
        if (next < p.n_tiles) img_stage();
        __syncthreads();   // every wave is done reading the pooled patch; the next image patch is in place
    }
}

__global__ __launch_bounds__(tstem::NT, 2) void conv_tiny_stem_f32(const TinyStemArgs p) { conv_tiny_stem_body<tstem::F32>(p); }

template <class E>
__global__ __launch_bounds__(tstem::NT, 2) void conv_tiny_stem16(const TinyStemArgs p) { conv_tiny_stem_body<E>(p); }

template <class E, class KERNEL>
static hipError_t launch_conv_tiny_stem(KERNEL kernel, const TinyStemArgs &a, hipStream_t s)
{
    using namespace tstem;
    if (a.H <= 0 || a.W <= 0 || a.H % 32 || a.W % 32 || a.B <= 0 || !a.img || !a.w0 || !a.scale0 || !a.shift0 || !a.w1 || !a.scale1 || !a.shift1 || !a.dst)
        return hipErrorInvalidValue;
    TinyStemArgs p = a;
    p.tiles_y = (a.H / 4) / TH;
    p.tiles_x = (a.W / 4) / TW;
    const long long n = (long long)a.B * p.tiles_y * p.tiles_x;
    if (n > 0x7fffffffll) return hipErrorInvalidValue;
    p.n_tiles = (int)n;
    const int cus = a.n_cus > 0 ? a.n_cus : 256;                // read once at plan time (y3_net_plan)
    const int grid = persistent_stem_grid(p.n_tiles, WG_PER_CU, cus);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), lds_bytes<E>(), s, p);
    return hipGetLastError();
}

hipError_t launch_conv_tiny_stem_f32(const TinyStemArgs &a, hipStream_t s) { return launch_conv_tiny_stem<tstem::F32>(conv_tiny_stem_f32, a, s); }
hipError_t launch_conv_tiny_stem_bf16(const TinyStemArgs &a, hipStream_t s) { return launch_conv_tiny_stem<Bf16Elem>(conv_tiny_stem16<Bf16Elem>, a, s); }
hipError_t launch_conv_tiny_stem_f16(const TinyStemArgs &a, hipStream_t s) { return launch_conv_tiny_stem<F16Elem>(conv_tiny_stem16<F16Elem>, a, s); }

}  // namespace y3
