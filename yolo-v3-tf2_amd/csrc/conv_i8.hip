// int8 plans (Y3_DTYPE_I8): implicit-GEMM convolution with int8 operands on the gfx950 matrix cores, exact i32 accumulate
// (v_mfma_i32_32x32x32_i8 / v_mfma_i32_16x16x64_i8: the cycles of the bf16 forms at twice the K).  A sibling of conv_16bit.h rather than a
// further element type of it: that header's instantiations keep their registers by staying untouched.  What is the same, byte for byte:
//   * activations NHWC, weights packed [CoutPad][K] (k = tap*Cin + c); an int8 tensor of C channels is a 16-bit tensor of C/2 to the copies;
//   * K tile = 128 bytes per row (128 channels), LDS-DMA only: unpadded 128-B rows, 16-B chunk XOR-swizzled (swizzled_chunk<8>), double buffered;
//   * a lane's operand is 16 bytes from row l & 31, piece 2s + (l >> 5) (32x32x32) or row l & 15, piece 4s + (l >> 4) (16x16x64) -- the places a
//     bf16 fragment comes from.  A and B take their k from the same byte offsets and integer sums do not depend on order, so whatever k
//     order the instruction gives the 16 bytes cancels;
//   * accumulator layouts (mfma32_row / mfma16_row: C/D maps do not depend on the element type).
// What differs is the epilogue ("int8 plans", the scheme kernel and NumPy restatement share):
//   v = (float)acc * sc[c] + sh[c]      two roundings, never contracted
//   v = max(v, 0.1f * v)                when leaky
//   v = (float)r * q_res + v            when there is a shortcut; r the int8 shortcut value, q_res its tensor's scale
//   q = clamp(rintf(v * q_inv), -127, 127)
// int8 output: per-wave, barrier-free LDS transposition as in conv_16bit.h, 16 channels per 16-byte piece, the shortcut read in the same
// pieces.  fp32 output (head grids): v stored as is, through the workgroup-wide fp32 tile, with the in-tile head decode available.
// No split-K, no weight-resident form, no BK = 32 tiles (include/y3.h).
#include <algorithm>
#include <type_traits>

#include "conv_common.h"

namespace y3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float bn_act_i8(int acc, float sc, float sh, int leaky)
{
    float v = (float)acc * sc + sh;
    if (leaky) v = fmaxf(v, 0.1f * v);
    return v;
}

// symmetric int8: round to nearest even, clamp to [-127, 127]
__device__ __forceinline__ int quant_i8(float v, float inv)
{
    return (int)fminf(fmaxf(rintf(v * inv), -127.0f), 127.0f);
}

// byte b (0..3) of word w as a signed value
__device__ __forceinline__ int sbyte(unsigned w, int b) { return (int)(w << (24 - 8 * b)) >> 24; }

template <int TM, int TN, int WR, int WC, bool CONCAT, bool OUT_F32, bool M16>
__global__ __launch_bounds__(64 * WR * WC) void conv_i8_mfma(const ConvArgs p)
{
    constexpr int MB = M16 ? 2 * TM : TM, NB = M16 ? 2 * TN : TN;   // accumulator blocks per wave
    using acc_t = typename std::conditional<M16, i32x4, i32x16>::type;
    constexpr int DROWS = 8;         // rows one wave DMA instruction (1 KiB) fills
    constexpr int BM = 32 * TM * WR;
    constexpr int BN = 32 * TN * WC;
    constexpr int NT = 64 * WR * WC;
    constexpr int BKB = 128;         // bytes = channels per K tile
    constexpr int LPR = 8;           // lanes per row (16 B each)
    constexpr int RP = NT / LPR;     // rows per load pass
    constexpr int AP = BM / RP, BP = BN / RP;
    static_assert(BM % RP == 0 && BN % RP == 0 && AP >= 1 && BP >= 1, "tile too small for the thread count");
    constexpr int ROWB = BKB;
    constexpr int STAGE_B = (BM + BN) * ROWB;
    constexpr int CROW = BN + 4;     // floats per row of the fp32 epilogue tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;

    const int logical = xcd_contiguous_tile(blockIdx.x, gridDim.x);
    const int tilesN = p.CoutPad / BN;
    const int mt = logical / tilesN, nt = logical - mt * tilesN;
    const int m0 = mt * BM, n0 = nt * BN;

    const __amdgpu_buffer_rsrc_t rs0 = buffer_rsrc(p.src0, p.src0_bytes);
    const __amdgpu_buffer_rsrc_t rs1 = buffer_rsrc(CONCAT ? p.src1 : p.src0, CONCAT ? p.src1_bytes : p.src0_bytes);
    const __amdgpu_buffer_rsrc_t rsw = buffer_rsrc(p.wpk, p.w_bytes);
    const unsigned OOB0 = p.src0_bytes, OOB1 = CONCAT ? p.src1_bytes : p.src0_bytes;

    const int lrow = tid / LPR;
    const int lchunk = swizzled_chunk<8>(lrow, tid % LPR) * 16;   // first byte of the logical chunk landing in physical chunk tid % LPR
    int aoff[AP];
    int aoff1[CONCAT ? AP : 1];
    int ahw[AP];
    const int C1 = p.Cin - p.C0;
    const TileOrigin org = tile_origin(p, m0);
#pragma unroll
    for (int i = 0; i < AP; ++i)
        gather_row<CONCAT, 1>(p, org, m0 + i * RP + lrow, org.wo0 + i * RP + lrow, C1, aoff[i], aoff1[CONCAT ? i : 0], ahw[i]);
    unsigned boff[BP];
#pragma unroll
    for (int j = 0; j < BP; ++j) boff[j] = (unsigned)((n0 + j * RP + lrow) * p.K + lchunk);

    const int KT = p.K / BKB;
    int tap = 0, c0 = 0;
    unsigned avoff[AP];
    unsigned avoff1[CONCAT ? AP : 1];
    auto set_tap = [&]() {
        if (CONCAT) {
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                avoff[i] = (ahw[i] < 0) ? OOB0 : (unsigned)(aoff[i] + lchunk);
                avoff1[i] = (ahw[i] < 0) ? OOB1 : (unsigned)(aoff1[i] + lchunk);
            }
        } else {
            const int u = tap / p.ksize, v = tap - u * p.ksize;
            const int toff = (u * p.W + v) * p.Cin + lchunk;
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                const int hi = (ahw[i] >> 16) + u, wi = (int)(short)(ahw[i] & 0xffff) + v;
                const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                avoff[i] = ok ? (unsigned)(aoff[i] + toff) : OOB0;
            }
        }
    };
    set_tap();

    int kglob = 0;
    auto fetch_dma = [&](int buf) {
        unsigned char *sa = smem + buf * STAGE_B + wave * DROWS * ROWB;   // wave w fills rows [pass*RP + DROWS*w, +DROWS)
        unsigned char *sb = sa + BM * ROWB;
        if (CONCAT && c0 >= p.C0) {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lds_ptr)(sa + i * RP * ROWB), 16, (int)avoff1[i], c0 - p.C0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_ptr)(sa + i * RP * ROWB), 16, (int)avoff[i], c0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < BP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sb + j * RP * ROWB), 16, (int)boff[j], kglob, 0, 0);
        kglob += BKB;
        c0 += BKB;
        if (c0 == p.Cin) {
            c0 = 0;
            ++tap;
            if (!CONCAT) set_tap();
        }
    };

    acc_t acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < (M16 ? 4 : 16); ++e) acc[i][j][e] = 0;

    fetch_dma(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int fr = M16 ? (lane & 15) : (lane & 31), fh = M16 ? (lane >> 4) : (lane >> 5);   // row in the block, k group
    const int a_frag = (wr * 32 * TM + fr) * ROWB;
    const int b_frag = BM * ROWB + (wc * 32 * TN + fr) * ROWB;
    constexpr int KS = M16 ? 2 : 4;                  // MFMA k steps per K tile: 64 / 32 bytes of k each
    constexpr int BR = M16 ? 16 : 32;                // rows per block
    int foff[KS];  // byte offset of this lane's 16-B piece of k-step s inside its row
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) foff[s_] = swizzled_chunk<LPR>(fr, (M16 ? 4 : 2) * s_ + fh) * 16;

    for (int kt = 0; kt < KT; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < KT) fetch_dma(cur ^ 1);
        const unsigned char *sa = smem + cur * STAGE_B + a_frag;
        const unsigned char *sb = smem + cur * STAGE_B + b_frag;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            i32x4 fa[MB], fb[NB];
#pragma unroll
            for (int i = 0; i < MB; ++i) fa[i] = *reinterpret_cast<const i32x4 *>(sa + i * BR * ROWB + foff[s]);
#pragma unroll
            for (int j = 0; j < NB; ++j) fb[j] = *reinterpret_cast<const i32x4 *>(sb + j * BR * ROWB + foff[s]);
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    if constexpr (M16) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
                    else acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    if constexpr (!OUT_F32) {
        // ---- int8 output: per-wave epilogue, no workgroup barrier (conv_16bit.h says why) ----------------------------------------------
        // Every wave transposes its own 32 x (32 TN) fp32 blocks through a private LDS scratch (the operand tiles are dead after the loop's
        // last barrier) and stores whole 16-byte pieces of 16 channels; the shortcut is read in the same pieces.
        constexpr int CW = 32 * TN;              // floats per scratch row = channels per wave
        constexpr int PPRW = CW / 16;            // 16-byte output pieces per row
        constexpr int NPL = 32 * PPRW / 64;      // pieces per lane per 32-row block
        float *S = reinterpret_cast<float *>(smem) + wave * (32 * CW);
        signed char *dstb = static_cast<signed char *>(p.dst);
        const signed char *res = static_cast<const signed char *>(p.residual);
        const int nw = n0 + wc * CW;             // first channel of this wave
        float sc[NB], sh[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            sc[j] = p.scale[nw + j * BR + fr];
            sh[j] = p.shift[nw + j * BR + fr];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mw = m0 + (wr * TM + i) * 32;   // first row of this block
            u32x4 rr[NPL];
            if (res) {   // shortcut operand first: its latency hides behind the accumulator write-out
#pragma unroll
                for (int it = 0; it < NPL; ++it) {
                    const int q = lane + it * 64;
                    const int r = q / PPRW, pc = q - r * PPRW;
                    rr[it] = (mw + r < p.M && nw + pc * 16 < p.Cout) ? *reinterpret_cast<const u32x4 *>(res + (size_t)(mw + r) * p.Cout + nw + pc * 16)
                                                                     : u32x4{0u, 0u, 0u, 0u};
                }
            }
            if constexpr (M16) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) S[mfma16_row(e, fh, mb) * CW + j * 16 + fr] = bn_act_i8(acc[2 * i + mb][j][e], sc[j], sh[j], p.leaky);
            } else {
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) S[mfma32_row(e, fh) * CW + j * 32 + fr] = bn_act_i8(acc[i][j][e], sc[j], sh[j], p.leaky);
            }
            // lanes read what OTHER lanes of this wave wrote: a wave's LDS operations run in order; the builtins keep the compiler from reordering
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int it = 0; it < NPL; ++it) {
                const int q = lane + it * 64;
                const int r = q / PPRW, pc = q - r * PPRW;
                u32x4 out;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(S + r * CW + pc * 16 + 4 * k);
                    unsigned w = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        float x = v[b];
                        if (res) x = (float)sbyte(rr[it][k], b) * p.q_res + x;
                        w |= ((unsigned)quant_i8(x, p.q_inv) & 0xffu) << (8 * b);
                    }
                    out[k] = w;
                }
                if (mw + r < p.M && nw + pc * 16 < p.Cout) *reinterpret_cast<u32x4 *>(dstb + (size_t)(mw + r) * p.Cout + nw + pc * 16) = out;
            }
            // ... and the next pass's writes below this pass's reads
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    } else {
        // ---- fp32 output (head grids, Cout = 255): workgroup-wide fp32 tile, one 32-row block of every wave per pass, as in conv_16bit.h ----
        constexpr int EROWS = WR * 32;
        float *C = reinterpret_cast<float *>(smem);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (i > 0) __syncthreads();   // previous pass fully read
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int nl = wc * TN * 32 + j * BR + fr;
                const float sc = p.scale[n0 + nl], sh = p.shift[n0 + nl];
                if constexpr (M16) {
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                        for (int e = 0; e < 4; ++e) C[(wr * 32 + 16 * mb + mfma16_row(e, fh)) * CROW + nl] = bn_act_i8(acc[2 * i + mb][j][e], sc, sh, p.leaky);
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) C[(wr * 32 + mfma32_row(e, fh)) * CROW + nl] = bn_act_i8(acc[i][j][e], sc, sh, p.leaky);
                }
            }
            __syncthreads();
            float *dst = static_cast<float *>(p.dst);
            if (dst != nullptr) {
                for (int idx = tid; idx < EROWS * BN; idx += NT) {
                    const int r = idx / BN, col = idx - r * BN;
                    const int m = m0 + (r >> 5) * 32 * TM + i * 32 + (r & 31), n = n0 + col;
                    if (m < p.M && n < p.Cout) dst[(size_t)m * p.Cout + n] = C[r * CROW + col];
                }
            }
            // detection head with its decode fused in (y3_net_forward_decode): the same fp32 tile, the same body as decode.hip
            if (p.dec.boxes != nullptr)
                decode_rows_from_lds<NT>(C, CROW, EROWS, [&](int r) { return m0 + (r >> 5) * 32 * TM + i * 32 + (r & 31); }, p.M, p.dec);
        }
    }
}

template <int TM, int TN, int WR, int WC, bool CONCAT, bool OUT_F32, bool M16>
static hipError_t launch_kb_i8(const ConvArgs &a, hipStream_t s)
{
    constexpr int BM = 32 * TM * WR, BN = 32 * TN * WC;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.CoutPad / BN;
    const size_t stages = 2 * (size_t)(BM + BN) * 128;
    const size_t ctile = OUT_F32 ? (size_t)WR * 32 * (BN + 4) * sizeof(float) : (size_t)WR * WC * 32 * 32 * TN * sizeof(float);
    return launch_conv_kernel<conv_i8_mfma<TM, TN, WR, WC, CONCAT, OUT_F32, M16>>(a, tilesM * tilesN, 64 * WR * WC, std::max(stages, ctile), s);
}

template <int TM, int TN, int WR, int WC, bool M16>
static hipError_t launch_tb_i8(const ConvArgs &a, bool out_f32, hipStream_t s)
{
    return dispatch_concat_out(a.src1 != nullptr, out_f32, [&](auto concat, auto f32) {
        return launch_kb_i8<TM, TN, WR, WC, decltype(concat)::value, decltype(f32)::value, M16>(a, s);
    });
}

struct TileI8 { TileInfo info; hipError_t (*launch)(const ConvArgs &, bool out_f32, hipStream_t); };
template <int TM, int TN, int WR, int WC, bool M16 = false>
static constexpr TileI8 tile_i8() { return {{32 * TM * WR, 32 * TN * WC, WR * WC, 2, 128}, launch_tb_i8<TM, TN, WR, WC, M16>}; }

// The ids of the bf16 table (conv_16bit.h) for the tiles that have an int8 form: the LDS-DMA tiles with 128-byte rows, both MFMA shapes.
// bk is in channels = bytes: 128.
static const TileI8 kTilesI8[BF16_TILE_COUNT] = {
    {}, {}, {}, {}, {}, {}, {}, {},             //  0..7: register-staged and BK = 32 tiles: no int8 form
    tile_i8<2, 2, 2, 2>(),                      //  8: 128x128
    {},
    tile_i8<2, 1, 2, 2>(),                      // 10: 128x64
    tile_i8<1, 1, 2, 2>(),                      // 11: 64x64
    tile_i8<1, 2, 2, 2>(),                      // 12: 64x128
    {}, {}, {}, {},                             // 13..16
    tile_i8<2, 2, 4, 4>(),                      // 17: 256x256, 16 waves
    {},
    tile_i8<1, 2, 4, 4>(),                      // 19: 128x256, 16 waves
    {}, {}, {}, {},                             // 20..23
    tile_i8<2, 2, 4, 4, true>(),                // 24: tile 17 on 16x16x64
    {},
    tile_i8<1, 2, 4, 4, true>(),                // 26: tile 19 on 16x16x64
    tile_i8<2, 2, 2, 2, true>(),                // 27: tile 8 on 16x16x64
    {},
    tile_i8<1, 2, 2, 2, true>(),                // 29: tile 12 on 16x16x64
    {}, {}, {}, {}, {}, {}, {},                 // 30..36
};

TileInfo conv_i8_tile_info(int tile) { return (tile >= 0 && tile < BF16_TILE_COUNT) ? kTilesI8[tile].info : TileInfo{}; }
bool conv_i8_tile_built(int tile) { return tile >= 0 && tile < BF16_TILE_COUNT && kTilesI8[tile].launch != nullptr; }

hipError_t launch_conv_i8(const ConvArgs &a, int tile, bool out_f32, hipStream_t s)
{
    if (!conv_i8_tile_built(tile)) return hipErrorInvalidValue;
    const TileInfo &t = kTilesI8[tile].info;
    if (a.dec.boxes != nullptr && (!out_f32 || t.bn < a.CoutPad)) return hipErrorInvalidValue;   // a fused head needs all its channels in one tile
    if (a.dst == nullptr && a.dec.boxes == nullptr) return hipErrorInvalidValue;
    if (!tile_fits(t, a.Cin, a.src1 ? a.C0 : -1, a.CoutPad) || a.K % 128) return hipErrorInvalidValue;
    // the int8 epilogue moves 16 channels per piece: whole 16-byte pieces of dst and of the shortcut
    if (!out_f32 && (a.Cout % 16 || ((uintptr_t)a.dst & 15) || ((uintptr_t)a.residual & 15))) return hipErrorInvalidValue;
    if (out_f32 && a.residual) return hipErrorInvalidValue;
    return kTilesI8[tile].launch(a, out_f32, s);
}

}  // namespace y3
