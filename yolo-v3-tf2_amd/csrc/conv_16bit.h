// Implicit-GEMM convolution with 16-bit operands on the gfx950 matrix cores, fp32 accumulate: the one kernel body of the bf16 plans
// (conv_bf16.hip, v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16) and of the fp16 plans (conv_f16.hip, the _f16 forms of the same two
// instructions), generic over the element traits E (Bf16Elem / F16Elem, y3_device.h).  Included by those two files and by conv_i8.hip
// (next paragraph); each of the two instantiates the tile table below for its type.  The operand lane maps, the fragments of eight elements
// and the accumulator layouts are the same for both types; the type shows in the MFMA, in the one rounding of the epilogue (E::pack2) and in
// the widening of the shortcut operand.
//
// The names (file, conv16_mfma; the tools and the records under profiles/ parse them) now stand for the kernel of 16-BYTE PIECES: a third
// element type, I8Elem (conv_i8.hip, the int8 plans), instantiates the same body.  What an operand row, a lane's fragment and an output piece
// are is counted in bytes (E::BYTES per element: EB, EPP, KROWB below), so int8 is the 128-byte-row LDS-DMA tiles at BK = 128 channels; its
// accumulators are i32 and enter bn_act through (float), and its output pieces hold 16 channels, quantised by E::quant.  The
// register-staged form and the 64-byte rows are built for the 16-bit types only (the static_asserts of the kernel).
//
// BASELINE config 5 ("bf16 MFMA fused conv+BN+LeakyReLU"): same fused op as conv_f32.hip
// (reference: core/parse_model.py:27-52,72,134,155-156) with 16-bit activations/weights in HBM and LDS.
//   * activations NHWC 16-bit, weights packed [CoutPad][K] 16-bit (k = tap*Cin + c), head outputs fp32;
//   * K tile = BK elements (BK = 64: one 128-B line per row; BK = 32 for the two Cin = 32 layers); LDS rows are
//     2*BK + 16 bytes (odd number of 16-B slots -> conflict-free ds_read_b128 of 16 different rows), double buffered;
//   * MFMA 32x32x16: lane (r = l & 31, h = l >> 5) feeds A[row r][k = 16s + 8h .. +7] as one ds_read_b128;
//   * epilogue through LDS: accumulators (+scale/shift, leaky) are written as an fp32 [BM][BN+4] tile, then every
//     thread converts 8 consecutive channels (+ 16-bit residual) and issues ONE 16-byte store -> full 128-B lines.
//
// Split-K (SPLIT = true, the low-latency plans of y3_net_set_low_latency_bf16 / _f16; tiles 11 and 12 only, instantiated by both
// files through launch_conv16_split below): gridDim.y = S, slice y walks
// K tiles [y*KT/S, (y+1)*KT/S) of the same tap-major walk and stores its raw fp32 accumulators (no epilogue, rows >= M included) straight
// from the accumulator registers into slab y of a workspace [S][Mpad][CoutPad] fp32, through the slab's own buffer resource.
// splitk_finish16, a separate launch on the same stream, adds the slabs in the order 0, 1, ..., S-1 and applies the epilogue.
// int8 (y3_net_set_low_latency_i8, conv_i8.hip: launch_conv_i8_split): the same slice launch at BK = 128 with the slab holding the raw
// i32 accumulators -- no conversion, so the split is exact at every S -- and a finish kernel of its own, splitk_finish_i8, which adds
// integers and applies the int8 epilogue.
#pragma once
#include <algorithm>
#include <type_traits>

#include "conv_common.h"

namespace y3 {

__device__ __forceinline__ u32x4 bload16(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, 0);
}

// The epilogue's arithmetic, shared by the unsplit kernel and splitk_finish16 so that equal accumulators give equal bits:
// y = acc * scale + shift (two roundings: the build never contracts them), leaky as max(y, 0.1 y) ...
__device__ __forceinline__ float bn_act(float acc, float sc, float sh, int leaky)
{
    float v = acc * sc + sh;
    if (leaky) v = fmaxf(v, 0.1f * v);
    return v;
}
// ... then eight consecutive channels: + the 16-bit shortcut widened to fp32 (when there is one), one rounding to E's format
template <class E>
__device__ __forceinline__ u32x4 add_res_pack(float (&v)[8], const u32x4 &rr, bool has_res)
{
    if (has_res) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = E::widen_lo(rr[k]) + v[2 * k];
            v[2 * k + 1] = E::widen_hi(rr[k]) + v[2 * k + 1];
        }
    }
    u32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = E::pack2(v[2 * k], v[2 * k + 1]);
    return out;
}

// DMA: operand tiles filled by direct-to-LDS buffer loads: unpadded 128-B rows, 16-B chunk index XOR-swizzled on the source
// address and on the fragment reads (swizzled_chunk, conv_common.h).
// DMA with BK = 32 (round 3): 64-B rows, a wave instruction fills 16 rows.  Half the
// LDS per stage: 128x256 / 256x128 tiles of 8 waves fit TWO workgroups per CU (MINW = 4 caps the registers at 128), so that
// one workgroup's epilogue (27 % of the bf16 conv stack, profiles/r03_ab_bf16_epilogue_probe.txt) runs beside the other's K loop.
// M16 (round 3): the same tile on v_mfma_f32_16x16x32_bf16 -- 2TM x 2TN blocks of 16x16 per wave instead of TM x TN of 32x32.
// Same LDS image, same bytes read per K tile, same MFMA cycles per FLOP; the chip holds a higher clock on this shape
// (MI355X_MICROARCH.md "DVFS give-back" item 7: 1.12-1.15 x the FLOP/s on random data).  Fragment: lane l holds k = 8 (l >> 4) ..
// + 7 of row l & 15; C: acc[mb][nb][j] = row 16 mb + 4 (l >> 4) + j, column 16 nb + (l & 15).
// Y3_STAMP / Y3_STAMP_IDS: the phase stamps of the diagnostic build, defined by conv_bf16.hip ahead of this header; nothing otherwise
#ifndef Y3_STAMP
#define Y3_STAMP(k) do { } while (0)
#define Y3_STAMP_IDS() do { } while (0)
#endif

template <class E, int TM, int TN, int WR, int WC, int BK, bool CONCAT, bool OUT_F32, bool DMA = false, int MINW = 1, bool M16 = false, bool SPLIT = false>
__global__ __launch_bounds__(64 * WR * WC, MINW) void conv16_mfma(const ConvArgs p)
{
    constexpr int EB = E::BYTES;     // bytes per element: 2, or 1 (int8)
    constexpr int EPP = 16 / EB;     // elements per 16-byte piece
    constexpr int KROWB = EB * BK;   // bytes of one row of a K tile
    static_assert(!SPLIT || (DMA && KROWB == 128 && !M16 && !OUT_F32), "the split-K form is built for the LDS-DMA 32x32 tiles with 128-byte rows (BK = 64, int8: 128)");
    Y3_STAMP(0);
    Y3_STAMP_IDS();
    static_assert(!DMA || KROWB == 128 || (KROWB == 64 && EB == 2), "LDS-DMA variant needs 128-byte rows, or 64-byte rows of 16-bit elements");
    static_assert(!M16 || (DMA && KROWB == 128), "the 16x16 form is built on the 128-byte swizzled rows");
    static_assert(EB == 2 || (EB == 1 && DMA), "the register-staged form is built for 16-bit elements only");
    constexpr int MB = M16 ? 2 * TM : TM, NB = M16 ? 2 * TN : TN;   // accumulator blocks per wave
    using acc_t = typename std::conditional<M16, typename E::acc16, typename E::acc32>::type;
    constexpr int DROWS = 1024 / KROWB;   // rows one wave DMA instruction (1 KiB) fills: 8 (128-byte rows) or 16 (64-byte rows)
    constexpr int BM = 32 * TM * WR;
    constexpr int BN = 32 * TN * WC;
    constexpr int NT = 64 * WR * WC;
    constexpr int LPR = BK / EPP;    // lanes per row (16 B each)
    constexpr int RP = NT / LPR;     // rows per load pass
    constexpr int AP = BM / RP, BP = BN / RP;
    static_assert(BM % RP == 0 && BN % RP == 0 && AP >= 1 && BP >= 1, "tile too small for the thread count");
    constexpr int ROWB = DMA ? KROWB : KROWB + 16;  // LDS row bytes
    constexpr int STAGE_B = (BM + BN) * ROWB;      // bytes per stage
    constexpr int CROW = BN + 4;                   // floats per row of the epilogue tile
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
    // first element of this lane's 16-B piece in the K tile (DMA: the logical chunk landing in physical chunk tid % LPR; 64-byte-row key written out: measured)
    const int lchunk = DMA ? (KROWB == 128 ? swizzled_chunk<8>(lrow, tid % LPR) : (tid % LPR) ^ ((lrow >> 2) & 3)) * EPP : (tid % LPR) * EPP;
    int aoff[AP];
    int aoff1[CONCAT ? AP : 1];
    int ahw[AP];
    const int C1 = p.Cin - p.C0;
    const TileOrigin org = tile_origin(p, m0);   // (b, ho, wo) of every row: conv_common.h
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        if constexpr (OUT_F32 && !CONCAT && EB == 2) {   // the 16-bit head convs: gather_row's offsets written out (through it five prologue instructions moved: measured; int8 was built on gather_row)
            const int m = m0 + i * RP + lrow;
            int b, ho, wo;
            tile_row(p, org, org.wo0 + i * RP + lrow, b, ho, wo);
            const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
            aoff[i] = ((b * p.H + hi0) * p.W + wi0) * p.Cin;
            ahw[i] = (m < p.M) ? ((hi0 << 16) | (wi0 & 0xffff)) : (int)0x80000000;
        } else gather_row<CONCAT, 1>(p, org, m0 + i * RP + lrow, org.wo0 + i * RP + lrow, C1, aoff[i], aoff1[CONCAT ? i : 0], ahw[i]);
    }
    unsigned boff[BP];
#pragma unroll
    for (int j = 0; j < BP; ++j) boff[j] = (unsigned)((n0 + j * RP + lrow) * p.K + lchunk) * (unsigned)EB;

    // K tiles of this workgroup's walk: all of them, or slice blockIdx.y of gridDim.y (starting at tile kt0 of the walk)
    const int kt0 = SPLIT ? (int)blockIdx.y * (p.K / BK) / (int)gridDim.y : 0;
    const int KT = SPLIT ? ((int)blockIdx.y + 1) * (p.K / BK) / (int)gridDim.y - kt0 : p.K / BK;
    int tap = 0, c0 = 0;
    if constexpr (SPLIT) {   // the walk's state at tile kt0 (wave-uniform); a concat slice may begin in either source: the fetch picks it from c0
        const int tpt = p.Cin / BK;
        tap = kt0 / tpt;
        c0 = (kt0 - tap * tpt) * BK;
    }
    unsigned avoff[AP];
    unsigned avoff1[CONCAT ? AP : 1];
    auto set_tap = [&]() {   // as in conv_f32x3.hip; written out in both: DESIGN.md section 4, "One row per tile"
        if (CONCAT) {
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                avoff[i] = (ahw[i] < 0) ? OOB0 : (unsigned)(aoff[i] + lchunk) * (unsigned)EB;
                avoff1[i] = (ahw[i] < 0) ? OOB1 : (unsigned)(aoff1[i] + lchunk) * (unsigned)EB;
            }
        } else {
            const int u = tap / p.ksize, v = tap - u * p.ksize;
            const int toff = (u * p.W + v) * p.Cin + lchunk;
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                const int hi = (ahw[i] >> 16) + u, wi = (int)(short)(ahw[i] & 0xffff) + v;
                const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                avoff[i] = ok ? (unsigned)(aoff[i] + toff) * (unsigned)EB : OOB0;
            }
        }
    };
    set_tap();

    int kglob = SPLIT ? kt0 * BK : 0;
    // the K walk both fetch forms end with: the next BK channels of this tap, else the next tap
    auto advance_k = [&]() {
        kglob += BK;
        c0 += BK;
        if (c0 == p.Cin) {
            c0 = 0;
            ++tap;
            if (!CONCAT) set_tap();
        }
    };

    u32x4 ra[AP], rb[BP];
    auto fetch_dma = [&](int buf) {
        unsigned char *sa = smem + buf * STAGE_B + wave * DROWS * ROWB;   // wave w fills rows [pass*RP + DROWS*w, +DROWS)
        unsigned char *sb = sa + BM * ROWB;
        if (CONCAT && c0 >= p.C0) {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lds_ptr)(sa + i * RP * ROWB), 16, (int)avoff1[i], (c0 - p.C0) * EB, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_ptr)(sa + i * RP * ROWB), 16, (int)avoff[i], c0 * EB, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < BP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sb + j * RP * ROWB), 16, (int)boff[j], kglob * EB, 0, 0);
        advance_k();
    };
    auto fetch = [&]() {
        if (CONCAT) {
            if (c0 < p.C0) {
#pragma unroll
                for (int i = 0; i < AP; ++i) ra[i] = bload16(rs0, avoff[i], c0 * EB);
            } else {
#pragma unroll
                for (int i = 0; i < AP; ++i) ra[i] = bload16(rs1, avoff1[i], (c0 - p.C0) * EB);
            }
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i) ra[i] = bload16(rs0, avoff[i], c0 * EB);
        }
#pragma unroll
        for (int j = 0; j < BP; ++j) rb[j] = bload16(rsw, boff[j], kglob * EB);
        advance_k();
    };
    auto stage = [&](int buf) {
        unsigned char *sa = smem + buf * STAGE_B;
        unsigned char *sb = sa + BM * ROWB;
#pragma unroll
        for (int i = 0; i < AP; ++i) *reinterpret_cast<u32x4 *>(sa + (i * RP + lrow) * ROWB + lchunk * EB) = ra[i];
#pragma unroll
        for (int j = 0; j < BP; ++j) *reinterpret_cast<u32x4 *>(sb + (j * RP + lrow) * ROWB + lchunk * EB) = rb[j];
    };

    acc_t acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < (M16 ? 4 : 16); ++e) acc[i][j][e] = 0;

    Y3_STAMP(1);
    if (DMA) {
        fetch_dma(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        fetch();
        stage(0);
    }
    __syncthreads();
    Y3_STAMP(2);

    const int fr = M16 ? (lane & 15) : (lane & 31), fh = M16 ? (lane >> 4) : (lane >> 5);   // row in the block, k group
    const int a_frag = (wr * 32 * TM + fr) * ROWB + (DMA ? 0 : fh * 16);
    const int b_frag = BM * ROWB + (wc * 32 * TN + fr) * ROWB + (DMA ? 0 : fh * 16);
    constexpr int KS = M16 ? KROWB / 64 : KROWB / 32;   // MFMA k steps per K tile: 64 / 32 bytes of k each
    constexpr int BR = M16 ? 16 : 32;                // rows per block
    int foff[KS];  // byte offset of this lane's 16-B piece of k-step s inside its row
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_)
        foff[s_] = DMA ? swizzled_chunk<LPR>(fr, (M16 ? 4 : 2) * s_ + fh) * 16 : s_ * 32;

    for (int kt = 0; kt < KT; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < KT) {
            if (DMA) fetch_dma(cur ^ 1); else fetch();
        }
        const unsigned char *sa = smem + cur * STAGE_B + a_frag;
        const unsigned char *sb = smem + cur * STAGE_B + b_frag;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            typename E::frag fa[MB], fb[NB];
#pragma unroll
            for (int i = 0; i < MB; ++i) fa[i] = *reinterpret_cast<const typename E::frag *>(sa + i * BR * ROWB + foff[s]);
#pragma unroll
            for (int j = 0; j < NB; ++j) fb[j] = *reinterpret_cast<const typename E::frag *>(sb + j * BR * ROWB + foff[s]);
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    if constexpr (M16) acc[i][j] = E::mfma16(fa[i], fb[j], acc[i][j]);
                    else acc[i][j] = E::mfma32(fa[i], fb[j], acc[i][j]);
                }
        }
        if (DMA) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (kt + 1 < KT) {
            stage(cur ^ 1);
        }
        __syncthreads();
    }

    Y3_STAMP(3);
    // ---- epilogue through LDS, one 32-row sub-tile of every wave per pass ----------------------------------
    // pass i: wave (wr, wc) writes rows [wr*32, +32) x cols [wc*32*TN, +32*TN) of a [WR*32][BN+4] fp32 tile (its i-th
    // accumulator row block), then all threads convert 8 consecutive channels each and store 16 B.
    if constexpr (SPLIT) {
        // raw accumulators -> slab blockIdx.y, straight from the registers: p.dst is the workspace, p.dst_bytes the bytes of ONE slab
        // [Mpad][CoutPad] (Mpad = whole tiles, so every row of the tile has its place; the range check of the slab's own buffer resource
        // drops anything else).  A store instruction writes two rows of 32 consecutive floats (int8: raw i32 sums): whole 128-byte lines.
        const __amdgpu_buffer_rsrc_t rss = buffer_rsrc(static_cast<const char *>(p.dst) + (size_t)blockIdx.y * p.dst_bytes, p.dst_bytes);
        const int slab_row_bytes = p.CoutPad * 4;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wc * TN + j) * 32 + fr;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mbase = m0 + (wr * TM + i) * 32 + 4 * fh;
                const unsigned vbase = (unsigned)(mbase * p.CoutPad + n) * 4u;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    unsigned bits;   // int8: the i32 sum itself (a partial sum beyond 2^24 has no float), else the fp32 accumulator
                    if constexpr (EB == 1) bits = (unsigned)acc[i][j][e];
                    else bits = __builtin_bit_cast(unsigned, (float)acc[i][j][e]);
                    __builtin_amdgcn_raw_buffer_store_b32(bits, rss, (int)vbase, mfma32_row(e) * slab_row_bytes, 0);
                }
            }
        }
    } else if constexpr (!OUT_F32) {
        // ---- output in the element type: per-wave epilogue, no workgroup barrier ------------------------------------------
        // Every wave transposes its own 32 x (32 TN) fp32 blocks through a private LDS scratch (the operand tiles are dead
        // after the loop's last barrier) and stores whole 16-byte pieces of EPP channels (8, int8: 16): 16-bit rows of 64 TN
        // bytes per wave, full 128-B lines for TN >= 2.  LDS operations of one wave execute in order, so the write -> read
        // hand-off between its lanes needs no barrier, and a wave leaves as soon as ITS stores are issued.  The shortcut is added
        // in fp32 before the single rounding to the element type (the oracle's bf16 mode rounds where the pipeline stores);
        // int8 (conv_i8.hip has the scheme): the shortcut value times its tensor's scale, then E::quant, four bytes a word.
        // (round 3: the workgroup-wide fp32 tile + 2 barriers per pass this replaces cost 27 % of the bf16 conv stack,
        // profiles/r03_ab_bf16_epilogue_probe.txt)
        constexpr int CW = 32 * TN;              // floats per scratch row = channels per wave
        constexpr int PPRW = CW / EPP;            // 16-byte output pieces per row
        constexpr int NPL = 32 * PPRW / 64;      // pieces per lane per 32-row block
        float *S = reinterpret_cast<float *>(smem) + wave * (32 * CW);
        typename E::stored *dstb = static_cast<typename E::stored *>(p.dst);
        const typename E::stored *res = static_cast<const typename E::stored *>(p.residual);
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
            // (round 5: all TM passes' shortcut loads requested up front, so that none queues behind a pass's stores, measured 0.6 % SLOWER,
            // profiles/r05_ab_bf16_shortcut_hoist.txt: 64 loads per CU in flight at once instead of 32 twice)
            if (res) {   // shortcut operand first: its latency hides behind the accumulator write-out
#pragma unroll
                for (int it = 0; it < NPL; ++it) {
                    const int q = lane + it * 64;
                    const int r = q / PPRW, pc = q - r * PPRW;
                    // int8 asks Cout % 16 only, so a wave's last pieces may lie past Cout: its column guard, here and at the store, is one
                    // condition with a constant term (a bool narrowed under if constexpr moved the 20 int8-output instantiations: measured)
                    rr[it] = (mw + r < p.M && (EB == 2 || nw + pc * EPP < p.Cout)) ? *reinterpret_cast<const u32x4 *>(res + (size_t)(mw + r) * p.Cout + nw + pc * EPP)
                                                                                    : u32x4{0u, 0u, 0u, 0u};
                }
            }
            if constexpr (M16) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            S[mfma16_row(e, fh, mb) * CW + j * 16 + fr] = bn_act((float)acc[2 * i + mb][j][e], sc[j], sh[j], p.leaky);
                        }
            } else {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        S[mfma32_row(e, fh) * CW + j * 32 + fr] = bn_act((float)acc[i][j][e], sc[j], sh[j], p.leaky);
                    }
                }
            }
            // lanes read what OTHER lanes of this wave wrote: the hardware runs a wave's LDS operations in order, and these three
            // builtins (no instructions) keep the compiler from moving the reads above the writes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int it = 0; it < NPL; ++it) {
                const int q = lane + it * 64;
                const int r = q / PPRW, pc = q - r * PPRW;
                u32x4 out;
                if constexpr (EB == 2) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(S + r * CW + pc * 8);
                    const f32x4 v1 = *reinterpret_cast<const f32x4 *>(S + r * CW + pc * 8 + 4);
                    float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    out = add_res_pack<E>(v, rr[it], res != nullptr);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const f32x4 v = *reinterpret_cast<const f32x4 *>(S + r * CW + pc * EPP + 4 * k);
                        unsigned w = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            float x = v[b];
                            if (res) x = (float)E::sbyte(rr[it][k], b) * p.q_res + x;
                            w |= ((unsigned)E::quant(x, p.q_inv) & 0xffu) << (8 * b);
                        }
                        out[k] = w;
                    }
                }
                if (mw + r < p.M && (EB == 2 || nw + pc * EPP < p.Cout)) *reinterpret_cast<u32x4 *>(dstb + (size_t)(mw + r) * p.Cout + nw + pc * EPP) = out;
            }
            // ... and the next pass's writes below this pass's reads
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        Y3_STAMP(4);   // thread 0 = wave 0: its own stores issued (not yet retired)
    } else {
        // ---- fp32 output (head grids, Cout = 255): workgroup-wide fp32 tile, one 32-row block of every wave per pass, as in conv_f32x3.hip ----
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
                        for (int e = 0; e < 4; ++e) {
                            C[(wr * 32 + 16 * mb + mfma16_row(e, fh)) * CROW + nl] = bn_act((float)acc[2 * i + mb][j][e], sc, sh, p.leaky);
                        }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        C[(wr * 32 + mfma32_row(e, fh)) * CROW + nl] = bn_act((float)acc[i][j][e], sc, sh, p.leaky);
                    }
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
            // detection head with its decode fused in (y3_net_forward_decode; the launcher guarantees a tile that spans all
            // 3 * (5 + nc) channels): the EROWS pixels of this pass are decoded from the fp32 tile in LDS, same body as decode.hip
            if (p.dec.boxes != nullptr)
                decode_rows_from_lds<NT>(C, CROW, EROWS, [&](int r) { return m0 + (r >> 5) * 32 * TM + i * 32 + (r & 31); }, p.M, p.dec);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Round-3 record (code removed again): a PERSISTENT form of this kernel -- workgroups walking tiles bid, bid + G, ...,
// the next tile's first K tile prefetched before the epilogue, a counted s_waitcnt leaving the tile's stores in flight --
// was built to hide the output stores (profiles/r03_ab_bf16_epilogue_probe.txt: the stores alone cost 20 % of the bf16
// conv stack: 10.0 ms with them, 8.0 without).  Bit-identical, 34 bf16 parity tests green, and 10 % SLOWER (11.09 vs
// 10.07 ms, profiles/r03_ab_bf16_persistent.txt).  Two facts defeat it: (1) memory operations retire in issue order, so the
// first wait for a K tile issued after the stores waits for the stores as well -- they can overlap one K iteration
// (~1 us), not a tile; (2) with one workgroup per CU (128 KB of LDS) and equal work per tile all 256 workgroups store at
// the same moment: a 32 MB burst, 4 MB per XCD = the whole L2, which drains at the HBM write rate (~8 us) while HBM idles
// during the K loops.  What would help is out-of-phase workgroups (two per CU), which this tile's LDS and register
// budget do not admit.
// ---------------------------------------------------------------------------------------------------------
// Round-2 record (code removed in round 4): a pipelined 256x256x64 tile (id 20) with the K loop of the guide's "256^2 8-phase
// template" (LDS-DMA loads in flight across raw s_barriers, counted vmcnt, the second M half of the waves one barrier behind
// the first) was correct on the first build and 10-15 % SLOWER than the 16-wave two-phase tile 17
// (profiles/r02_tile_sweep_bf16_pipelined_b128_s416.txt, r02_bf16_pipelined_tile_pmc.txt: MFMA busy 0.45 vs 0.58).
// ---------------------------------------------------------------------------------------------------------
template <class E, int TM, int TN, int WR, int WC, int BK, bool CONCAT, bool OUT_F32, bool DMA, int MINW, bool M16>
static hipError_t launch_kb(const ConvArgs &a, hipStream_t s)
{
    constexpr int BM = 32 * TM * WR, BN = 32 * TN * WC;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.CoutPad / BN;
    const size_t stages = 2 * (size_t)(BM + BN) * (DMA ? E::BYTES * BK : E::BYTES * BK + 16);
    // epilogue: fp32 output -> one workgroup-wide 32-row block per wave row; output in the element type -> 32 x (32 TN) floats per wave
    const size_t ctile = OUT_F32 ? (size_t)WR * 32 * (BN + 4) * sizeof(float) : (size_t)WR * WC * 32 * 32 * TN * sizeof(float);
    return launch_conv_kernel<conv16_mfma<E, TM, TN, WR, WC, BK, CONCAT, OUT_F32, DMA, MINW, M16>>(a, tilesM * tilesN, 64 * WR * WC,
                                                                                                 std::max(stages, ctile), s);
}

template <class E, int TM, int TN, int WR, int WC, int BK, bool DMA, int MINW, bool M16>
static hipError_t launch_tb(const ConvArgs &a, bool out_f32, hipStream_t s)
{
    return dispatch_concat_out(a.src1 != nullptr, out_f32, [&](auto concat, auto f32) {
        return launch_kb<E, TM, TN, WR, WC, BK, decltype(concat)::value, decltype(f32)::value, DMA, MINW, M16>(a, s);
    });
}

// One row per tile id: the geometry, read off the template arguments (the kernel is always double buffered), and the launcher of that
// instantiation for element type E; a retired id is an empty row.
struct Tile16 { TileInfo info; hipError_t (*launch)(const ConvArgs &, bool out_f32, hipStream_t); };
template <class E, int TM, int TN, int WR, int WC, int BK, bool DMA = false, int MINW = 1, bool M16 = false>
static constexpr Tile16 tile() { return {{32 * TM * WR, 32 * TN * WC, WR * WC, 2, BK}, launch_tb<E, TM, TN, WR, WC, BK, DMA, MINW, M16>}; }

// weight-resident 3x3 / stride 1, Cin = 32 / 64 (conv_res_16bit.h): 4 x 32 pixels x 64 channels per workgroup tile; stores 16-bit only
template <class E> hipError_t launch_res_of(const ConvArgs &a, hipStream_t s);
template <> inline hipError_t launch_res_of<Bf16Elem>(const ConvArgs &a, hipStream_t s) { return launch_conv_res_bf16(a, s); }
template <> inline hipError_t launch_res_of<F16Elem>(const ConvArgs &a, hipStream_t s) { return launch_conv_res_f16(a, s); }
template <class E>
static hipError_t launch_res(const ConvArgs &a, bool out_f32, hipStream_t s)
{
    return (!out_f32 && conv_res_bf16_fits(a)) ? launch_res_of<E>(a, s) : hipErrorInvalidValue;
}

// Ids are stable (tuning files refer to them) and the same for both element types.  The table holds exactly the tiles a plan can select --
// a packaged tuning table (tuning/bf16_*.json), the library's heuristic or the head-decode fallback (choose_tile_bf16 / refine_bf16 in
// y3_net.cpp) names every one of them (tests/test_abi.py); the other ids are retired.  I8Elem has a table of its own under the same ids
// (an explicit specialisation, conv_i8.hip).
template <class E> struct Tiles16 { static const Tile16 table[BF16_TILE_COUNT]; };
template <class E> const Tile16 Tiles16<E>::table[BF16_TILE_COUNT] = {
    tile<E, 2, 2, 2, 2, 64>(),                  //  0: 128x128
    {}, {},
    tile<E, 1, 1, 2, 2, 64>(),                  //  3: 64x64
    tile<E, 1, 1, 4, 1, 64>(),                  //  4: 128x32
    tile<E, 2, 1, 2, 2, 32>(),                  //  5: 128x64, BK 32 (Cin = 32 layers)
    tile<E, 1, 1, 2, 2, 32>(),                  //  6: 64x64, BK 32
    {},
    tile<E, 2, 2, 2, 2, 64, true>(),            //  8: 128x128 LDS-DMA
    {},
    tile<E, 2, 1, 2, 2, 64, true>(),            // 10: 128x64 LDS-DMA
    tile<E, 1, 1, 2, 2, 64, true>(),            // 11: 64x64 LDS-DMA
    tile<E, 1, 2, 2, 2, 64, true>(),            // 12: 64x128 LDS-DMA
    {}, {}, {}, {},                             // 13..16
    tile<E, 2, 2, 4, 4, 64, true>(),            // 17: 256x256, 16 waves, LDS-DMA
    {},
    tile<E, 1, 2, 4, 4, 64, true>(),            // 19: 128x256, 16 waves, LDS-DMA
    {}, {},                                     // 20 (the pipelined tile of round 2, see above), 21
    tile<E, 2, 2, 4, 2, 32, true, 4>(),         // 22: 256x128, 8 waves, LDS-DMA with BK 32, two workgroups per CU
    {},
    tile<E, 2, 2, 4, 4, 64, true, 1, true>(),   // 24: tile 17 on 16x16x32 MFMAs
    {},
    tile<E, 1, 2, 4, 4, 64, true, 1, true>(),   // 26: tile 19 on 16x16x32
    tile<E, 2, 2, 2, 2, 64, true, 1, true>(),   // 27: tile 8 (128x128, 4 waves) on 16x16x32
    {},
    tile<E, 1, 2, 2, 2, 64, true, 1, true>(),   // 29: tile 12 (64x128, 4 waves) on 16x16x32
    {}, {},                                     // 30, 31
    {{128, 64, 8, 2, 32}, launch_res<E>},       // 32
    // 33..35 (3x3 / stride 1 with tap-row reuse) and 36 (256x256 on four waves of 128x128, hand-pipelined): parity-green, neutral / slower in the
    // two-lane step (profiles/r04_ab_bf16_rs.txt, r04_tile_sweep_bf16_w4.txt); code in the history (commit 1777145)
    {}, {}, {}, {},
};

// The unsplit launch of tile id `tile` for element type E (launch_conv_bf16 / launch_conv_f16)
template <class E>
static hipError_t launch_conv16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s)
{
    if (tile < 0 || tile >= BF16_TILE_COUNT || !Tiles16<E>::table[tile].launch) return hipErrorInvalidValue;
    const TileInfo &t = Tiles16<E>::table[tile].info;
    if (a.dec.boxes != nullptr && (!out_f32 || t.bn < a.CoutPad)) return hipErrorInvalidValue;   // a fused head needs all its channels in one tile
    if (a.dst == nullptr && a.dec.boxes == nullptr) return hipErrorInvalidValue;
    if (!tile_fits(t, a.Cin, a.src1 ? a.C0 : -1, a.CoutPad)) return hipErrorInvalidValue;
    return Tiles16<E>::table[tile].launch(a, out_f32, s);
}

// Second half of a split-K conv: per element slab[0] + slab[1] + ... + slab[S-1], added in that order, then exactly the unsplit epilogue's
// operations through the same helpers (bn_act, add_res_pack<E>).  16-bit output: eight channels per thread, 16-byte loads and stores
// (Cout % 8 == 0).  OUT_F32 (a conv that writes an fp32 net output itself, Cout = 255 in CoutPad = 256 included): one element per thread.
template <class E, bool OUT_F32>
__global__ __launch_bounds__(256) void splitk_finish16(const float *__restrict__ ws, int S, size_t slab_elems, int cout_pad,
                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                       const unsigned short *__restrict__ residual, void *__restrict__ dst, int M, int cout,
                                                       int leaky)
{
    constexpr int W = OUT_F32 ? 1 : 8;
    const int per_row = cout / W;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)M * per_row) return;
    const int m = (int)(idx / per_row);
    const int n = ((int)(idx - (size_t)m * per_row)) * W;
    const float *src = ws + (size_t)m * cout_pad + n;
    if constexpr (OUT_F32) {
        float v = *src;
        for (int s = 1; s < S; ++s) v = v + src[(size_t)s * slab_elems];
        static_cast<float *>(dst)[(size_t)m * cout + n] = bn_act(v, scale[n], shift[n], leaky);
    } else {
        f32x4 a0 = *reinterpret_cast<const f32x4 *>(src), a1 = *reinterpret_cast<const f32x4 *>(src + 4);
        for (int s = 1; s < S; ++s) {
            a0 = a0 + *reinterpret_cast<const f32x4 *>(src + (size_t)s * slab_elems);
            a1 = a1 + *reinterpret_cast<const f32x4 *>(src + (size_t)s * slab_elems + 4);
        }
        const f32x4 sc0 = *reinterpret_cast<const f32x4 *>(scale + n), sc1 = *reinterpret_cast<const f32x4 *>(scale + n + 4);
        const f32x4 sh0 = *reinterpret_cast<const f32x4 *>(shift + n), sh1 = *reinterpret_cast<const f32x4 *>(shift + n + 4);
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = bn_act(a0[k], sc0[k], sh0[k], leaky);
            v[4 + k] = bn_act(a1[k], sc1[k], sh1[k], leaky);
        }
        const size_t o = (size_t)m * cout + n;
        u32x4 rr{0u, 0u, 0u, 0u};
        if (residual) rr = *reinterpret_cast<const u32x4 *>(residual + o);
        *reinterpret_cast<u32x4 *>(static_cast<unsigned short *>(dst) + o) = add_res_pack<E>(v, rr, residual != nullptr);
    }
}

// The split-K form is instantiated for the two tiles a small plan lands on: 11 (64x64) and 12 (64x128), both LDS-DMA with 128-byte rows
// (BK 64; int8: 128), four waves
template <class E, int TN>
static hipError_t launch_split_t(const ConvArgs &c, int grid, int S, hipStream_t s)
{
    constexpr int BK = 128 / E::BYTES;
    constexpr size_t lds = 2 * (size_t)(64 + 64 * TN) * 128;   // the two operand stages; a split launch has no epilogue tile
    if (c.src1) return launch_conv_kernel<conv16_mfma<E, 1, TN, 2, 2, BK, true, false, true, 1, false, true>>(c, grid, 256, lds, s, S);
    return launch_conv_kernel<conv16_mfma<E, 1, TN, 2, 2, BK, false, false, true, 1, false, true>>(c, grid, 256, lds, s, S);
}

inline bool conv16_split_tile(int tile) { return tile == 11 || tile == 12; }

// The split launch of tile id `tile` for element type E and its finish launch on the same stream (launch_conv_bf16_split / launch_conv_f16_split)
template <class E>
static hipError_t launch_conv16_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s)
{
    if (!conv16_split_tile(tile)) return hipErrorInvalidValue;
    const auto [c, slab, grid] = split_launch(a, Tiles16<E>::table[tile].info, S, ws, ws_bytes);
    if (!slab) return hipErrorInvalidValue;
    // the 16-bit form of the finish launch moves eight channels per thread: whole 16-byte pieces of dst and of the shortcut
    if (!out_f32 && (a.Cout % 8 || ((uintptr_t)a.dst & 15) || ((uintptr_t)a.residual & 15))) return hipErrorInvalidValue;
    if (out_f32 && a.residual) return hipErrorInvalidValue;
    if (hipError_t e = tile == 12 ? launch_split_t<E, 2>(c, grid, S, s) : launch_split_t<E, 1>(c, grid, S, s); e != hipSuccess) return e;
    const float *wsf = static_cast<const float *>(ws);
    const unsigned short *res = static_cast<const unsigned short *>(a.residual);
    const size_t n = (size_t)a.M * (out_f32 ? a.Cout : a.Cout / 8);
    const dim3 fgrid((unsigned)((n + 255) / 256));
    if (out_f32)
        hipLaunchKernelGGL((splitk_finish16<E, true>), fgrid, dim3(256), 0, s, wsf, S, slab / 4, a.CoutPad, a.scale, a.shift, res, a.dst, a.M, a.Cout, a.leaky);
    else
        hipLaunchKernelGGL((splitk_finish16<E, false>), fgrid, dim3(256), 0, s, wsf, S, slab / 4, a.CoutPad, a.scale, a.shift, res, a.dst, a.M, a.Cout, a.leaky);
    return hipGetLastError();
}

}  // namespace y3
