// fp32-accurate convolution on the bf16 matrix cores: every fp32 value is carried as THREE bf16 planes
// (hi, mid, lo: x = hi + mid + lo exactly, 3 x 8 significand bits = the 24 bits of fp32) and every product
// a*b is formed from the six leading partial products
//      hi*hi + hi*mid + mid*hi + hi*lo + lo*hi + mid*mid          (dropped terms are <= 2^-24 |a*b|)
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  bf16 x bf16 products are exact in fp32, so the result has
// fp32-level accuracy (the parity bar of the fp32 path -- 1e-4 on boxes/scores against the fp32 oracle -- is the
// bar of this path, same tests) at 1/6 of the bf16 MFMA rate = 2.67x the rate of v_mfma_f32_32x32x2_f32.
//
// A second scheme of the same kernel (NPL = 2, "f32x2") carries a value as TWO fp16 planes, x = h + l' * 2^-11 with
// h = fp16(x) and l' = fp16((x - h) * 2^11) (the power-of-two scale keeps l' a normal number whenever |x| > 2^-13),
// and forms a*b from three products on v_mfma_f32_32x32x16_f16:
//      ha*hb -> accumulator 0;   ha*lb' + la'*hb -> accumulator 1;   result = acc0 + acc1 * 2^-11
// (dropped: la*lb <= 2^-22 |a*b|; fp16 x fp16 products are exact in fp32).  Half the MFMAs and two thirds of the bytes
// of the three-plane scheme -- it matters because both run at the socket power limit -- for a
// representation error of 2^-22 instead of 2^-24 and a value range of |x| < 65504.
//
// Same fused op as conv_f32.hip / conv_bf16.hip (reference: core/parse_model.py:27-52,72,134,155-156).
// Layout: activations [pixel][plane 0..2][C] bf16, weights [CoutPad][plane][K] bf16, head outputs fp32.
// Operand tiles go HBM/L2 -> LDS by direct-to-LDS buffer loads (one tile per plane), double buffered; LDS rows are
// 2*BK bytes with the 16-B chunk index XOR-swizzled (swizzled_chunk) on the source address and on the fragment reads.
#include <algorithm>
#include <type_traits>

#include "conv_common.h"

namespace y3 {

// The LDS-DMA instructions of the next K tile are issued together at the top of the iteration.  Issuing them one or two at a time between
// the MFMA groups (also pinned there with sched_group_barrier), three LDS stages and BK 16 / 64 were measured and retired
// (profiles/r01_tile_sweep_f32x3_b64_s416.txt; the timing-only probes of round 1: profiles/r01_probe_*.txt).
template <int NPL, int TM, int TN, int WR, int WC, int BK, bool CONCAT, bool OUT_F32, int STAGES = 2>
__global__ __launch_bounds__(64 * WR * WC) void conv_f32x3_mfma(const ConvArgs p)
{
    static_assert(NPL == 2 || NPL == 3, "two fp16 planes or three bf16 planes");
    static_assert(STAGES == 1 || STAGES == 2, "one LDS stage or two (double buffered)");
    constexpr int NACC = NPL == 2 ? 2 : 1;   // accumulator sets (two-plane scheme: cross terms carry a 2^11 scale)
    constexpr int BM = 32 * TM * WR;
    constexpr int BN = 32 * TN * WC;
    constexpr int NT = 64 * WR * WC;
    constexpr int LPR = BK / 8;        // 16-B chunks (8 bf16) per row: 2, 4 or 8
    constexpr int RPI = 64 / LPR;      // rows written by one wave-wide LDS-DMA instruction
    constexpr int RP = NT / LPR;       // rows per load pass of the whole workgroup
    constexpr int AP = (BM + RP - 1) / RP, BP = (BN + RP - 1) / RP;   // a pass may cover fewer rows than RP: whole
    static_assert(BM % RPI == 0 && BN % RPI == 0, "tile rows must be whole wave instructions");   // waves then skip it
    constexpr int ROWB = 2 * BK;                      // LDS row bytes (64 or 128)
    constexpr int PLANE_B = (BM + BN) * ROWB;         // one plane of one stage: A rows then B rows
    constexpr int STAGE_B = NPL * PLANE_B;
    constexpr int CROW = BN + 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;

    const int logical = xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x);
    const int tilesN = p.CoutPad / BN;
    const int mt = logical / tilesN, nt = logical - mt * tilesN;
    const int m0 = mt * BM, n0 = nt * BN;

    const __amdgpu_buffer_rsrc_t rs0 = buffer_rsrc(p.src0, p.src0_bytes);
    const __amdgpu_buffer_rsrc_t rs1 = buffer_rsrc(CONCAT ? p.src1 : p.src0, CONCAT ? p.src1_bytes : p.src0_bytes);
    const __amdgpu_buffer_rsrc_t rsw = buffer_rsrc(p.wpk, p.w_bytes);
    const unsigned OOB0 = p.src0_bytes, OOB1 = CONCAT ? p.src1_bytes : p.src0_bytes;

    const int lrow = tid / LPR;
    const int lchunk = swizzled_chunk<LPR>(lrow, tid % LPR) * 8;  // logical chunk landing in physical chunk tid % LPR
    int aoff[AP];
    int aoff1[CONCAT ? AP : 1];
    int ahw[AP];
    const int C1 = p.Cin - p.C0;
    const TileOrigin org = tile_origin(p, m0);   // (b, ho, wo) of every row: conv_common.h
#pragma unroll
    for (int i = 0; i < AP; ++i)
        gather_row<CONCAT, NPL>(p, org, m0 + i * RP + lrow, org.wo0 + i * RP + lrow, C1, aoff[i], aoff1[CONCAT ? i : 0], ahw[i]);
    unsigned boff[BP];  // byte offset of plane 0 of weight row n, this lane's chunk
#pragma unroll
    for (int j = 0; j < BP; ++j) boff[j] = (unsigned)((n0 + j * RP + lrow) * NPL * p.K + lchunk) * 2u;

    int tap = 0, c0 = 0;
    unsigned avoff[AP];
    unsigned avoff1[CONCAT ? AP : 1];
    auto set_tap = [&]() {   // as in conv_bf16.hip; written out in both: DESIGN.md section 4, "One row per tile"
        if (CONCAT) {
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                avoff[i] = (ahw[i] < 0) ? OOB0 : (unsigned)(aoff[i] + lchunk) * 2u;
                avoff1[i] = (ahw[i] < 0) ? OOB1 : (unsigned)(aoff1[i] + lchunk) * 2u;
            }
        } else {
            const int u = tap / p.ksize, v = tap - u * p.ksize;
            const int toff = (u * p.W + v) * NPL * p.Cin + lchunk;
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                const int hi = (ahw[i] >> 16) + u, wi = (int)(short)(ahw[i] & 0xffff) + v;
                const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                avoff[i] = ok ? (unsigned)(aoff[i] + toff) * 2u : OOB0;
            }
        }
    };
    set_tap();

    int kglob = 0;
    auto fetch_dma = [&](int buf) {
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
            unsigned char *sa = smem + buf * STAGE_B + pl * PLANE_B + wave * RPI * ROWB;
            unsigned char *sb = sa + BM * ROWB;
            if (CONCAT && c0 >= p.C0) {
#pragma unroll
                for (int i = 0; i < AP; ++i)
                    if (i * RP + wave * RPI < BM)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lds_ptr)(sa + i * RP * ROWB), 16, (int)avoff1[i],
                                                                 (pl * C1 + c0 - p.C0) * 2, 0, 0);
            } else {
#pragma unroll
                for (int i = 0; i < AP; ++i)
                    if (i * RP + wave * RPI < BM)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_ptr)(sa + i * RP * ROWB), 16, (int)avoff[i],
                                                                 (pl * (CONCAT ? p.C0 : p.Cin) + c0) * 2, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < BP; ++j)
                if (j * RP + wave * RPI < BN)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sb + j * RP * ROWB), 16, (int)boff[j],
                                                             (pl * p.K + kglob) * 2, 0, 0);
        }
        kglob += BK;
        c0 += BK;
        if (c0 == p.Cin) {
            c0 = 0;
            ++tap;
            if (!CONCAT) set_tap();
        }
    };

    f32x16 acc[NACC][TM][TN];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][i][j][e] = 0.0f;

    const int KT = p.K / BK;
    fetch_dma(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int fr = lane & 31, fh = lane >> 5;
    const int a_frag = (wr * 32 * TM + fr) * ROWB;
    const int b_frag = BM * ROWB + (wc * 32 * TN + fr) * ROWB;
    int foff[BK / 16];
#pragma unroll
    for (int s_ = 0; s_ < BK / 16; ++s_) foff[s_] = swizzled_chunk<LPR>(fr, 2 * s_ + fh) * 16;

    for (int kt = 0; kt < KT; ++kt) {
        const int cur = (STAGES == 2) ? (kt & 1) : 0;
        const bool more = kt + 1 < KT;
        if (STAGES == 2 && more) fetch_dma(cur ^ 1);
        const unsigned char *st = smem + cur * STAGE_B;
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            typedef typename std::conditional<NPL == 3, bf16x8, f16x8>::type frag_t;
            frag_t fa[NPL][TM], fb[NPL][TN];
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    fa[pl][i] = *reinterpret_cast<const frag_t *>(st + pl * PLANE_B + a_frag + i * 32 * ROWB + foff[s]);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    fb[pl][j] = *reinterpret_cast<const frag_t *>(st + pl * PLANE_B + b_frag + j * 32 * ROWB + foff[s]);
            }
            // products outermost, (i, j) innermost: consecutive MFMAs never wait on each other's accumulator
            if constexpr (NPL == 3) {
                constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};   // hi*lo, lo*hi, mid*mid, hi*mid, mid*hi, hi*hi
#pragma unroll
                for (int q = 0; q < 6; ++q)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[q]][i], fb[PB[q]][j], acc[0][i][j], 0, 0, 0);
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q)    // h*l' and l'*h into the scaled accumulator set, then h*h
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            f32x16 &c = acc[q == 2 ? 0 : NACC - 1][i][j];
                            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[q == 1 ? 1 : 0][i], fb[q == 0 ? 1 : 0][j], c, 0, 0, 0);
                        }
            }
        }
        if (STAGES == 2) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else {
            __syncthreads();                       // every wave is done reading the single stage
            if (more) {
                fetch_dma(0);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
    }

    // ---- epilogue through LDS, one 32-row block of every wave per pass (as conv_bf16.hip) ------------------
    constexpr int EROWS = WR * 32;
    constexpr int PPR = BN / 8;
    constexpr int NPC = (EROWS * PPR + NT - 1) / NT;
    float *C = reinterpret_cast<float *>(smem);
    unsigned short *dstb = static_cast<unsigned short *>(p.dst);
    const unsigned short *res = static_cast<const unsigned short *>(p.residual);
    const size_t prow = (size_t)NPL * p.Cout;  // 16-bit elements per pixel
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        u32x4 rr[OUT_F32 ? 1 : NPC][NPL];
        if (!OUT_F32 && res) {
#pragma unroll
            for (int it = 0; it < NPC; ++it) {
                const int pc = tid + it * NT;
                const int r = pc / PPR, ch = (pc - r * PPR) * 8;
                const int m = m0 + (r >> 5) * 32 * TM + i * 32 + (r & 31);
                const bool ok = pc < EROWS * PPR && m < p.M && n0 + ch < p.Cout;
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
                    rr[it][pl] = ok ? *reinterpret_cast<const u32x4 *>(res + (size_t)m * prow + pl * p.Cout + n0 + ch)
                                    : u32x4{0u, 0u, 0u, 0u};
            }
        }
        if (i > 0) __syncthreads();
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nl = (wc * TN + j) * 32 + fr;
            const float sc = p.scale[n0 + nl], sh = p.shift[n0 + nl];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                // three planes: BN scale applied here; two planes: scale already folded into the packed weights, sc the power of two the
                // channel's weights were normalised by (exact)
                float v = NPL == 3 ? acc[0][i][j][e] * sc + sh
                                   : (acc[0][i][j][e] + acc[NACC - 1][i][j][e] * (1.0f / 2048.0f)) * sc + sh;
                if (p.leaky) v = fmaxf(v, 0.1f * v);
                C[(wr * 32 + mfma32_row(e, fh)) * CROW + nl] = v;
            }
        }
        __syncthreads();
        if (OUT_F32) {
            float *dst = static_cast<float *>(p.dst);
            for (int idx = tid; idx < EROWS * BN; idx += NT) {
                const int r = idx / BN, col = idx - r * BN;
                const int m = m0 + (r >> 5) * 32 * TM + i * 32 + (r & 31), n = n0 + col;
                if (m < p.M && n < p.Cout) dst[(size_t)m * p.Cout + n] = C[r * CROW + col];
            }
        } else {
#pragma unroll
            for (int it = 0; it < NPC; ++it) {
                const int pc = tid + it * NT;
                const int r = pc / PPR, ch = (pc - r * PPR) * 8;
                const int m = m0 + (r >> 5) * 32 * TM + i * 32 + (r & 31);
                if (pc >= EROWS * PPR || m >= p.M || n0 + ch >= p.Cout) continue;   // Cout < BN only for the 32-channel conv
                const f32x4 v0 = *reinterpret_cast<const f32x4 *>(C + r * CROW + ch);
                const f32x4 v1 = *reinterpret_cast<const f32x4 *>(C + r * CROW + ch + 4);
                float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                if (res) {
                    // shortcut operand rebuilt from its planes, Add([from, x]) = from + x
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float a0, a1;
                        join_planes<NPL>(rr[it], k, a0, a1);
                        v[2 * k] = a0 + v[2 * k];
                        v[2 * k + 1] = a1 + v[2 * k + 1];
                    }
                }
                u32x4 o[NPL];
                split_planes<NPL>(v, o);
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
                    *reinterpret_cast<u32x4 *>(dstb + (size_t)m * prow + pl * p.Cout + n0 + ch) = o[pl];
            }
        }
    }
}

template <int NPL, int TM, int TN, int WR, int WC, int BK, bool CONCAT, bool OUT_F32, int STAGES>
static hipError_t launch_kx(const ConvArgs &a, hipStream_t s)
{
    constexpr int BM = 32 * TM * WR, BN = 32 * TN * WC;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.CoutPad / BN;
    const size_t stages = STAGES * (size_t)NPL * (BM + BN) * (2 * BK);
    const size_t ctile = (size_t)WR * 32 * (BN + 4) * sizeof(float);
    return launch_conv_kernel<conv_f32x3_mfma<NPL, TM, TN, WR, WC, BK, CONCAT, OUT_F32, STAGES>>(a, tilesM * tilesN, 64 * WR * WC,
                                                                                                std::max(stages, ctile), s);
}

template <int NPL, int TM, int TN, int WR, int WC, int BK, int STAGES>
static hipError_t launch_tp(const ConvArgs &a, bool out_f32, hipStream_t s)
{
    return dispatch_concat_out(a.src1 != nullptr, out_f32, [&](auto concat, auto f32) {
        return launch_kx<NPL, TM, TN, WR, WC, BK, decltype(concat)::value, decltype(f32)::value, STAGES>(a, s);
    });
}

// One row per tile id, shared by the two plane-split modes: the geometry and, per mode, the launcher of its instantiation (null: not built
// for that mode; both null: a retired id).  The geometry is read off the template arguments the launchers are instantiated with.
using LaunchX = hipError_t (*)(const ConvArgs &, bool out_f32, hipStream_t);
struct TileX3 { TileInfo info; LaunchX launch3, launch2; };   // three bf16 planes, two fp16 planes
enum { P3 = 1, P2 = 2 };
template <int TM, int TN, int WR, int WC, int STAGES, int MODES>
static constexpr TileX3 tile()
{
    constexpr int BK = 32;
    TileX3 r = {{32 * TM * WR, 32 * TN * WC, WR * WC, STAGES, BK}, nullptr, nullptr};
    if constexpr ((MODES & P3) != 0) r.launch3 = launch_tp<3, TM, TN, WR, WC, BK, STAGES>;
    if constexpr ((MODES & P2) != 0) r.launch2 = launch_tp<2, TM, TN, WR, WC, BK, STAGES>;
    return r;
}

// Ids are stable (tuning/f32x3_*.json, f32x2_*.json name them).  Only the tiles a plan can select are built (the tuning tables, choose_tile_x3 /
// choose_tile_x2 in y3_net.cpp; tests/test_abi.py); the two-plane mode takes the schedules that won or came close in the three-plane sweeps.
static const TileX3 kTilesX3[X3_TILE_COUNT] = {
    tile<2, 2, 2, 2, 2, P3 | P2>(),   //  0: 128x128, 4 waves
    tile<2, 1, 2, 2, 2, P3 | P2>(),   //  1: 128x64
    tile<1, 1, 2, 2, 2, P3 | P2>(),   //  2: 64x64
    tile<1, 2, 2, 2, 2, P3 | P2>(),   //  3: 64x128
    tile<2, 2, 4, 2, 2, P3 | P2>(),   //  4: 256x128, 8 waves
    {}, {}, {},                       //  5..7
    tile<2, 2, 2, 4, 2, P3 | P2>(),   //  8: 128x256, 8 waves
    tile<2, 2, 2, 2, 1, P3>(),        //  9: 128x128, 4 waves, single LDS stage (3 workgroups / CU)
    {}, {},                           // 10, 11
    tile<2, 1, 2, 4, 2, P3 | P2>(),   // 12: 128x128, 8 waves (64x32 wave tile)
    tile<2, 1, 2, 2, 1, P3>(),        // 13: 128x64, single stage
    tile<1, 2, 2, 2, 1, P3>(),        // 14: 64x128, single stage
    {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {},   // 15..25
    tile<2, 1, 4, 4, 2, P2>(),        // 26: 256x128, 16 waves (64x32 wave tiles)
    tile<2, 1, 2, 8, 2, P2>(),        // 27: 128x256, 16 waves
    {}, {}, {}, {}, {}, {},           // 28..33
};

static const TileX3 *row_x3(int tile) { return (tile >= 0 && tile < X3_TILE_COUNT) ? &kTilesX3[tile] : nullptr; }

TileInfo conv_x3_tile_info(int tile) { return kTilesX3[row_x3(tile) ? tile : 0].info; }
bool conv_x3_tile_built(int tile) { return row_x3(tile) && row_x3(tile)->launch3; }
bool conv_x2_tile_built(int tile) { return row_x3(tile) && row_x3(tile)->launch2; }

static hipError_t launch_row(const TileX3 *t, LaunchX launch, const ConvArgs &a, bool out_f32, hipStream_t s)
{
    if (!launch || !tile_fits(t->info, a.Cin, a.src1 ? a.C0 : -1, a.CoutPad)) return hipErrorInvalidValue;   // retired id / other mode only
    return launch(a, out_f32, s);
}

hipError_t launch_conv_f32x3(const ConvArgs &a, int tile, bool out_f32, hipStream_t s)
{
    const TileX3 *t = row_x3(tile);
    return launch_row(t, t ? t->launch3 : nullptr, a, out_f32, s);
}

hipError_t launch_conv_f32x2(const ConvArgs &a, int tile, bool out_f32, hipStream_t s)
{
    const TileX3 *t = row_x3(tile);
    return launch_row(t, t ? t->launch2 : nullptr, a, out_f32, s);
}

}  // namespace y3
