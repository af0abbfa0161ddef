// fp32 implicit-GEMM convolution on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Replaces Conv2D -> BatchNormalization -> LeakyReLU(0.1) [-> Add] of the reference graph
// (reference: core/parse_model.py:27-52,155-156) and the UpSampling2D + Concatenate feeding the
// lateral 1x1 convs (reference: core/parse_model.py:72,134) with ONE launch per conv.
//
// GEMM view: M = B*Ho*Wo output pixels (NHWC order), N = Cout, K = taps*Cin with k = tap*Cin + c.
//   A[m][k]  = input pixel (ho*s-pad+u, wo*s-pad+v) channel c, gathered on the fly (zero outside)
//   B[n][k]  = packed weights [CoutPad][K]
// Block tile BM x BN x 32, WR x WC waves (64*WR*WC threads), wave tile (32*TM) x (32*TN).
// Both operand tiles live in LDS as [rows][32+4] floats (K contiguous, one 16-B pad per row:
// row stride 9 x 16 B makes every ds_read_b128 of 16 different rows conflict-free), filled with
// 16-B buffer loads -> ds_write_b128 (one LDS stage; the LDS-DMA tiles below also come double buffered, one barrier per K tile).
// A lane reads 4 consecutive k of its row as one ds_read_b128 and feeds them to 4 MFMAs; lanes
// 0-31 / 32-63 take k = 8q+t / 8q+4+t in MFMA (q,t), identically for A and B, so every k is
// contracted exactly once (the order of k inside a tile is irrelevant to the sum's value up to
// fp32 rounding).
// Epilogue from the accumulators: y = acc*scale[n] + shift[n]; leaky; + residual; store.
//
// Split-K (SPLIT = true, the low-latency plans of y3_net_set_low_latency): a launch of S slices runs S times the workgroups,
// gridDim.y = S.  Slice y walks K tiles [y*KT/S, (y+1)*KT/S) of the SAME walk an unsplit launch takes -- the chunk-major order is
// kept where it is in force, and slices are counted along that walk -- and stores its raw accumulators (no epilogue, rows >= M
// included: the slab is padded to whole tiles) into slab y of a workspace [S][Mpad][CoutPad].  splitk_finish_f32, a separate launch
// on the same stream, adds the slabs in the order 0, 1, ..., S-1 and applies the epilogue above.
//
// Border skip (BMIN = true; ConvArgs::pos_tab set: 3x3, single source, unsplit, B % 32 == 0): GEMM rows are batch-minor, m = j * B + b with j an
// index into the conv geometry's position table (positions sorted by which taps read inside the image), so a 32-row block is one output
// position of 32 images and a tile holds BM / 32 positions.  The K walk visits only the taps that are live for some position of the tile, in
// the order they had; what is left out are products with the zeros of the padding, so the result keeps its bits.
// The table's sort puts the tiles with such a short walk first; ConvArgs::border_tiles >= 0 deals them, and the interior tiles, evenly over the
// XCD M-ranges (balanced_tile, y3_kernels.h) -- which workgroup computes a tile changes, nothing of the tile.
#include <algorithm>
#include <type_traits>

#include "conv_common.h"

namespace y3 {

static constexpr int BK = 32;
// floats per LDS row: register-staged loads pad the row by 16 B, LDS-DMA rows are unpadded and swizzled
static constexpr int lds_row(int dma) { return dma ? BK : BK + 4; }

// 16-byte buffer load: per-lane voffset (range-checked against num_records) + wave-uniform soffset
__device__ __forceinline__ f32x4 buf_load16(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, 0);
    return __builtin_bit_cast(f32x4, v);
}

// DMA != 0: operand tiles are filled by direct-to-LDS buffer loads (no VGPR round trip, no ds_write): measured with
// tools/mfma_probe.hip, a 16-B load to VGPRs costs the SIMD ~8-16 cycles of matrix-pipe time and a ds_write_b128 ~13,
// an LDS-DMA load ~4.  LDS rows are then unpadded 128 B (a wave instruction writes 8 whole rows) and bank conflicts
// are avoided by an XOR swizzle of the 16-B chunk index (swizzled_chunk) applied on the SOURCE address and on the fragment reads.
//
// Removed in round 4 (records under profiles/r01_*, r02_*, code in the history): the timing-only PROBE ablations, the
// persistent stream-K schedule (neutral on 3x3, -10 % on 1x1 layers: profiles/r02_tile_sweep_f32_streamk_b64_s416.txt) and the
// residual-prefetch tiles (conv stack -0.3 %: profiles/r02_residual_prefetch_ab.txt).
#ifdef Y3_PHASE_STAMPS
// Diagnostic build only (csrc/build.py --variant ... -DY3_PHASE_STAMPS, tools/phase_stamps.py --dtype f32): thread 0 of every workgroup
// (up to 32768) of the launches whose K equals y3_dbg32_sel_k stores s_memrealtime (100 MHz) at kernel entry, before the first fetch,
// after the first barrier, after the K loop and after the epilogue, plus HW_ID / XCC_ID, into a buffer no other code reads.
__device__ unsigned long long y3_dbg32_stamps[8 * 32768];
__device__ int y3_dbg32_sel_k = -1;
#define Y3_STAMP32(k) do { if (threadIdx.x == 0 && blockIdx.x < 32768 && p.K == y3_dbg32_sel_k) y3_dbg32_stamps[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define Y3_STAMP32(k) do { } while (0)
#endif

template <int TM, int TN, int WR, int WC, bool CONCAT, int STAGES, int MINW = 1, int DMA = 0, bool SPLIT = false, bool BMIN = false>
__global__ __launch_bounds__(64 * WR * WC, MINW) void conv_f32_mfma(const ConvArgs p)
{
    static_assert(!SPLIT || (!DMA && STAGES == 1), "the split-K form is built for the register-staged single-stage tiles");
    static_assert(!BMIN || (!CONCAT && !SPLIT), "batch-minor rows are built for the unsplit single-source launch");
    Y3_STAMP32(0);
#ifdef Y3_PHASE_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 32768 && p.K == y3_dbg32_sel_k) {
        y3_dbg32_stamps[blockIdx.x * 8 + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
        y3_dbg32_stamps[blockIdx.x * 8 + 6] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
    }
#endif
    static_assert(DMA || STAGES == 1, "register-staged operand loads are single-stage; two stages need the LDS-DMA loads");
    constexpr int LDS_ROW = lds_row(DMA);
    constexpr int BM = 32 * TM * WR;
    constexpr int BN = 32 * TN * WC;
    constexpr int NT = 64 * WR * WC;
    constexpr int RP = NT / 8;   // rows per load pass (8 lanes x 16 B cover one 32-float row)
    constexpr int AP = BM / RP;  // A load passes
    constexpr int BP = BN / RP;
    static_assert(BM % RP == 0 && BN % RP == 0 && AP >= 1 && BP >= 1, "tile too small for the thread count");
    constexpr int STAGE = (BM + BN) * LDS_ROW;  // floats per LDS stage
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    if constexpr (!SPLIT) clk_stamp_entry(p.clk_stamps);   // measurement launches only (y3_net_measure_sclk); a split launch carries no stamps
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;

    const int nwg = gridDim.x;   // read here: passing gridDim.x further down reorders this kernel's prologue
    const int bid = blockIdx.x, xcd = bid & 7;
    const int logical = xcd_contiguous_tile(bid, nwg);   // (the xcd_gn > 0 order below replaces it)
    const int tilesN = p.CoutPad / BN;
    // K tiles of this workgroup's walk: all of them, or slice blockIdx.y of gridDim.y (starting at tile kt0 of the walk)
    const int kt0 = SPLIT ? (int)blockIdx.y * (p.K / BK) / (int)gridDim.y : 0;
    int KT = SPLIT ? ((int)blockIdx.y + 1) * (p.K / BK) / (int)gridDim.y - kt0 : p.K / BK;   // (BMIN: the live taps' tiles, below)
    const __amdgpu_buffer_rsrc_t rs0 = buffer_rsrc(p.src0, p.src0_bytes);
    const __amdgpu_buffer_rsrc_t rs1 = buffer_rsrc(CONCAT ? p.src1 : p.src0, CONCAT ? p.src1_bytes : p.src0_bytes);
    const __amdgpu_buffer_rsrc_t rsw = buffer_rsrc(p.wpk, p.w_bytes);
    // a voffset equal to num_records is out of range for the buffer's bounds check -> the load returns 0
    const unsigned OOB0 = p.src0_bytes, OOB1 = CONCAT ? p.src1_bytes : p.src0_bytes;

    const __amdgpu_buffer_rsrc_t rsd = buffer_rsrc(p.dst, p.dst_bytes);
    const __amdgpu_buffer_rsrc_t rsr = buffer_rsrc(p.residual ? p.residual : p.dst, p.dst_bytes);
    const int fr = lane & 31, fh = lane >> 5;

    int mt = logical / tilesN, nt = logical - mt * tilesN;
    if (BMIN && p.border_tiles >= 0) {
        // balanced order (y3_kernels.h; launch_k sizes the grid for it): the XCD grid of the blocked order below (8 x 1 where that order is
        // not in force), every M-range with its share of the short border tiles and of the interior ones.  Scalar work, once.
        const TileMN t = balanced_tile(bid, p.xcd_gn > 0 ? p.xcd_gn : 1, tilesN, p.border_tiles, (p.M + BM - 1) / BM);
        mt = t.mt;
        nt = t.nt;
        if (mt < 0) return;                    // padding workgroups
    } else if (p.xcd_gn > 0) {
        // XCD-blocked order (launch_k sizes the grid for it): the 8 XCDs form a (8/gn) x gn grid over the tile matrix;
        // XCD (xm, xn) owns M-tiles [xm*tilesM/gm, (xm+1)*tilesM/gm) x N-tiles [xn*tilesN/gn, +tilesN/gn), N fastest.
        // With gn > 1 an XCD streams only 1/gn of the weight matrix through its 4 MB L2 (the 256->512 and 512->1024
        // 3x3 weights are 4.7 / 18.9 MB) at the price of gn XCDs reading every activation tile.
        const int gn = p.xcd_gn, gm = 8 / gn;
        const int tilesM = (p.M + BM - 1) / BM;
        const int xm = xcd / gn, xn = xcd - xm * gn;
        const int nb = tilesN / gn;
        const int mlo = xm * tilesM / gm, mhi = (xm + 1) * tilesM / gm;
        const int j = bid >> 3;
        const int lm = j / nb;
        mt = mlo + lm;
        nt = xn * nb + (j - lm * nb);
        if (mt >= mhi) return;                 // padding workgroups of an uneven M split
    }
    const int m0 = mt * BM, n0 = nt * BN;

    // ---- per-thread gather state -------------------------------------------------------------
    const int lrow = tid >> 3;         // row inside a pass
    // first float of this lane's 16-B piece inside the 32-float K tile (DMA: the logical chunk that lands in physical chunk
    // tid & 7 of the row; rows of a pass differ by multiples of 32)
    const int lchunk = DMA ? swizzled_chunk<8>(lrow, tid & 7) * 4 : (tid & 7) * 4;
    int aoff[AP];                      // element offset of (b, hi0, wi0, 0) in src0 (may be negative)
    int aoff1[CONCAT ? AP : 1];        // CONCAT: element offset of (b, ho, wo, 0) in src1
    int ahw[AP];                       // hi0 << 16 | (wi0 & 0xffff); row >= M marked by hi0 = -32768
    const int C1 = p.Cin - p.C0;
    // BMIN: the tile's 32-row blocks, each one output position of 32 images (conv_common.h); `live` = the taps that read inside the image
    // for some position of the tile.  Raster rows: one unused block, every tap.
    constexpr int NBLK = BMIN ? BM / 32 : 1;
    TileBlocks blk{0, 0, 1, 0x1ffu};
    unsigned eent[BMIN ? TM : 1];   // BMIN: table entry and first image of the TM accumulator blocks of this wave (epilogue)
    int eimg[BMIN ? TM : 1];
    if constexpr (BMIN) {
        blk = tile_blocks<NBLK>(p, m0);
        if (blk.live == 0) blk.live = 1;   // (no position at all: cannot happen for a tile of the grid; every load is then out of range)
        KT = __builtin_popcount(blk.live) * (p.Cin / BK);
#pragma unroll
        for (int i = 0; i < TM; ++i) tile_block<NBLK>(p, blk, wr * TM + i, eent[i], eimg[i]);
    } else {
        const TileOrigin org = tile_origin(p, m0);   // (b, ho, wo) of every row: conv_common.h
#pragma unroll
        for (int i = 0; i < AP; ++i)
            gather_row<CONCAT, 1>(p, org, m0 + i * RP + lrow, org.wo0 + i * RP + lrow, C1, aoff[i], aoff1[CONCAT ? i : 0], ahw[i]);
    }
    const int tap0 = BMIN ? __builtin_ctz(blk.live) : 0;   // first tap of the walk (of every channel chunk)
    unsigned boff[BP];  // byte offset of this lane's piece of weight row n, k = 0
#pragma unroll
    for (int j = 0; j < BP; ++j) boff[j] = (unsigned)((n0 + j * RP + lrow) * p.K + lchunk) * 4u;

    // walking state of the *next* K tile to fetch.  The fp32 MFMA does not co-execute with VALU work
    // (SQ_VALU_MFMA_COEXEC_CYCLES == 0 in the profile), so the K loop must issue (almost) no vector ALU
    // instructions: per-lane byte offsets are fixed per tap (out-of-image lanes hold the out-of-range
    // sentinel) and everything that changes per K tile goes into the scalar soffset of the buffer load.
    // K order.  Classic (k_chunk == 0): k = tap * Cin + c walked upwards.  Chunked (k_chunk = CK channels, 3x3 convs): for
    // every chunk of CK input channels all taps, then the next chunk -- the SAME products summed in another order (weights stay
    // packed [n][tap * Cin + c]; only the soffsets change).  The 9 reads of a pixel's CK channels (one per tap) then fall into
    // 9 * CK / 32 consecutive K tiles instead of being Cin / 32 tiles apart, so the tap re-reads hit in L2: with the classic
    // order a 512 -> 1024 @13 launch fetched 1.5-1.9 GB from beyond L2 for 85 MB of operands (tools/traffic_per_layer.py).
    const int CK = (!CONCAT && p.k_chunk > 0 && p.k_chunk < p.Cin) ? p.k_chunk : p.Cin;
    int tap = tap0;
    int kglob = BMIN ? tap * p.Cin : 0;  // k index of the next tile to fetch
    int c0 = 0;
    int cend = CK;            // end of the current channel chunk (classic order: Cin)
    const int taps = p.ksize * p.ksize;
    if constexpr (SPLIT) {
        // the walk's state at tile kt0: chunks of CK channels (the whole Cin in the classic order and for a concat 1x1), inside a
        // chunk tap after tap, inside a tap CK / 32 tiles.  A concat slice may begin anywhere in src0 or src1: the fetch picks the
        // source from c0.
        const int tpc = CK / BK, per_chunk = taps * tpc;
        const int chunk = kt0 / per_chunk, r = kt0 - chunk * per_chunk;
        tap = r / tpc;
        c0 = chunk * CK + (r - tap * tpc) * BK;
        cend = (chunk + 1) * CK;
        kglob = tap * p.Cin + c0;
    }
    unsigned avoff[AP];                  // voffset of this lane's piece for the current tap (or OOB0)
    unsigned okmask[CONCAT ? 1 : AP];    // !CONCAT: bit t = tap t of this row lies inside the image
    unsigned abase4[CONCAT ? 1 : AP];    // !CONCAT: byte offset of this lane's piece of the row at tap (0, 0), channel 0
    unsigned avoff1[CONCAT ? AP : 1];    // CONCAT: same for src1
    auto set_tap = [&]() {
        if (CONCAT) {
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                avoff[i] = (ahw[i] < 0) ? OOB0 : (unsigned)(aoff[i] + lchunk) * 4u;
                avoff1[i] = (ahw[i] < 0) ? OOB1 : (unsigned)(aoff1[i] + lchunk) * 4u;
            }
        } else {
            // 4 vector instructions per row (bit test, compare, add, select): with the chunk-major K order this runs every
            // CK / 32 K tiles, and vector ALU time is lost MFMA time
            const int u = tap / p.ksize, v = tap - u * p.ksize;
            const unsigned toff4 = (unsigned)((u * p.W + v) * p.Cin) * 4u;
#pragma unroll
            for (int i = 0; i < AP; ++i) avoff[i] = ((okmask[i] >> tap) & 1u) ? abase4[i] + toff4 : OOB0;
        }
    };
    if constexpr (BMIN) {
        // pass i reads rows [i * RP + lrow]: block (i * RP + lrow) / 32 of the tile, wave-uniform (RP = 32: block i; RP = 64: the wave's half),
        // image = the block's first + lrow % 32.  okmask comes from the table (the formula below, evaluated on the host; a block of rows >= M
        // reads a zero entry), so it and the tap test of set_tap are scalar.
        static_assert(RP == 32 || RP == 64, "a load pass covers one or two 32-row blocks");
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            unsigned e;
            int b;
            tile_block<NBLK>(p, blk, RP == 32 ? i : 2 * i + (wave >> 2), e, b);
            b += lrow & 31;
            const int hi0 = pos_ho(e) * p.stride - p.pad, wi0 = pos_wo(e) * p.stride - p.pad;
            aoff[i] = ((b * p.H + hi0) * p.W + wi0) * p.Cin;
            okmask[i] = pos_mask(e);
            abase4[i] = (unsigned)(aoff[i] + lchunk) * 4u;
        }
    } else if (!CONCAT) {
        // per row: bit t of okmask = tap t reads inside the image (rows >= M: no bit set); byte offset of the lane's piece at tap 0
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            unsigned mk = 0;
            if (ahw[i] >= 0 || (ahw[i] >> 16) != -32768) {
                const int hi0 = ahw[i] >> 16, wi0 = (int)(short)(ahw[i] & 0xffff);
                if (p.ksize == 3) {
                    // closed form of the loop below: row u contributes bits 3u..3u+2, column v bit v of each row.  With the SIMD full
                    // of 64-cycle MFMAs every vector instruction of a prologue waits ~one MFMA for its issue slot
                    // (tools/phase_stamps.py --dtype f32: 32 us from entry to the first fetch): six compares instead of two nested loops
                    const unsigned H = (unsigned)p.H, W = (unsigned)p.W;
                    const unsigned rm = ((unsigned)hi0 < H ? 7u : 0u) | ((unsigned)(hi0 + 1) < H ? 56u : 0u) | ((unsigned)(hi0 + 2) < H ? 448u : 0u);
                    const unsigned cm = ((unsigned)wi0 < W ? 1u : 0u) | ((unsigned)(wi0 + 1) < W ? 2u : 0u) | ((unsigned)(wi0 + 2) < W ? 4u : 0u);
                    mk = rm & (cm * 73u);
                } else {
                    for (int u = 0; u < p.ksize; ++u)
                        for (int v = 0; v < p.ksize; ++v)
                            if ((unsigned)(hi0 + u) < (unsigned)p.H && (unsigned)(wi0 + v) < (unsigned)p.W) mk |= 1u << (u * p.ksize + v);
                }
            }
            okmask[i] = mk;
            abase4[i] = (unsigned)(aoff[i] + lchunk) * 4u;
        }
    }
    set_tap();

    // the K walk both fetch forms end with: the next 32 channels of this tap, else the next tap (chunked order: of this channel chunk)
    auto advance_k = [&]() {
        c0 += BK;
        if (c0 == cend) {
            if constexpr (BMIN) {   // the next live tap (none left: taps, as the full walk ends)
                const unsigned rest = blk.live >> (tap + 1);
                tap = rest ? tap + 1 + __builtin_ctz(rest) : taps;
            } else {
                ++tap;
            }
            if (!CONCAT && tap == taps && cend != p.Cin) {   // chunked order: next channel chunk, first tap again
                tap = tap0;
                cend += CK;
            }
            c0 = cend - CK;
            if (!CONCAT) set_tap();
        }
        kglob = tap * p.Cin + c0;
    };

    f32x4 ra[AP], rb[BP];
    auto fetch_dma = [&](int buf) {
        // wave w fills rows [pass*RP + 8w, +8) of each tile: LDS destination = M0 base + lane*16
        float *sa = smem + buf * STAGE + wave * 8 * LDS_ROW;
        float *sb = sa + BM * LDS_ROW;
        if (CONCAT && c0 >= p.C0) {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lds_ptr)(sa + i * RP * LDS_ROW), 16, (int)avoff1[i], (c0 - p.C0) * 4, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_ptr)(sa + i * RP * LDS_ROW), 16, (int)avoff[i], c0 * 4, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < BP; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sb + j * RP * LDS_ROW), 16, (int)boff[j], kglob * 4, 0, 0);
        advance_k();
    };
    auto fetch = [&]() {
        if (CONCAT) {
            // channels [0,C0) come from src0, [C0,Cin) from src1; a 32-wide K tile never straddles (C0 % 32 == 0)
            if (c0 < p.C0) {
#pragma unroll
                for (int i = 0; i < AP; ++i) ra[i] = buf_load16(rs0, avoff[i], c0 * 4);
            } else {
#pragma unroll
                for (int i = 0; i < AP; ++i) ra[i] = buf_load16(rs1, avoff1[i], (c0 - p.C0) * 4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i) ra[i] = buf_load16(rs0, avoff[i], c0 * 4);
        }
#pragma unroll
        for (int j = 0; j < BP; ++j) rb[j] = buf_load16(rsw, boff[j], kglob * 4);
        advance_k();
    };
    auto stage = [&](int buf) {
        float *sa = smem + buf * STAGE;
        float *sb = sa + BM * LDS_ROW;
#pragma unroll
        for (int i = 0; i < AP; ++i) *reinterpret_cast<f32x4 *>(sa + (i * RP + lrow) * LDS_ROW + lchunk) = ra[i];
#pragma unroll
        for (int j = 0; j < BP; ++j) *reinterpret_cast<f32x4 *>(sb + (j * RP + lrow) * LDS_ROW + lchunk) = rb[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    Y3_STAMP32(1);
    if (DMA) {
        fetch_dma(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        fetch();
        stage(0);
    }
    __syncthreads();
    Y3_STAMP32(2);

    const int a_frag = (wr * 32 * TM + fr) * LDS_ROW + (DMA ? 0 : fh * 4);
    const int b_frag = BM * LDS_ROW + (wc * 32 * TN + fr) * LDS_ROW + (DMA ? 0 : fh * 4);
    int foff[4];  // float offset of this lane's k-chunk q inside its row
#pragma unroll
    for (int q = 0; q < 4; ++q) foff[q] = DMA ? swizzled_chunk<8>(fr, 2 * q + fh) * 4 : q * 8;

    // epilogue geometry
    const bool interior = (m0 + BM <= p.M) && (n0 + BN <= p.Cout);
    // bytes between two rows of an accumulator block in dst: the next pixel; BMIN: the same pixel of the next image
    const int row_bytes = BMIN ? p.Ho * p.Wo * p.Cout * 4 : p.Cout * 4;

    for (int kt = 0; kt < KT; ++kt) {
        const int cur = (STAGES == 2) ? (kt & 1) : 0;
        if (DMA && STAGES == 2) {
            if (kt + 1 < KT) fetch_dma(cur ^ 1);   // every wave passed the barrier that ended tile kt-1: buf cur^1 is free
        } else if (!DMA) {
            if (kt + 1 < KT) fetch();
        }
        const float *sa = smem + cur * STAGE + a_frag;
        const float *sb = smem + cur * STAGE + b_frag;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4 *>(sa + i * 32 * LDS_ROW + foff[q]);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4 *>(sb + j * 32 * LDS_ROW + foff[q]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
            // (s_setprio 1 / 0 around this block: -0.6 % on the conv stack, tools/ab_libs.py, round 2)
        }
        if (DMA && STAGES == 2) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile kt+1 has landed (issued a whole K tile ago)
            __syncthreads();
        } else if (DMA) {
            if (kt + 1 < KT) {
                __syncthreads();   // every wave is done reading the single buffer
                fetch_dma(0);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        } else if (kt + 1 < KT) {
            __syncthreads();  // every wave is done reading the tile
            stage(0);
            __syncthreads();
        }
    }

    Y3_STAMP32(3);
    if constexpr (SPLIT) {
        // raw accumulators -> slab blockIdx.y: p.dst is the workspace, p.dst_bytes the bytes of ONE slab [Mpad][CoutPad] (Mpad = whole
        // tiles, so every row of the tile has its place; the range check of the slab's own buffer resource drops anything else)
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
                for (int e = 0; e < 16; ++e)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)acc[i][j][e]), rss, (int)vbase,
                                                          mfma32_row(e) * slab_row_bytes, 0);
            }
        }
    } else {
    // ---- epilogue ----------------------------------------------------------------------------
    // accumulator element e of lane l: column (n) = l & 31, row (m) = mfma32_row(e, l >> 5).
    // Straight-line: out-of-tile elements get a voffset == num_records, which the buffer bounds check
    // turns into "load 0 / drop the store"; the 16 residual loads of a sub-tile are issued together.
    // interior tiles (the common case): one per-lane voffset per sub-tile, the row displacement of accumulator
    // element e rides in the scalar soffset -> no per-element address or bounds arithmetic on the VALU
    auto emit = [&](auto leaky_tag, auto res_tag, auto interior_tag) {
        constexpr bool LEAKY = decltype(leaky_tag)::value, RES = decltype(res_tag)::value;
        // shadows the run-time flag: straight-line code per case (the run-time form compiled to a branch around every
        // load and store; A/B r03: conv stack -0.07 %, i.e. neutral -- kept for the shorter instruction stream)
        constexpr bool interior = decltype(interior_tag)::value;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wc * TN + j) * 32 + fr;
            const float sh = p.shift[n];   // the BN scale is folded into the packed weights (y3_net.cpp)
            const bool n_ok = n < p.Cout;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mbase = m0 + (wr * TM + i) * 32 + 4 * fh;
                unsigned vbase;
                if constexpr (BMIN) {   // block wr * TM + i of the tile: pixel (ho, wo) of images img + 4 fh + mfma32_row(e)
                    const unsigned pe = eent[i];
                    const int b = eimg[i] + 4 * fh;
                    vbase = (unsigned)(((b * p.Ho + pos_ho(pe)) * p.Wo + pos_wo(pe)) * p.Cout + n) * 4u;
                } else {
                    vbase = (unsigned)(mbase * p.Cout + n) * 4u;
                }
                unsigned off[16];
                if (!interior) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int m = mbase + mfma32_row(e);
                        if constexpr (BMIN) off[e] = (n_ok && m < p.M) ? vbase + (unsigned)(mfma32_row(e) * row_bytes) : p.dst_bytes;
                        else off[e] = (n_ok && m < p.M) ? (unsigned)(m * p.Cout + n) * 4u : p.dst_bytes;
                    }
                }
                float r[16];
                if (RES) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int so = mfma32_row(e) * row_bytes;
                        r[e] = __builtin_bit_cast(float, interior ? __builtin_amdgcn_raw_buffer_load_b32(rsr, (int)vbase, so, 0)
                                                                  : __builtin_amdgcn_raw_buffer_load_b32(rsr, (int)off[e], 0, 0));
                    }
                }
                // element pairs as 2-vectors: the compiler selects v_pk_add_f32 / v_pk_mul_f32 (one instruction per pair, the same
                // IEEE operation per element): with the SIMD full of 64-cycle MFMAs every vector instruction of an epilogue
                // waits ~one MFMA for its issue slot, so the count of instructions is what the epilogue costs
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    f32x2 v2 = f32x2{acc[i][j][e], acc[i][j][e + 1]} + f32x2{sh, sh};
                    if (LEAKY) {
                        const f32x2 t2 = v2 * f32x2{0.1f, 0.1f};
                        v2 = f32x2{fmaxf(v2[0], t2[0]), fmaxf(v2[1], t2[1])};   // == (v >= 0 ? v : 0.1 v) for every finite v
                    }
                    if (RES) v2 = f32x2{r[e], r[e + 1]} + v2;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int ee = e + h;
                        const int so = mfma32_row(ee) * row_bytes;
                        if (interior)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)v2[h]), rsd, (int)vbase, so, 0);
                        else
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)v2[h]), rsd, (int)off[ee], 0, 0);
                    }
                }
            }
        }
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    auto emit2 = [&](auto leaky_tag, auto res_tag) {
        if (interior) emit(leaky_tag, res_tag, T_{}); else emit(leaky_tag, res_tag, F_{});
    };
    if (p.residual) {
        if (p.leaky) emit2(T_{}, T_{}); else emit2(F_{}, T_{});
    } else {
        if (p.leaky) emit2(T_{}, F_{}); else emit2(F_{}, F_{});
    }
    Y3_STAMP32(4);   // thread 0 = wave 0: its own stores issued (not yet retired)
    clk_stamp_exit(p.clk_stamps);
    }
}

// Second half of a split-K conv: dst[m][n] = epilogue(slab[0][m][n] + slab[1][m][n] + ... + slab[S-1][m][n]), the slabs added in that
// order, then exactly the conv epilogue's operations (+ shift, leaky as max(v, 0.1 v), + residual).  VEC: four channels per thread with
// 16-byte accesses (Cout % 4 == 0); otherwise one element per thread (the Cout = 255 head shape).
template <bool VEC>
__global__ __launch_bounds__(256) void splitk_finish_f32(const float *__restrict__ ws, int S, size_t slab_elems, int cout_pad,
                                                         const float *__restrict__ shift, const float *__restrict__ residual,
                                                         float *__restrict__ dst, int M, int cout, int leaky)
{
    constexpr int W = VEC ? 4 : 1;
    typedef float vec __attribute__((ext_vector_type(W)));
    const int per_row = cout / W;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)M * per_row) return;
    const int m = (int)(idx / per_row);
    const int n = ((int)(idx - (size_t)m * per_row)) * W;
    const float *src = ws + (size_t)m * cout_pad + n;
    vec v = *reinterpret_cast<const vec *>(src);
    for (int s = 1; s < S; ++s) v = v + *reinterpret_cast<const vec *>(src + (size_t)s * slab_elems);
    v = v + *reinterpret_cast<const vec *>(shift + n);
    if (leaky) {
        const vec t = v * 0.1f;
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = fmaxf(v[k], t[k]);
    }
    const size_t o = (size_t)m * cout + n;
    if (residual) v = *reinterpret_cast<const vec *>(residual + o) + v;
    *reinterpret_cast<vec *>(dst + o) = v;
}

template <int TM, int TN, int WR, int WC, bool CONCAT, int STAGES, int MINW, int DMA>
static hipError_t launch_k(const ConvArgs &a, hipStream_t s)
{
    constexpr int BM = 32 * TM * WR, BN = 32 * TN * WC;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.CoutPad / BN;
    const size_t lds = STAGES * (size_t)(BM + BN) * lds_row(DMA) * sizeof(float);
    int grid = tilesM * tilesN;
    if (a.xcd_gn > 0) {
        if (8 % a.xcd_gn || tilesN % a.xcd_gn) return hipErrorInvalidValue;
        const int gm = 8 / a.xcd_gn;
        int rows = 0;                                           // largest M block
        for (int xm = 0; xm < gm; ++xm) rows = std::max(rows, (xm + 1) * tilesM / gm - xm * tilesM / gm);
        grid = 8 * rows * (tilesN / a.xcd_gn);
    }
    if constexpr (!CONCAT) {   // batch-minor rows with the border taps skipped: the launch decision (refine_f32) sets the table only where this holds
        if (a.pos_tab) {
            if (a.ksize != 3 || a.B < 32 || a.B % 32 || a.M != a.B * a.Ho * a.Wo || a.Ho > kPosMaxGrid || a.Wo > kPosMaxGrid) return hipErrorInvalidValue;
            if (a.border_tiles > tilesM) return hipErrorInvalidValue;
            if (a.border_tiles >= 0) grid = balanced_grid(a.xcd_gn > 0 ? a.xcd_gn : 1, tilesN, a.border_tiles, tilesM);   // (xcd_gn was checked above)
            return launch_conv_kernel<conv_f32_mfma<TM, TN, WR, WC, false, STAGES, MINW, DMA, false, true>>(a, grid, 64 * WR * WC, lds, s);
        }
    } else if (a.pos_tab) {
        return hipErrorInvalidValue;
    }
    return launch_conv_kernel<conv_f32_mfma<TM, TN, WR, WC, CONCAT, STAGES, MINW, DMA>>(a, grid, 64 * WR * WC, lds, s);
}

template <int TM, int TN, int WR, int WC, int STAGES, int MINW, int DMA>
static hipError_t launch_t(const ConvArgs &a, hipStream_t s)
{
    return a.src1 ? launch_k<TM, TN, WR, WC, true, STAGES, MINW, DMA>(a, s) : launch_k<TM, TN, WR, WC, false, STAGES, MINW, DMA>(a, s);
}

// One row per tile id: the geometry, read off the template arguments, and the launcher of that instantiation; a retired id is an empty row.
struct TileF32 { TileInfo info; hipError_t (*launch)(const ConvArgs &, hipStream_t); };
// MINW: register budget (waves per SIMD) -- with 4, the two accumulators of the 32x64 wave tile stay in architectural VGPRs and the epilogue
// needs no v_accvgpr_read (nor the prologue 32-64 v_accvgpr_write: with the SIMD full of 64-cycle MFMAs every vector instruction outside the
// K loop waits ~one MFMA for its issue slot, profiles/r03_ab_f32_prologue.txt).  DMA: direct-to-LDS operand loads.
template <int TM, int TN, int WR, int WC, int STAGES = 1, int MINW = 1, int DMA = 0>
static constexpr TileF32 tile() { return {{32 * TM * WR, 32 * TN * WC, WR * WC, STAGES, BK}, launch_t<TM, TN, WR, WC, STAGES, MINW, DMA>}; }

// weight-resident 3x3 / stride 1 / Cin = 32 (conv_res_f32.hip): 8 x 16 pixels x 64 channels per workgroup tile
static hipError_t launch_res(const ConvArgs &a, hipStream_t s) { return conv_res_f32_fits(a) ? launch_conv_res_f32(a, s) : hipErrorInvalidValue; }

// Ids are stable (tuning files refer to them).  The table holds exactly the tiles a plan can select -- a packaged tuning table
// (tuning/f32_*.json) or the library's heuristic (choose_tile in y3_net.cpp) names every one of them (tests/test_abi.py).  The other ids of
// rounds 1-4 (the register-staged two-stage tiles 0..5, the 8- and 16-wave 128x128 / 256x128 tiles, the register-budget variant 24, the
// two-stage LDS-DMA tiles 28..30, the timing-only probes 20..22, 25) are retired: y3_tile_built answers 0; the sweeps that retired them
// are under profiles/.
static const TileF32 kTiles[TILE_COUNT] = {
    {}, {}, {}, {}, {}, {},           //  0..5
    tile<2, 2, 2, 2>(),               //  6: 128x128, 4 waves
    {},
    tile<2, 1, 4, 1>(),               //  8: 256x32
    tile<1, 2, 4, 1, 1, 4>(),         //  9: 128x64
    tile<1, 2, 2, 2, 1, 4>(),         // 10: 64x128
    tile<1, 1, 2, 2, 1, 4>(),         // 11: 64x64
    tile<2, 1, 2, 4>(),               // 12: 128x128, 8 waves
    {}, {}, {}, {},                   // 13..16
    tile<1, 1, 4, 2>(),               // 17: 128x64, 8 waves
    {}, {}, {}, {}, {},               // 18..22
    tile<2, 2, 2, 2, 1, 3>(),         // 23: 128x128 within 3 waves per SIMD of registers
    {}, {},                           // 24, 25
    tile<1, 2, 2, 2, 2, 4, 1>(),      // 26: 64x128, LDS-DMA, two stages
    tile<1, 1, 2, 2, 2, 4, 1>(),      // 27: 64x64, LDS-DMA, two stages
    {}, {}, {},                       // 28..30
    tile<1, 2, 2, 2, 1, 4, 1>(),      // 31: 64x128, LDS-DMA, single stage
    tile<1, 1, 2, 2, 1, 4, 1>(),      // 32: 64x64, LDS-DMA, single stage
    {{128, 64, 8, 2, BK}, launch_res},   // 33
};

#ifdef Y3_PHASE_STAMPS
extern "C" int y3_dbg32_select_k(int K) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(y3_dbg32_sel_k), &K, sizeof(int)); }
extern "C" int y3_dbg32_copy_stamps(unsigned long long *dst, int n_words)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(y3_dbg32_stamps), (size_t)n_words * sizeof(unsigned long long));
}
#endif

// The split-K form is instantiated for the two tiles a small plan selects: 10 (64x128) and 11 (64x64), both register-staged, single-stage
template <int TN>
static hipError_t launch_split_t(const ConvArgs &c, int grid, int S, hipStream_t s)
{
    constexpr size_t lds = (size_t)(64 + 64 * TN) * lds_row(0) * sizeof(float);
    if (c.src1) return launch_conv_kernel<conv_f32_mfma<1, TN, 2, 2, true, 1, 4, 0, true>>(c, grid, 256, lds, s, S);
    return launch_conv_kernel<conv_f32_mfma<1, TN, 2, 2, false, 1, 4, 0, true>>(c, grid, 256, lds, s, S);
}

bool conv_split_tile(int tile) { return tile == 10 || tile == 11; }

hipError_t launch_conv_f32_split(const ConvArgs &a, int tile, int S, void *ws, size_t ws_bytes, hipStream_t s)
{
    if (!conv_split_tile(tile)) return hipErrorInvalidValue;
    const auto [c, slab, grid] = split_launch(a, kTiles[tile].info, S, ws, ws_bytes);
    if (!slab) return hipErrorInvalidValue;
    if (hipError_t e = tile == 10 ? launch_split_t<2>(c, grid, S, s) : launch_split_t<1>(c, grid, S, s); e != hipSuccess) return e;
    const float *wsf = static_cast<const float *>(ws), *res = static_cast<const float *>(a.residual);
    float *dst = static_cast<float *>(a.dst);
    const bool vec = a.Cout % 4 == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)res & 15) == 0;
    const size_t n = (size_t)a.M * (vec ? a.Cout / 4 : a.Cout);
    const dim3 fgrid((unsigned)((n + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(splitk_finish_f32<true>, fgrid, dim3(256), 0, s, wsf, S, slab / 4, a.CoutPad, a.shift, res, dst, a.M, a.Cout, a.leaky);
    else
        hipLaunchKernelGGL(splitk_finish_f32<false>, fgrid, dim3(256), 0, s, wsf, S, slab / 4, a.CoutPad, a.shift, res, dst, a.M, a.Cout, a.leaky);
    return hipGetLastError();
}

TileInfo conv_tile_info(int tile) { return kTiles[(tile >= 0 && tile < TILE_COUNT) ? tile : 0].info; }

bool conv_tile_built(int tile) { return tile >= 0 && tile < TILE_COUNT && kTiles[tile].launch; }

hipError_t launch_conv_f32(const ConvArgs &a, int tile, hipStream_t s)
{
    if (!conv_tile_built(tile) || !tile_fits(kTiles[tile].info, a.Cin, a.src1 ? a.C0 : -1, a.CoutPad)) return hipErrorInvalidValue;
    return kTiles[tile].launch(a, s);
}

}  // namespace y3
