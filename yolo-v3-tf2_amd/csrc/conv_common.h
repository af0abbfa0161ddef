// What the implicit-GEMM MFMA conv kernels share on the device (included by the .hip files only): the rows of a tile as (image, output row,
// output column) with the A-operand offsets, the chunk swizzle of the LDS-DMA operand rows and the accumulator row mappings.  Force-inlined
// arithmetic, no state; what reads memory under conditions (set_tap, the fp32-output epilogue) stays in the kernels: DESIGN.md section 4.
#pragma once
#include "y3_device.h"
#include "y3_kernels.h"

namespace y3 {

// GEMM row m = (b * Ho + ho) * Wo + wo.  The tile's first row m0 is decomposed with wave-uniform (scalar) divisions; a lane's
// displacement d from it is folded in with an exact small float division -- vector integer division costs ~40 VALU instructions
// each, and VALU time is lost MFMA time for every wave on the SIMD.  Exactness: x = wo0 + d < BM + Wo <= 1024 and y = ho0 + qx
// likewise, so (float)x + 0.5 is exact, and the rounding of the product by the rounded reciprocal (relative error < 2^-22) cannot
// carry it across an integer: the nearest integers are >= 0.5 / Wo away, far more than x * 2^-22.
struct TileOrigin { int b0, ho0, wo0; float rcpW, rcpH; };   // (image, output row, output column) of row m0; 1 / Wo, 1 / Ho

__device__ __forceinline__ TileOrigin tile_origin(const ConvArgs &p, int m0)
{
    TileOrigin t;
    const int HoWo = p.Ho * p.Wo;
    t.b0 = m0 / HoWo;
    const int r0 = m0 - t.b0 * HoWo;
    t.ho0 = r0 / p.Wo;
    t.wo0 = r0 - t.ho0 * p.Wo;
    t.rcpW = 1.0f / (float)p.Wo;
    t.rcpH = 1.0f / (float)p.Ho;
    return t;
}

// (b, ho, wo) of the row whose column sum is x = t.wo0 + (m - m0)
__device__ __forceinline__ void tile_row(const ConvArgs &p, const TileOrigin &t, int x, int &b, int &ho, int &wo)
{
    const int qx = (int)(((float)x + 0.5f) * t.rcpW);
    wo = x - qx * p.Wo;
    const int y = t.ho0 + qx;
    const int qy = (int)(((float)y + 0.5f) * t.rcpH);
    ho = y - qy * p.Ho;
    b = t.b0 + qy;
}

// The A-operand offsets of row m as the kernels declare them (aoff, aoff1, ahw: conv_f32.hip; a row >= M gets ahw = 0x80000000); c1 = Cin - C0, EPC = stored
// elements per pixel and channel (the plane count).  The callers form m, x as (m0 + i * RP) + lrow and c1 ahead of tile_origin: formed here, conv_f32_mfma took one more SGPR.
template <bool CONCAT, int EPC>
__device__ __forceinline__ void gather_row(const ConvArgs &p, const TileOrigin &t, int m, int x, int c1, int &aoff, int &aoff1, int &ahw)
{
    int b, ho, wo;
    tile_row(p, t, x, b, ho, wo);
    if (CONCAT) {
        const int H0 = p.up0 ? (p.H >> 1) : p.H, W0 = p.up0 ? (p.W >> 1) : p.W;
        const int h0 = p.up0 ? (ho >> 1) : ho, w0 = p.up0 ? (wo >> 1) : wo;
        aoff = ((b * H0 + h0) * W0 + w0) * EPC * p.C0;
        aoff1 = ((b * p.H + ho) * p.W + wo) * EPC * c1;
        ahw = (m < p.M) ? 0 : (int)0x80000000;
    } else {
        const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
        aoff = ((b * p.H + hi0) * p.W + wi0) * EPC * p.Cin;
        ahw = (m < p.M) ? ((hi0 << 16) | (wi0 & 0xffff)) : (int)0x80000000;
    }
}

// Batch-minor rows (ConvArgs::pos_tab set, B % 32 == 0): GEMM row m = j * B + b, j an index into the position table, so each 32-row block of
// a tile is ONE output position of 32 consecutive images.  Everything here is wave-uniform: one scalar division for the tile, then compares.
// The entries behind the table (blocks of rows >= M) are zero: no live tap, position (0, 0).
struct TileBlocks { int j0, r0, n32; unsigned live; };   // block 0 of the tile: table index, 32-image group; groups per position; OR of the blocks' tap masks

__device__ __forceinline__ unsigned pos_entry(const ConvArgs &p, int j)
{
    const int n = p.Ho * p.Wo;
    return (unsigned)__builtin_amdgcn_readfirstlane((int)p.pos_tab[j < n ? j : n]);
}

template <int NBLK>
__device__ __forceinline__ TileBlocks tile_blocks(const ConvArgs &p, int m0)
{
    TileBlocks t;
    t.n32 = p.B >> 5;
    const int g0 = m0 >> 5;
    t.j0 = t.n32 == 1 ? g0 : g0 / t.n32;
    t.r0 = g0 - t.j0 * t.n32;
    t.live = 0;
    int j = t.j0, r = t.r0;
#pragma unroll
    for (int k = 0; k < NBLK; ++k) {
        t.live |= pos_mask(pos_entry(p, j));
        if (++r == t.n32) {
            r = 0;
            ++j;
        }
    }
    return t;
}

// block kb (< NBLK, wave-uniform, possibly known only at run time) of the tile: its table entry and its first image
template <int NBLK>
__device__ __forceinline__ void tile_block(const ConvArgs &p, const TileBlocks &t, int kb, unsigned &ent, int &img)
{
    int j = t.j0, r = t.r0 + kb;
#pragma unroll
    for (int w = 1; w < NBLK; ++w)   // r < n32 + NBLK - 1: at most NBLK - 1 positions further
        if (r >= t.n32) {
            r -= t.n32;
            ++j;
        }
    ent = pos_entry(p, j);
    img = r << 5;
}

// LDS-DMA operand rows of LPR 16-byte chunks (2, 4 or 8), unpadded: chunk c of row r is stored at chunk position c ^ key(r), key = (r >> shift) & (LPR - 1)
// with the shift that lets 16 consecutive rows cover all 16 slots of a 256-byte bank row.  XOR is its own inverse: the same call gives the logical chunk
// landing in a physical position (the SOURCE address of a direct-to-LDS load) and the physical position of a logical chunk (a fragment read).
template <int LPR>
__device__ __forceinline__ int swizzled_chunk(int row, int chunk)
{
    static_assert(LPR == 2 || LPR == 4 || LPR == 8, "16-byte chunks per LDS row");
    constexpr int SHIFT = (LPR == 8) ? 1 : (LPR == 4) ? 2 : 3;
    return chunk ^ ((row >> SHIFT) & (LPR - 1));
}

// Accumulator layouts, summed in the order the epilogues had (another order moves instructions).  32x32: element e of lane l is column l & 31, row mfma32_row(e, l >> 5)
__device__ __forceinline__ constexpr int mfma32_row(int e, int fh = 0) { return 4 * fh + (e & 3) + 8 * (e >> 2); }
// 16x16x32: element e (0..3) of lane l is column l & 15, row mfma16_row(e, l >> 4, mb) of a 32-row block of two (mb = 0, 1)
__device__ __forceinline__ constexpr int mfma16_row(int e, int fh, int mb = 0) { return 16 * mb + 4 * fh + e; }

}  // namespace y3
