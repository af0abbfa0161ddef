// int8 plans (Y3_DTYPE_I8): implicit-GEMM convolution with int8 operands on the gfx950 matrix cores, exact i32 accumulate
// (v_mfma_i32_32x32x32_i8 / v_mfma_i32_16x16x64_i8: the cycles of the bf16 forms at twice the K).  A third element type, I8Elem, of the one
// kernel body of conv_16bit.h (conv16_mfma<E, ...>), which counts rows, fragments and pieces in bytes.  What int8 shares with the 16-bit types:
//   * activations NHWC, weights packed [CoutPad][K] (k = tap*Cin + c); the tile decomposition, the A-row gather, the K walk, the launchers;
//   * K tile = 128 bytes per row (BK = 128 channels), LDS-DMA only: unpadded 128-B rows, 16-B chunk XOR-swizzled, double buffered;
//   * a lane's operand is 16 bytes from row l & 31, piece 2s + (l >> 5) (32x32x32) or row l & 15, piece 4s + (l >> 4) (16x16x64) -- the places a
//     bf16 fragment comes from.  A and B take their k from the same byte offsets and integer sums do not depend on order, so whatever k
//     order the instruction gives the 16 bytes cancels;
//   * accumulator layouts (mfma32_row / mfma16_row: C/D maps do not depend on the element type), the per-wave transposing epilogue and the
//     workgroup-wide fp32 epilogue of the head grids with the in-tile head decode.
// What differs: the traits below, the tiles built (the ten with 128-byte rows), three launch checks, the head convs' prologue (gather_row,
// not the 16-bit types' written-out one) and the epilogue's arithmetic ("int8 plans", the scheme kernel and NumPy
// restatement share):
//   v = (float)acc * sc[c] + sh[c]      two roundings, never contracted
//   v = max(v, 0.1f * v)                when leaky
//   v = (float)r * q_res + v            when there is a shortcut; r the int8 shortcut value, q_res its tensor's scale
//   q = clamp(rintf(v * q_inv), -127, 127)
// int8 output: 16 channels per 16-byte piece, the shortcut read in the same pieces.  fp32 output (head grids): v stored as is.
// No split-K, no weight-resident form, no BK = 32 tiles (include/y3.h).
#include "conv_16bit.h"

namespace y3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

struct I8Elem {
    using frag = i32x4;   // sixteen elements
    using acc32 = i32x16;
    using acc16 = i32x4;
    using stored = signed char;
    static constexpr int BYTES = 1;
    static __device__ __forceinline__ i32x16 mfma32(frag a, frag b, i32x16 c) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ i32x4 mfma16(frag a, frag b, i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
    // symmetric int8: round to nearest even, clamp to [-127, 127]
    static __device__ __forceinline__ int quant(float v, float inv) { return (int)fminf(fmaxf(rintf(v * inv), -127.0f), 127.0f); }
    // byte b (0..3) of word w as a signed value
    static __device__ __forceinline__ int sbyte(unsigned w, int b) { return (int)(w << (24 - 8 * b)) >> 24; }
};

template <int TM, int TN, int WR, int WC, bool M16 = false>
static constexpr Tile16 tile_i8() { return tile<I8Elem, TM, TN, WR, WC, 128, true, 1, M16>(); }

// The ids of the 16-bit table for the tiles that have an int8 form: the LDS-DMA tiles with 128-byte rows, both MFMA shapes.
// bk is in channels = bytes: 128.  (inline: a discardable definition, like the implicit instantiations of the 16-bit tables -- the device pass
// would otherwise emit this constant table with its references to the host-side launchers.)
template <> inline const Tile16 Tiles16<I8Elem>::table[BF16_TILE_COUNT] = {
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

TileInfo conv_i8_tile_info(int tile) { return (tile >= 0 && tile < BF16_TILE_COUNT) ? Tiles16<I8Elem>::table[tile].info : TileInfo{}; }
bool conv_i8_tile_built(int tile) { return tile >= 0 && tile < BF16_TILE_COUNT && Tiles16<I8Elem>::table[tile].launch != nullptr; }

hipError_t launch_conv_i8(const ConvArgs &a, int tile, bool out_f32, hipStream_t s)
{
    if (a.K % 128) return hipErrorInvalidValue;
    // the int8 epilogue moves 16 channels per piece: whole 16-byte pieces of dst and of the shortcut
    if (!out_f32 && (a.Cout % 16 || ((uintptr_t)a.dst & 15) || ((uintptr_t)a.residual & 15))) return hipErrorInvalidValue;
    if (out_f32 && a.residual) return hipErrorInvalidValue;
    return launch_conv16<I8Elem>(a, tile, out_f32, s);
}

}  // namespace y3
