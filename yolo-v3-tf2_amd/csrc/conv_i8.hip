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
// Split-K (low-latency int8 plans, y3_net_set_low_latency_i8; tiles 11 and 12): the SPLIT form of the kernel body stores a slice's raw i32
// accumulators into its slab [S][Mpad][CoutPad] of 4-byte elements, and splitk_finish_i8 below adds the slabs as integers and applies
// the four lines above.  i32 sums do not depend on order, so a split conv gives the unsplit conv's bits on all data and at every S.
// No weight-resident form, no BK = 32 tiles (include/y3.h).
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

// Second half of a split-K int8 conv (low-latency int8 plans): per element the S slab values added as integers -- exact, so the sum is the
// unsplit launch's accumulator whatever S is -- then the four lines of the header above through the unsplit epilogue's helpers.  int8
// output: 16 channels per thread, one 16-byte output piece, the shortcut read in the same piece (Cout % 16 == 0).  OUT_F32 (a conv that
// writes an fp32 net output itself, Cout = 255 in CoutPad = 256 included): one element per thread.
template <bool OUT_F32>
__global__ __launch_bounds__(256) void splitk_finish_i8(const int *__restrict__ ws, int S, size_t slab_elems, int cout_pad,
                                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                                        const signed char *__restrict__ residual, void *__restrict__ dst, int M, int cout,
                                                        int leaky, float q_res, float q_inv)
{
    constexpr int W = OUT_F32 ? 1 : 16;
    const int per_row = cout / W;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)M * per_row) return;
    const int m = (int)(idx / per_row);
    const int n = ((int)(idx - (size_t)m * per_row)) * W;
    const int *src = ws + (size_t)m * cout_pad + n;
    if constexpr (OUT_F32) {
        int acc = *src;
        for (int s = 1; s < S; ++s) acc += src[(size_t)s * slab_elems];
        static_cast<float *>(dst)[(size_t)m * cout + n] = bn_act((float)acc, scale[n], shift[n], leaky);
    } else {
        i32x4 acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = *reinterpret_cast<const i32x4 *>(src + 4 * k);
        for (int s = 1; s < S; ++s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += *reinterpret_cast<const i32x4 *>(src + (size_t)s * slab_elems + 4 * k);
        }
        const size_t o = (size_t)m * cout + n;
        u32x4 rr{0u, 0u, 0u, 0u};
        if (residual) rr = *reinterpret_cast<const u32x4 *>(residual + o);
        u32x4 out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(scale + n + 4 * k), sh = *reinterpret_cast<const f32x4 *>(shift + n + 4 * k);
            unsigned w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float x = bn_act((float)acc[k][b], sc[b], sh[b], leaky);
                if (residual) x = (float)I8Elem::sbyte(rr[k], b) * q_res + x;
                w |= ((unsigned)I8Elem::quant(x, q_inv) & 0xffu) << (8 * b);
            }
            out[k] = w;
        }
        *reinterpret_cast<u32x4 *>(static_cast<signed char *>(dst) + o) = out;
    }
}

bool conv_i8_split_tile(int tile) { return conv16_split_tile(tile); }

// The split launch of tile 11 / 12 (K tiles of 128) and its finish launch on the same stream, with the checks of launch_conv_i8
hipError_t launch_conv_i8_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s)
{
    if (a.K % 128 || !conv16_split_tile(tile)) return hipErrorInvalidValue;
    // the finish launch moves 16 channels per thread: whole 16-byte pieces of dst and of the shortcut
    if (!out_f32 && (a.Cout % 16 || ((uintptr_t)a.dst & 15) || ((uintptr_t)a.residual & 15))) return hipErrorInvalidValue;
    if (out_f32 && a.residual) return hipErrorInvalidValue;
    const auto [c, slab, grid] = split_launch(a, Tiles16<I8Elem>::table[tile].info, S, ws, ws_bytes);
    if (!slab) return hipErrorInvalidValue;
    if (hipError_t e = tile == 12 ? launch_split_t<I8Elem, 2>(c, grid, S, s) : launch_split_t<I8Elem, 1>(c, grid, S, s); e != hipSuccess) return e;
    const int *wsi = static_cast<const int *>(ws);
    const signed char *res = static_cast<const signed char *>(a.residual);
    const size_t n = (size_t)a.M * (out_f32 ? a.Cout : a.Cout / 16);
    const dim3 fgrid((unsigned)((n + 255) / 256));
    if (out_f32)
        hipLaunchKernelGGL((splitk_finish_i8<true>), fgrid, dim3(256), 0, s, wsi, S, slab / 4, a.CoutPad, a.scale, a.shift, res, a.dst, a.M, a.Cout, a.leaky, a.q_res, a.q_inv);
    else
        hipLaunchKernelGGL((splitk_finish_i8<false>), fgrid, dim3(256), 0, s, wsi, S, slab / 4, a.CoutPad, a.scale, a.shift, res, a.dst, a.M, a.Cout, a.leaky, a.q_res, a.q_inv);
    return hipGetLastError();
}

}  // namespace y3
