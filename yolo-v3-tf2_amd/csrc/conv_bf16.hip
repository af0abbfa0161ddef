// bf16 plans: the instantiations of the 16-bit implicit-GEMM conv kernel (conv_16bit.h) for bf16 elements (v_mfma_f32_32x32x16_bf16 /
// 16x16x32_bf16), and what only bf16 plans have: the split-K form of tiles 11 and 12 with its finish launch (the low-latency bf16 plans of
// y3_net_set_low_latency_bf16) and the phase stamps of the diagnostic build.
#include "conv_common.h"

namespace y3 {
#ifdef Y3_PHASE_STAMPS
// Diagnostic build only (csrc/build.py --variant ... -DY3_PHASE_STAMPS, tools/phase_stamps.py): thread 0 of every workgroup of the
// launches whose K equals y3_dbg_sel_k stores s_memrealtime (100 MHz) at kernel entry, before the first fetch, after the first
// barrier, after the K loop and after the epilogue, plus HW_ID / XCC_ID, into a buffer no other code reads.
__device__ unsigned long long y3_dbg_stamps[8 * 8192];
__device__ int y3_dbg_sel_k = -1;
#define Y3_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192 && p.K == y3_dbg_sel_k) y3_dbg_stamps[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define Y3_STAMP_IDS() do { if (threadIdx.x == 0 && blockIdx.x < 8192 && p.K == y3_dbg_sel_k) { \
        y3_dbg_stamps[blockIdx.x * 8 + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    /* HW_REG_HW_ID */ \
        y3_dbg_stamps[blockIdx.x * 8 + 6] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   /* HW_REG_XCC_ID */ } } while (0)
#endif
}  // namespace y3

#include "conv_16bit.h"

namespace y3 {

// Second half of a split-K conv: per element slab[0] + slab[1] + ... + slab[S-1], added in that order, then exactly the unsplit epilogue's
// operations through the same helpers (bn_act, add_res_pack).  bf16 output: eight channels per thread, 16-byte loads and stores
// (Cout % 8 == 0).  OUT_F32 (a conv that writes an fp32 net output itself, Cout = 255 in CoutPad = 256 included): one element per thread.
template <bool OUT_F32>
__global__ __launch_bounds__(256) void splitk_finish_bf16(const float *__restrict__ ws, int S, size_t slab_elems, int cout_pad,
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
        *reinterpret_cast<u32x4 *>(static_cast<unsigned short *>(dst) + o) = add_res_pack<Bf16Elem>(v, rr, residual != nullptr);
    }
}

#ifdef Y3_PHASE_STAMPS
extern "C" int y3_dbg_select_k(int K) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(y3_dbg_sel_k), &K, sizeof(int)); }
extern "C" int y3_dbg_copy_stamps(unsigned long long *dst, int n_words)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(y3_dbg_stamps), (size_t)n_words * sizeof(unsigned long long));
}
#endif

// The split-K form is instantiated for the two tiles a small plan lands on: 11 (64x64) and 12 (64x128), both LDS-DMA, BK 64, four waves
template <int TN>
static hipError_t launch_split_t(const ConvArgs &c, int grid, int S, hipStream_t s)
{
    constexpr size_t lds = 2 * (size_t)(64 + 64 * TN) * 128;   // the two operand stages; a split launch has no epilogue tile
    if (c.src1) return launch_conv_kernel<conv16_mfma<Bf16Elem, 1, TN, 2, 2, 64, true, false, true, 1, false, true>>(c, grid, 256, lds, s, S);
    return launch_conv_kernel<conv16_mfma<Bf16Elem, 1, TN, 2, 2, 64, false, false, true, 1, false, true>>(c, grid, 256, lds, s, S);
}

bool conv_bf16_split_tile(int tile) { return tile == 11 || tile == 12; }

hipError_t launch_conv_bf16_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s)
{
    if (!conv_bf16_split_tile(tile)) return hipErrorInvalidValue;
    const auto [c, slab, grid] = split_launch(a, Tiles16<Bf16Elem>::table[tile].info, S, ws, ws_bytes);
    if (!slab) return hipErrorInvalidValue;
    // the bf16 form of the finish launch moves eight channels per thread: whole 16-byte pieces of dst and of the shortcut
    if (!out_f32 && (a.Cout % 8 || ((uintptr_t)a.dst & 15) || ((uintptr_t)a.residual & 15))) return hipErrorInvalidValue;
    if (out_f32 && a.residual) return hipErrorInvalidValue;
    if (hipError_t e = tile == 12 ? launch_split_t<2>(c, grid, S, s) : launch_split_t<1>(c, grid, S, s); e != hipSuccess) return e;
    const float *wsf = static_cast<const float *>(ws);
    const unsigned short *res = static_cast<const unsigned short *>(a.residual);
    const size_t n = (size_t)a.M * (out_f32 ? a.Cout : a.Cout / 8);
    const dim3 fgrid((unsigned)((n + 255) / 256));
    if (out_f32)
        hipLaunchKernelGGL(splitk_finish_bf16<true>, fgrid, dim3(256), 0, s, wsf, S, slab / 4, a.CoutPad, a.scale, a.shift, res, a.dst, a.M, a.Cout, a.leaky);
    else
        hipLaunchKernelGGL(splitk_finish_bf16<false>, fgrid, dim3(256), 0, s, wsf, S, slab / 4, a.CoutPad, a.scale, a.shift, res, a.dst, a.M, a.Cout, a.leaky);
    return hipGetLastError();
}

TileInfo conv_bf16_tile_info(int tile) { return Tiles16<Bf16Elem>::table[(tile >= 0 && tile < BF16_TILE_COUNT) ? tile : 0].info; }

bool conv_bf16_tile_built(int tile) { return tile >= 0 && tile < BF16_TILE_COUNT && Tiles16<Bf16Elem>::table[tile].launch; }

hipError_t launch_conv_bf16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s) { return launch_conv16<Bf16Elem>(a, tile, out_f32, s); }

}  // namespace y3
