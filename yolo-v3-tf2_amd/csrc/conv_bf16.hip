// bf16 plans: the instantiations of the 16-bit implicit-GEMM conv kernel (conv_16bit.h) for bf16 elements (v_mfma_f32_32x32x16_bf16 /
// 16x16x32_bf16), the split-K form of tiles 11 and 12 with its finish launch for bf16 (the low-latency bf16 plans of
// y3_net_set_low_latency_bf16; the code is conv_16bit.h's), and what only bf16 plans have: the phase stamps of the diagnostic build.
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

#ifdef Y3_PHASE_STAMPS
extern "C" int y3_dbg_select_k(int K) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(y3_dbg_sel_k), &K, sizeof(int)); }
extern "C" int y3_dbg_copy_stamps(unsigned long long *dst, int n_words)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(y3_dbg_stamps), (size_t)n_words * sizeof(unsigned long long));
}
#endif

bool conv_bf16_split_tile(int tile) { return conv16_split_tile(tile); }

hipError_t launch_conv_bf16_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s)
{
    return launch_conv16_split<Bf16Elem>(a, tile, out_f32, S, ws, ws_bytes, s);
}

TileInfo conv_bf16_tile_info(int tile) { return Tiles16<Bf16Elem>::table[(tile >= 0 && tile < BF16_TILE_COUNT) ? tile : 0].info; }

bool conv_bf16_tile_built(int tile) { return tile >= 0 && tile < BF16_TILE_COUNT && Tiles16<Bf16Elem>::table[tile].launch; }

hipError_t launch_conv_bf16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s) { return launch_conv16<Bf16Elem>(a, tile, out_f32, s); }

}  // namespace y3
