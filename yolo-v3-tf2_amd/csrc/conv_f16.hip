// fp16 plans (Y3_DTYPE_F16): the instantiations of the 16-bit implicit-GEMM conv kernel (conv_16bit.h) for IEEE fp16 elements
// (v_mfma_f32_32x32x16_f16 / 16x16x32_f16, the bf16 rate), fp32 accumulate.  Same tile table and tile ids as conv_bf16.hip
// (conv_bf16_tile_info / conv_bf16_tile_built answer for both), and the split-K form of tiles 11 and 12 with its finish launch for fp16
// (the low-latency fp16 plans of y3_net_set_low_latency_f16).  The epilogue rounds once, to nearest even, with IEEE overflow: a value
// beyond 65504 is stored as inf.
#include "conv_16bit.h"

namespace y3 {

hipError_t launch_conv_f16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s) { return launch_conv16<F16Elem>(a, tile, out_f32, s); }

hipError_t launch_conv_f16_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s)
{
    return launch_conv16_split<F16Elem>(a, tile, out_f32, S, ws, ws_bytes, s);
}

}  // namespace y3
