// fp16 plans (Y3_DTYPE_F16): the instantiations of the 16-bit implicit-GEMM conv kernel (conv_16bit.h) for IEEE fp16 elements
// (v_mfma_f32_32x32x16_f16 / 16x16x32_f16, the bf16 rate), fp32 accumulate.  Same tile table and tile ids as conv_bf16.hip
// (conv_bf16_tile_info / conv_bf16_tile_built answer for both); no split-K form: fp16 plans never split.  The epilogue rounds once, to
// nearest even, with IEEE overflow: a value beyond 65504 is stored as inf.
#include "conv_16bit.h"

namespace y3 {

hipError_t launch_conv_f16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s) { return launch_conv16<F16Elem>(a, tile, out_f32, s); }

}  // namespace y3
