// bf16 plans: the weight-resident 3x3 / stride-1 conv (conv_res_16bit.h, tile id 32) for bf16 elements, and the shape rule of that kernel,
// which both 16-bit plans share.
#include "conv_res_16bit.h"

namespace y3 {

bool conv_res_bf16_fits(const ConvArgs &a) { return res16::fits(a); }

hipError_t launch_conv_res_bf16(const ConvArgs &a, hipStream_t s) { return res16::launch<Bf16Elem>(a, s); }

}  // namespace y3
