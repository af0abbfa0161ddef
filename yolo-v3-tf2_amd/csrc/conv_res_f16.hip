// fp16 plans (Y3_DTYPE_F16): the weight-resident 3x3 / stride-1 conv (conv_res_16bit.h, tile id 32) for IEEE fp16 elements.
#include "conv_res_16bit.h"

namespace y3 {

hipError_t launch_conv_res_f16(const ConvArgs &a, hipStream_t s) { return res16::launch<F16Elem>(a, s); }

}  // namespace y3
