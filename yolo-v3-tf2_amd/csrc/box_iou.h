// The IoU of a packed detection row with a ground-truth row, shared by the counters kernel (evaluate.hip) and the AP matching
// kernel (ap_match.hip): ONE body, so that both judge a pair of boxes by the same bits.
// reference: evaluate_detections.py:39-49 (iou_alg: no epsilon in the union).  fp32, every operation rounded on its own
// (-ffp-contract=off), a true division, minimum / maximum with NumPy's NaN rules.
#pragma once
#include <hip/hip_runtime.h>

namespace y3 {

// np.maximum / np.minimum: a NaN in either operand is the result
__device__ __forceinline__ float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }

// (x1, y1, x2, y2) with its area a1 = (x2 - x1) * (y2 - y1) against q = {xmin, ymin, xmax, ymax}: inter / ((a1 + a2) - inter)
__device__ __forceinline__ float box_iou(float x1, float y1, float x2, float y2, float a1, const float4 &q)
{
    const float ow = np_max(np_min(x2, q.z) - np_max(x1, q.x), 0.0f);
    const float oh = np_max(np_min(y2, q.w) - np_max(y1, q.y), 0.0f);
    const float inter = ow * oh;
    const float a2 = (q.z - q.x) * (q.w - q.y);
    return inter / ((a1 + a2) - inter);
}

}  // namespace y3
