// Evaluation counters on the GPU (SURVEY.md 8f "n4"; include/y3.h, y3_evaluate_detections): the per-class pred / gt / TP / FP / FN
// counters of reference evaluate_detections.py:37-48,82-135 for a whole batch and for every NMS score threshold of the sweep of
// reference evaluate_yolov3.py:153-232, from ONE set of packed detections.  The greedy padded NMS never lets a box be affected
// by boxes scored below it, so the detections at a higher score threshold are the rows of the lowest threshold's result with
// score > threshold; only that row mask depends on the threshold.
// One 256-thread workgroup per image.  The image's ground truth is staged in LDS; a thread owns up to four packed rows and
// computes their best ground-truth row and TP decision once (they do not depend on the score threshold); then, per threshold,
// the active rows are counted into per-class LDS counters, and the non-zero ones are added to the caller's int64 counters with
// 64-bit vector atomic adds.  Integer adds commute: the result does not depend on the order the workgroups arrive in.
// IoU in fp32, each operation rounded on its own (the library is built with -ffp-contract=off), minimum / maximum and arg-max
// with NumPy's NaN rules (box_iou.h, the body ap_match.hip shares): host restatement evaluate_detections.sweep_counters, bit for bit.
#include "box_iou.h"
#include "y3_kernels.h"

namespace y3 {

namespace {

constexpr int kEvalThreads = 256;
constexpr int kEvalRowsPerThread = kEvalMaxBoxes / kEvalThreads;
static_assert(kEvalRowsPerThread * kEvalThreads == kEvalMaxBoxes, "a thread owns max_boxes / 256 rows");

}  // namespace

// LDS: gt boxes [max_gt][4] f32 | gt classes [max_gt] i32 | assigned bits [max_gt / 32 rounded up] | counts [5 * nc] u32
// (preds, gts, tp, fp, fn: the order of a counters row)
__global__ __launch_bounds__(kEvalThreads) void evaluate_kernel(const unsigned *__restrict__ packed, const int32_t *__restrict__ nv,
                                                                int M, const float *__restrict__ gt_boxes,
                                                                const int32_t *__restrict__ gt_classes,
                                                                const int32_t *__restrict__ gt_count, int G, int nc, float iou_thr,
                                                                EvalThresholds thr, int T, int one_class,
                                                                unsigned long long *__restrict__ counters)
{
    extern __shared__ __align__(16) unsigned char lds[];
    float *s_box = reinterpret_cast<float *>(lds);
    int *s_cls = reinterpret_cast<int *>(s_box + (size_t)G * 4);
    const int mask_words = (G + 31) >> 5;
    unsigned *s_assigned = reinterpret_cast<unsigned *>(s_cls + G);
    unsigned *s_cnt = s_assigned + mask_words;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(nv[b], 0), M), g_n = min(max(gt_count[b], 0), G);
    const size_t row_words = (size_t)5 * nc + 2;

    // stage the ground truth; a class outside [0, nc) makes the image an error image at every threshold
    const float *gb = gt_boxes + (size_t)b * G * 4;
    const int32_t *gc = gt_classes + (size_t)b * G;
    for (int i = tid; i < g_n * 4; i += kEvalThreads) s_box[i] = gb[i];
    int bad = 0;
    for (int i = tid; i < g_n; i += kEvalThreads) {
        const int c = one_class ? 0 : gc[i];
        s_cls[i] = c;
        bad |= (c < 0 || c >= nc);
    }
    const int gt_bad = __syncthreads_or(bad);
    if (gt_bad) {
        if (tid < T) atomicAdd(counters + (size_t)tid * row_words + 5 * (size_t)nc, 1ull);   // errors
        return;
    }

    // per owned row: score, class, best ground-truth row (first maximum, a NaN counts as the maximum) and the TP decision
    float score[kEvalRowsPerThread];
    int cls[kEvalRowsPerThread], best[kEvalRowsPerThread];
    bool decision[kEvalRowsPerThread];
#pragma unroll
    for (int k = 0; k < kEvalRowsPerThread; ++k) {
        const int r = tid + k * kEvalThreads;
        score[k] = 0.0f;
        cls[k] = 0;
        best[k] = -1;
        decision[k] = false;
        if (r < n) {
            const unsigned *o = packed + ((size_t)b * M + r) * 7;
            const float x1 = __uint_as_float(o[0]), y1 = __uint_as_float(o[1]);
            const float x2 = __uint_as_float(o[2]), y2 = __uint_as_float(o[3]);
            score[k] = __uint_as_float(o[4]);
            cls[k] = one_class ? 0 : (int)o[5];
            const float a1 = (x2 - x1) * (y2 - y1);
            float bv = 0.0f;
            for (int g = 0; g < g_n; ++g) {
                const float4 q = *reinterpret_cast<const float4 *>(s_box + g * 4);   // every lane reads the same row: a broadcast
                const float iou = box_iou(x1, y1, x2, y2, a1, q);
                if (g == 0 || (bv == bv && !(iou <= bv))) {   // np.argmax: the first NaN ends the search
                    bv = iou;
                    best[k] = g;
                }
            }
            decision[k] = g_n > 0 && bv > iou_thr && s_cls[best[k]] == cls[k];
        }
    }

    for (int t = 0; t < T; ++t) {
        const float s_t = thr.s[t];
        for (int i = tid; i < 5 * nc; i += kEvalThreads) s_cnt[i] = 0;
        for (int i = tid; i < mask_words; i += kEvalThreads) s_assigned[i] = 0;
        // a prediction class outside [0, nc) among the rows of this threshold: an error image at this threshold
        int bad_pred = 0;
#pragma unroll
        for (int k = 0; k < kEvalRowsPerThread; ++k)
            bad_pred |= (tid + k * kEvalThreads < n && score[k] > s_t && (cls[k] < 0 || cls[k] >= nc));
        if (__syncthreads_or(bad_pred)) {   // (also the barrier behind the zeroing)
            if (tid == 0) atomicAdd(counters + (size_t)t * row_words + 5 * (size_t)nc, 1ull);
            continue;
        }
#pragma unroll
        for (int k = 0; k < kEvalRowsPerThread; ++k) {
            if (tid + k * kEvalThreads < n && score[k] > s_t) {
                atomicAdd(&s_cnt[cls[k]], 1u);                                   // preds
                atomicAdd(&s_cnt[(decision[k] ? 2 : 3) * nc + cls[k]], 1u);      // tp / fp
                if (decision[k]) atomicOr(&s_assigned[best[k] >> 5], 1u << (best[k] & 31));
            }
        }
        __syncthreads();
        for (int g = tid; g < g_n; g += kEvalThreads) {
            const int c = s_cls[g];
            atomicAdd(&s_cnt[nc + c], 1u);                                       // gts
            if (!((s_assigned[g >> 5] >> (g & 31)) & 1u)) atomicAdd(&s_cnt[4 * nc + c], 1u);   // fn
        }
        __syncthreads();
        unsigned long long *row = counters + (size_t)t * row_words;
        for (int i = tid; i < 5 * nc; i += kEvalThreads) {
            const unsigned v = s_cnt[i];
            if (v) atomicAdd(row + i, (unsigned long long)v);
        }
        if (tid == 0) atomicAdd(row + 5 * (size_t)nc + 1, 1ull);                 // examples
        __syncthreads();   // the counts are zeroed again at the top
    }
}

size_t evaluate_lds_bytes(int max_gt, int nclasses)
{
    return (size_t)max_gt * 20 + (size_t)((max_gt + 31) / 32) * 4 + (size_t)nclasses * 20;
}

hipError_t launch_evaluate(const void *packed, const int32_t *nv, int B, int M, const float *gt_boxes, const int32_t *gt_classes,
                           const int32_t *gt_count, int G, int nc, float iou_thr, const EvalThresholds &thr, int T, int one_class,
                           int64_t *counters, hipStream_t s)
{
    const size_t lds = evaluate_lds_bytes(G, nc);
    // 4 KB at 100 rows of ground truth and 80 classes; only a launch beyond the 64 KB every kernel may use (more than ~2000 classes)
    // raises the kernel's limit, once per device, to what the largest admitted arguments need (100 KB of the CU's 160)
    static LdsAttrOnce attr;
    if (lds > 64 * 1024)
        if (hipError_t e = set_max_lds_once(attr, reinterpret_cast<const void *>(evaluate_kernel),
                                            (int)evaluate_lds_bytes(kEvalMaxGt, kEvalMaxClasses)); e != hipSuccess)
            return e;
    hipLaunchKernelGGL(evaluate_kernel, dim3((unsigned)B), dim3(kEvalThreads), lds, s, static_cast<const unsigned *>(packed), nv, M,
                       gt_boxes, gt_classes, gt_count, G, nc, iou_thr, thr, T, one_class,
                       reinterpret_cast<unsigned long long *>(counters));
    return hipGetLastError();
}

}  // namespace y3
