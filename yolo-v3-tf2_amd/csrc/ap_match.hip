// Greedy matching of detections to ground truth for average precision (include/y3.h, y3_match_detections): per image and per IoU
// threshold, the packed rows are walked in row order (y3_net_detect writes them in descending score) and each takes the free
// ground-truth row of its class with the largest IoU >= threshold, the higher row on a tie; a ground-truth row is taken at most
// once per threshold.  No reference counterpart: the rule is this project's statement of the COCO matching.
// One workgroup per image, ONE wave per IoU threshold: the walk is serial over the rows and needs no barrier.  The image's ground
// truth and its rows are staged in LDS; lane l of a wave owns the ground-truth rows l, l + 64, ... and keeps their "taken" bits in
// a register (16 bits at max_gt = 1024); the winner of a row is found by a wave reduction over (IoU, g) -- skipped when no lane
// or one lane has a candidate, the common cases -- and lane 0 sets bit k of the row's LDS mask word.  After one barrier every
// record slot of the image is written (fixed slots, no cursor: the record order is a function of the input order alone) and the
// ground-truth rows per class go to the caller's int64 totals with 64-bit vector atomic adds of the non-zero LDS counts.
// IoU: box_iou.h, the body evaluate_kernel uses.  Host restatement evaluate_detections.match_detections, bit for bit.
#include "box_iou.h"
#include "y3_kernels.h"

namespace y3 {

namespace {
constexpr int kWave = 64;
static_assert(kEvalMaxGt <= 32 * kWave, "a lane keeps the taken bits of max_gt / 64 ground-truth rows in one 32-bit register");
static_assert(kEvalMaxThresholds * kWave <= 1024, "one wave per IoU threshold in one workgroup");
static_assert(kEvalMaxClasses <= 0x10000, "a record holds the class in its low 16 bits");
}  // namespace

// LDS: gt boxes [G][4] f32 | row boxes [M][4] f32 | gt classes [G] i32 | row classes [M] i32 | row masks [M] u32 | gt per class [nc] u32
__global__ __launch_bounds__(kEvalMaxThresholds * kWave) void ap_match_kernel(
    const unsigned *__restrict__ packed, const int32_t *__restrict__ nv, int M, const float *__restrict__ gt_boxes,
    const int32_t *__restrict__ gt_classes, const int32_t *__restrict__ gt_count, int G, int nc, EvalThresholds thr, int one_class,
    uint2 *__restrict__ records, unsigned long long *__restrict__ totals)
{
    extern __shared__ __align__(16) unsigned char lds[];
    float *s_box = reinterpret_cast<float *>(lds);
    float *s_row = s_box + (size_t)G * 4;
    int *s_gcls = reinterpret_cast<int *>(s_row + (size_t)M * 4);
    int *s_rcls = s_gcls + G;
    unsigned *s_mask = reinterpret_cast<unsigned *>(s_rcls + M);
    unsigned *s_cnt = s_mask + M;

    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;      // nt = 64 n_iou
    const int n = min(max(nv[b], 0), M), g_n = min(max(gt_count[b], 0), G);
    const unsigned *rows = packed + (size_t)b * M * 7;
    uint2 *rec = records + (size_t)b * M;

    // stage the ground truth and the rows; a class outside [0, nc) on either side makes the image an error image
    const float *gb = gt_boxes + (size_t)b * G * 4;
    const int32_t *gc = gt_classes + (size_t)b * G;
    for (int i = tid; i < g_n * 4; i += nt) s_box[i] = gb[i];
    int bad = 0;
    for (int i = tid; i < g_n; i += nt) {
        const int c = one_class ? 0 : gc[i];
        s_gcls[i] = c;
        bad |= (c < 0 || c >= nc);
    }
    for (int r = tid; r < n; r += nt) {
        const unsigned *o = rows + (size_t)r * 7;
        *reinterpret_cast<float4 *>(s_row + r * 4) =
            make_float4(__uint_as_float(o[0]), __uint_as_float(o[1]), __uint_as_float(o[2]), __uint_as_float(o[3]));
        const int c = one_class ? 0 : (int)o[5];
        s_rcls[r] = c;
        bad |= (c < 0 || c >= nc);
    }
    for (int r = tid; r < M; r += nt) s_mask[r] = 0;
    for (int i = tid; i < nc; i += nt) s_cnt[i] = 0;
    if (__syncthreads_or(bad)) {
        for (int r = tid; r < M; r += nt) rec[r] = make_uint2(0u, 0xFFFFFFFFu);
        if (tid == 0) atomicAdd(totals + nc, 1ull);                      // errors
        return;
    }
    for (int g = tid; g < g_n; g += nt) atomicAdd(&s_cnt[s_gcls[g]], 1u);

    // wave k walks the rows at threshold k
    const int k = tid >> 6, lane = tid & (kWave - 1);
    const float t = thr.s[k];
    const int slots = (g_n + kWave - 1) >> 6;
    unsigned taken = 0;                                                   // bit j: ground-truth row lane + 64 j
    // the lane's first ground-truth row stays in registers (all of them up to 64 rows of ground truth), and the next row is read
    // while this one is decided: the serial chain of a row is then the IoU arithmetic and the vote alone
    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int c0 = -1;                                                          // no row class is negative here
    if (lane < g_n) {
        q0 = *reinterpret_cast<const float4 *>(s_box + lane * 4);
        c0 = s_gcls[lane];
    }
    float4 p_next = q0;
    int c_next = 0;
    const int n_walk = g_n > 0 ? n : 0;                                   // without ground truth no row matches: nothing to walk
    if (n_walk > 0) {
        p_next = *reinterpret_cast<const float4 *>(s_row);                // every lane reads the same row: a broadcast
        c_next = s_rcls[0];
    }
    for (int r = 0; r < n_walk; ++r) {
        const float4 p = p_next;
        const int c = c_next;
        if (r + 1 < n_walk) {
            p_next = *reinterpret_cast<const float4 *>(s_row + (r + 1) * 4);
            c_next = s_rcls[r + 1];
        }
        const float a1 = (p.z - p.x) * (p.w - p.y);
        float bv = 0.0f;
        int bg = -1;
        if (c0 == c && !(taken & 1u)) {
            const float v = box_iou(p.x, p.y, p.z, p.w, a1, q0);
            if (v >= t) {                                                 // a NaN never qualifies
                bv = v;
                bg = lane;
            }
        }
        for (int j = 1; j < slots; ++j) {
            const int g = lane + (j << 6);
            if (g < g_n && !((taken >> j) & 1u) && s_gcls[g] == c) {
                const float v = box_iou(p.x, p.y, p.z, p.w, a1, *reinterpret_cast<const float4 *>(s_box + g * 4));
                if (v >= t && (bg < 0 || v >= bv)) {                     // the higher g on a tie
                    bv = v;
                    bg = g;
                }
            }
        }
        const unsigned long long have = __ballot(bg >= 0);
        if (!have) continue;
        if (have & (have - 1)) {                                          // several lanes: the largest (IoU, g), into every lane
#pragma unroll
            for (int m = 1; m < kWave; m <<= 1) {
                const float ov = __shfl_xor(bv, m);
                const int og = __shfl_xor(bg, m);
                if (og >= 0 && (bg < 0 || ov > bv || (ov == bv && og > bg))) {
                    bv = ov;
                    bg = og;
                }
            }
        }
        if (bg >= 0 && (bg & (kWave - 1)) == lane) taken |= 1u << (bg >> 6);   // the owner of the winner (with one candidate, only it has bg >= 0)
        if (lane == 0) atomicOr(&s_mask[r], 1u << k);
    }
    __syncthreads();

    for (int r = tid; r < M; r += nt)
        rec[r] = r < n ? make_uint2(rows[(size_t)r * 7 + 4], (unsigned)s_rcls[r] | (s_mask[r] << 16)) : make_uint2(0u, 0xFFFFFFFFu);
    for (int i = tid; i < nc; i += nt) {
        const unsigned v = s_cnt[i];
        if (v) atomicAdd(totals + i, (unsigned long long)v);
    }
    if (tid == 0) atomicAdd(totals + nc + 1, 1ull);                      // images
}

size_t ap_match_lds_bytes(int max_boxes, int max_gt, int nclasses)
{
    return (size_t)max_gt * 20 + (size_t)max_boxes * 24 + (size_t)nclasses * 4;
}
static_assert((size_t)kEvalMaxGt * 20 + (size_t)kEvalMaxBoxes * 24 + (size_t)kEvalMaxClasses * 4 <= 64 * 1024,
              "the largest admitted launch stays inside the 64 KB every kernel may use");

hipError_t launch_ap_match(const void *packed, const int32_t *nv, int B, int M, const float *gt_boxes, const int32_t *gt_classes,
                           const int32_t *gt_count, int G, int nc, const EvalThresholds &thr, int K, int one_class, uint32_t *records,
                           int64_t *totals, hipStream_t s)
{
    hipLaunchKernelGGL(ap_match_kernel, dim3((unsigned)B), dim3((unsigned)(K * kWave)), ap_match_lds_bytes(M, G, nc), s,
                       static_cast<const unsigned *>(packed), nv, M, gt_boxes, gt_classes, gt_count, G, nc, thr, one_class,
                       reinterpret_cast<uint2 *>(records), reinterpret_cast<unsigned long long *>(totals));
    return hipGetLastError();
}

}  // namespace y3
