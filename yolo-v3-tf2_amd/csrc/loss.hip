// Validation loss on the GPU (include/y3.h, y3_yolo_assign_targets / y3_yolo_loss): the label assignment of reference
// core/preprocess_dataset.py:19-92 (_arrange_in_grid) in its sparse form, and the four loss sums of core/loss_func.py:19-69 per
// image and scale, from the raw head grids of y3_net_forward.  No gradient is taken: this scores a weight file, it does not train.
//
// assign_targets_kernel: one 256-thread workgroup per image, a thread per ground-truth row.  Each row picks its anchor (first
// maximum of the nine width/height IoUs) and its cell; the rows' cell keys go to LDS, where a row loses its cell to any later
// row with the same key (tensor_scatter_nd_update applies its updates in order).  Only the keys are shared between rows, so only
// they are staged: a row's box is read once, by its own thread.
//
// yolo_loss_kernel: one 1024-thread workgroup per (image, scale).  The image's assigned rows of this scale are marked in an LDS
// bitmap of 3 g^2 bits; a wave per assigned row computes its xy / wh / class terms (lanes over the classes) into LDS; then every
// thread sweeps channel 4 of its rows n = tid, tid + 1024, ... for the objectness term and, at a marked row, picks up that row's
// three terms.  The fp32 terms are summed in fp64: per thread in sweep order, then down the wave by shuffles, then over the 16
// waves in order -- an order fixed by the grid size alone, so an image's twelve sums do not depend on the batch around it, on
// max_gt or on the order of its ground-truth rows.  No atomics on floating-point values anywhere.
// fp32 arithmetic, each operation rounded on its own (the library is built with -ffp-contract=off).
#include <algorithm>

#include "y3_kernels.h"

namespace y3 {

namespace {

constexpr int kAssignThreads = 256;
constexpr int kLossThreads = 1024, kLossWaves = kLossThreads / 64;
constexpr int kSweepBatch = 4;   // channel-4 loads a thread has in flight
constexpr float kEps = 1e-7f, kHi = 1.0f - 1e-7f;   // Keras' epsilon() and 1 - epsilon() in fp32

// Keras clips a probability to [eps, 1 - eps] before it takes a logarithm of it
__device__ __forceinline__ float clipped_sigmoid(float x) { return fminf(fmaxf(sigmoidf_(x), kEps), kHi); }

}  // namespace

__global__ __launch_bounds__(kAssignThreads) void assign_targets_kernel(const float *__restrict__ gt_boxes,
                                                                        const int32_t *__restrict__ gt_classes,
                                                                        const int32_t *__restrict__ gt_count, int G, int nc,
                                                                        LossGeom geo, int32_t *__restrict__ cells)
{
    extern __shared__ __align__(16) unsigned char lds[];
    int *s_key = reinterpret_cast<int *>(lds);   // [G]: the row's index in decode's row order, -1 without one

    const int b = blockIdx.x, tid = threadIdx.x;
    const int count = min(max(gt_count[b], 0), G);
    const float *gb = gt_boxes + (size_t)b * G * 4;
    const int32_t *gc = gt_classes + (size_t)b * G;

    int bad = 0;
    for (int r = tid; r < G; r += kAssignThreads) {
        int key = -1;
        if (r < count) {
            const float x1 = gb[r * 4 + 0], y1 = gb[r * 4 + 1], x2 = gb[r * 4 + 2], y2 = gb[r * 4 + 3];
            const int c = gc[r];
            const float w = x2 - x1, h = y2 - y1;
            // the first maximum of the nine IoUs: a later anchor wins only when strictly greater (a NaN never wins)
            int best = 0;
            float bv = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float aw = geo.anchors[k / 3][k % 3][0], ah = geo.anchors[k / 3][k % 3][1];
                const float inter = fminf(w, aw) * fminf(h, ah);
                const float iou = inter / ((w * h + aw * ah) - inter);
                if (k == 0 || iou > bv) {
                    bv = iou;
                    best = k;
                }
            }
            const int s = best / 3, a = best - s * 3;
            const int g = geo.g[s];
            const float fx = ((x1 + x2) / 2) * (float)g, fy = ((y1 + y2) / 2) * (float)g;
            // (int) truncates toward zero like tf.cast: the cell is inside [0, g) exactly when -1 < f < g (false for a NaN)
            const bool ok = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && c >= 0 && c < nc &&
                            fx > -1.0f && fx < (float)g && fy > -1.0f && fy < (float)g;
            if (ok)
                key = geo.off[s] + ((int)fy * g + (int)fx) * 3 + a;
            else
                bad = 1;
        }
        s_key[r] = key;
    }
    const int error_image = __syncthreads_or(bad);   // (also the barrier behind the keys)

    int32_t *out = cells + (size_t)b * G;
    for (int r = tid; r < G; r += kAssignThreads) {
        int v = -1;
        if (r < count) {
            if (error_image) {
                v = -3;
            } else {
                v = s_key[r];
                for (int q = r + 1; q < count; ++q)
                    if (s_key[q] == v) {   // a later row took the cell
                        v = -2;
                        break;
                    }
            }
        }
        out[r] = v;
    }
}

// LDS: wave sums [16][4] f64 | cell of row r inside this scale [G] i32 (-1: none) | terms [G][3] f32 (xy, wh, class) | bitmap
__global__ __launch_bounds__(kLossThreads) void yolo_loss_kernel(LossGrids grids, LossGeom geo, int nc,
                                                                 const float *__restrict__ gt_boxes,
                                                                 const int32_t *__restrict__ gt_classes,
                                                                 const int32_t *__restrict__ cells, int G, double *__restrict__ loss)
{
    extern __shared__ __align__(16) unsigned char lds[];
    double *s_red = reinterpret_cast<double *>(lds);
    int *s_cell = reinterpret_cast<int *>(s_red + kLossWaves * 4);
    float *s_term = reinterpret_cast<float *>(s_cell + G);
    unsigned *s_bits = reinterpret_cast<unsigned *>(s_term + (size_t)G * 3);

    const int b = blockIdx.x / 3, s = blockIdx.x - b * 3, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = geo.g[s], rows = 3 * g * g, off = geo.off[s], F = 5 + nc;
    const float *grid = grids.p[s] + (size_t)b * rows * F;
    const float *gb = gt_boxes + (size_t)b * G * 4;
    const int32_t *gc = gt_classes + (size_t)b * G;
    const int32_t *cl = cells + (size_t)b * G;
    double *out = loss + ((size_t)b * 3 + s) * 4;

    for (int i = tid; i < (rows + 31) >> 5; i += kLossThreads) s_bits[i] = 0;
    int bad = 0;
    for (int r = tid; r < G; r += kLossThreads) {
        const int v = cl[r];
        int n = v - off;
        if (v < 0 || n < 0 || n >= rows) n = -1;   // no cell, or a cell of another scale (or of no scale: never dereferenced)
        // an error image of y3_yolo_assign_targets; an assigned row (of any scale: the three workgroups of the image agree) whose
        // class cannot index its logits makes one here as well
        bad |= (v == -3) || (v >= 0 && (gc[r] < 0 || gc[r] >= nc));
        s_cell[r] = n;
    }
    if (__syncthreads_or(bad)) {   // (also the barrier behind the zeroed bitmap and the cells)
        if (tid < 4) out[tid] = 0.0;
        return;
    }
    for (int r = tid; r < G; r += kLossThreads) {
        const int n = s_cell[r];
        if (n >= 0) atomicOr(&s_bits[n >> 5], 1u << (n & 31));
    }

    // a wave per assigned row: xy, wh (every lane computes the same values) and the class term (lanes over the classes)
    for (int r = wave; r < G; r += kLossWaves) {
        const int n = s_cell[r];
        if (n < 0) continue;   // wave-uniform
        const int cell = n / 3, a = n - cell * 3, row = cell / g, col = cell - row * g;
        const float *t = grid + (size_t)n * F;
        const float x1 = gb[r * 4 + 0], y1 = gb[r * 4 + 1], x2 = gb[r * 4 + 2], y2 = gb[r * 4 + 3];
        const float tw = x2 - x1, th = y2 - y1;
        const float scale = 2.0f - tw * th;
        const float tx = ((x1 + x2) / 2) * (float)g - (float)col, ty = ((y1 + y2) / 2) * (float)g - (float)row;
        const float dx = tx - sigmoidf_(t[0]), dy = ty - sigmoidf_(t[1]);
        const float xy = scale * (dx * dx + dy * dy);
        float lw = logf(tw / geo.anchors[s][a][0]), lh = logf(th / geo.anchors[s][a][1]);
        if (isinf(lw)) lw = 0.0f;   // tf.where(is_inf): a zero-width box; a NaN stays
        if (isinf(lh)) lh = 0.0f;
        const float dw = lw - t[2], dh = lh - t[3];
        const float wh = scale * (dw * dw + dh * dh);
        // sparse_categorical_crossentropy on probabilities: log of the clipped sigmoid, then softmax cross-entropy of those
        float m = -INFINITY;
        for (int k = lane; k < nc; k += 64) m = fmaxf(m, logf(clipped_sigmoid(t[5 + k])));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
        float sum = 0.0f;
        for (int k = lane; k < nc; k += 64) sum += expf(logf(clipped_sigmoid(t[5 + k])) - m);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);   // a + b == b + a: every lane holds the same bits
        const float lc = logf(clipped_sigmoid(t[5 + gc[r]]));
        const float cls = logf(sum) - (lc - m);
        if (lane == 0) {
            s_term[r * 3 + 0] = xy;
            s_term[r * 3 + 1] = wh;
            s_term[r * 3 + 2] = cls;
        }
    }
    __syncthreads();

    // the sweep: channel 4 of every row; kSweepBatch loads in flight per thread
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n0 = tid; n0 < rows; n0 += kLossThreads * kSweepBatch) {
        float t4[kSweepBatch];
#pragma unroll
        for (int j = 0; j < kSweepBatch; ++j) {
            const int n = n0 + j * kLossThreads;
            t4[j] = n < rows ? grid[(size_t)n * F + 4] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < kSweepBatch; ++j) {
            const int n = n0 + j * kLossThreads;
            if (n >= rows) break;
            const float p = clipped_sigmoid(t4[j]);
            const bool assigned = (s_bits[n >> 5] >> (n & 31)) & 1u;
            acc[2] += (double)(assigned ? -logf(p + kEps) : -logf((1.0f - p) + kEps));
            if (assigned) {
                int r = 0;
                while (r < G - 1 && s_cell[r] != n) ++r;   // the marked row's ground-truth row
                acc[0] += (double)s_term[r * 3 + 0];
                acc[1] += (double)s_term[r * 3 + 1];
                acc[3] += (double)s_term[r * 3 + 2];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[i] += __shfl_down(acc[i], d);
        if (lane == 0) s_red[wave * 4 + i] = acc[i];
    }
    __syncthreads();
    if (tid < 4) {
        double v = 0.0;
        for (int w = 0; w < kLossWaves; ++w) v += s_red[w * 4 + tid];
        out[tid] = v;
    }
}

size_t loss_lds_bytes(int max_gt, int g)
{
    return (size_t)kLossWaves * 4 * sizeof(double) + (size_t)max_gt * 16 + (size_t)((3 * g * g + 31) / 32) * 4;
}

hipError_t launch_assign_targets(const float *gt_boxes, const int32_t *gt_classes, const int32_t *gt_count, int B, int G, int nc,
                                 const LossGeom &geo, int32_t *cells, hipStream_t s)
{
    hipLaunchKernelGGL(assign_targets_kernel, dim3((unsigned)B), dim3(kAssignThreads), (size_t)G * 4, s, gt_boxes, gt_classes, gt_count,
                       G, nc, geo, cells);
    return hipGetLastError();
}

hipError_t launch_yolo_loss(const LossGrids &grids, const LossGeom &geo, int B, int nc, const float *gt_boxes,
                            const int32_t *gt_classes, const int32_t *cells, int G, double *loss, hipStream_t s)
{
    // one LDS size for the three scales of a launch: the largest grid's bitmap (41 KB at max_gt = 1024 and g = 256, the limits)
    const size_t lds = loss_lds_bytes(G, std::max(geo.g[0], std::max(geo.g[1], geo.g[2])));
    hipLaunchKernelGGL(yolo_loss_kernel, dim3((unsigned)B * 3u), dim3(kLossThreads), lds, s, grids, geo, nc, gt_boxes, gt_classes, cells,
                       G, loss);
    return hipGetLastError();
}

}  // namespace y3
