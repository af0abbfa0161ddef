// yolo_decode (+ the class arg-max / score of yolo_nms) on gfx950.
//
// Replaces reference core/yolo_decode_layer.py:4-36 (split, sigmoid x3, exp*anchor, meshgrid add,
// divide, +-wh/2, concat, reshape, concat) and core/yolo_nms.py:18-24 (argmax, reduce_max, multiply).
// HBM-bound: 4*(5+nc) bytes read per box.  A workgroup of 256 lanes copies 64 boxes (contiguous 64*(5+nc)
// floats of one scale) into LDS with 16-B coalesced loads; four lanes then share one box: lane q takes field q of
// (x, y, w, h) and the classes q, q+4, q+8, ... (a quarter of the sigmoids each), and the four partial
// (first-maximum, index) pairs are merged with two lane exchanges.  22 KB of LDS per workgroup keeps 7 workgroups =
// 28 waves per CU in flight, so the copy of one workgroup overlaps the sigmoids of the others.  Class probabilities are
// written back through LDS so that the [B,N,nc] store is coalesced.
// Arithmetic: sigmoid(x) = 1/(1+exp(-x)), true divisions, fp32, no contraction (-ffp-contract=off).
#include "decode_tile.h"

namespace y3 {

template <bool WRITE_PROBS, bool WRITE_SCORES>
__global__ __launch_bounds__(DEC_THREADS) void decode_kernel(const DecodeLaunch L, float *__restrict__ bboxes,
                                                             float *__restrict__ conf, float *__restrict__ probs,
                                                             int64_t *__restrict__ cls, float *__restrict__ scores)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const DecodeTile T = decode_tile_load(L, lds);
    const int tid = threadIdx.x, q = T.q;
    // lane 0: x, lane 1: y, lane 2: w, lane 3: h; classes q, q + 4, ... (decode_box.h: the body the fused head convs share)
    f32x4 bb;
    float c, best;
    int besti;
    decode_box_lanes<WRITE_PROBS, WRITE_SCORES>(T.t, q, tid & 63, L.a.nc, T.gh, T.gw, T.row, T.col, q >= 2 ? L.a.anchors[T.s][T.a][q - 2] : 0.0f, T.live, bb, c, best, besti);
    if (q == 0 && T.live) {
        *reinterpret_cast<f32x4 *>(bboxes + T.out_row * 4) = bb;
        if (conf) conf[T.out_row] = c;
        if (WRITE_SCORES) {
            cls[T.out_row] = (int64_t)besti;
            scores[T.out_row] = c * best;
        }
    }
    if (WRITE_PROBS) {
        __syncthreads();
        // the block's boxes may straddle images; rows of one image are contiguous in probs, so resolve per box
        const int nc = L.a.nc, F = 5 + nc;
        const int nout = T.nbox * nc;
        for (int i = tid; i < nout; i += DEC_THREADS) {
            const int jb = i / nc, k = i - jb * nc;
            const long long gj = T.box0 + jb;
            const int bj = (int)(gj / T.per_img);
            const int rj = (int)(gj - (long long)bj * T.per_img);
            const long long orow = (long long)bj * L.a.N + L.a.off[T.s] + rj;
            probs[orow * nc + k] = lds[jb * F + 5 + k];
        }
    }
}

size_t decode_lds_bytes(int nc) { return (size_t)DEC_BOXES * (5 + nc) * sizeof(float); }

template <bool WRITE_PROBS, bool WRITE_SCORES>
static hipError_t launch_decode_as(const DecodeLaunch &L, int blocks, size_t lds, float *bboxes, float *conf, float *probs, int64_t *cls,
                                   float *scores, hipStream_t s)
{
    static LdsAttrOnce attr;  // per instantiation
    const auto k = decode_kernel<WRITE_PROBS, WRITE_SCORES>;
    if (hipError_t e = set_max_lds_once(attr, reinterpret_cast<const void *>(k), (int)lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(DEC_THREADS), lds, s, L, bboxes, conf, probs, cls, scores);
    return hipGetLastError();
}

hipError_t launch_decode(const DecodeArgs &a, float *bboxes, float *conf, float *probs, int64_t *cls, float *scores,
                         hipStream_t s)
{
    DecodeLaunch L;
    L.a = a;
    const int blocks = decode_blocks(L);
    const size_t lds = decode_lds_bytes(a.nc);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const bool wp = probs != nullptr, wsc = scores != nullptr;
    if (wp && wsc) return launch_decode_as<true, true>(L, blocks, lds, bboxes, conf, probs, cls, scores, s);
    if (wp) return launch_decode_as<true, false>(L, blocks, lds, bboxes, conf, probs, cls, scores, s);
    if (wsc) return launch_decode_as<false, true>(L, blocks, lds, bboxes, conf, probs, cls, scores, s);
    return launch_decode_as<false, false>(L, blocks, lds, bboxes, conf, probs, cls, scores, s);
}

// class_indices = argmax(probs, -1) (int64, first max), scores = conf * reduce_max(probs, -1)
// reference: core/yolo_nms.py:18-24.  Stand-alone form for callers that hold [B,N,nc] probabilities.
__global__ __launch_bounds__(256) void class_scores_kernel(const float *__restrict__ conf,
                                                           const float *__restrict__ probs, size_t n, int nc,
                                                           int64_t *__restrict__ cls, float *__restrict__ scores)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *p = probs + i * nc;
    float best = p[0];
    int besti = 0;
    for (int k = 1; k < nc; ++k) {
        const float v = p[k];
        if (v > best) {
            best = v;
            besti = k;
        }
    }
    cls[i] = besti;
    scores[i] = conf[i] * best;
}

hipError_t launch_class_scores(const float *conf, const float *probs, size_t n, int nc, int64_t *cls, float *scores,
                               hipStream_t s)
{
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(class_scores_kernel, grid, block, 0, s, conf, probs, n, nc, cls, scores);
    return hipGetLastError();
}

}  // namespace y3
