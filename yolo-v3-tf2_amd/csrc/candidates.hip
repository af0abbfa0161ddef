// Multi-label candidates on gfx950 (include/y3.h, y3_yolo_decode_candidates_hw; no reference counterpart): every pair (box n, class c)
// with conf[n] * prob[n,c] > S is a candidate of its own, numbered in the order (n ascending, c ascending) and stored in the first
// `capacity` slots of its image.  The order comes from counts and prefix sums alone -- no atomic decides a slot:
//   1. candidates_kernel<false>: the decode's workgroups (256 lanes, 64 boxes' logits in LDS, four lanes per box through
//      decode_box_lanes, the body decode.hip and the fused heads share) leave the number of candidates of every box in ws [B,N] i32;
//   2. cand_scan_kernel: one workgroup per image turns its N counts into exclusive prefixes in place, writes total[b] and the filler
//      rows k >= min(total, capacity);
//   3. candidates_kernel<true>: the same decode again; every wave then walks the (box, class) pairs of its own 16 boxes in order, 64 pairs
//      per step, and places the survivors by ballot / popcount: slot = prefix of the box + rank of the pair inside the box.  Consecutive
//      lanes hold consecutive pairs, so where survivors are dense consecutive lanes store consecutive rows.
// Arithmetic: score = conf * prob, one fp32 multiply of the two values decode_kernel<WRITE_PROBS> stores (-ffp-contract=off).
#include "decode_tile.h"

namespace y3 {

static constexpr int CAND_WAVE_BOXES = DEC_BOXES / 4;   // boxes whose pairs one wave walks

struct CandLaunch {
    DecodeLaunch d;
    float S;
    int K;
};

// WRITE = false: counts[b * N + n] = candidates of box n.  WRITE = true: counts holds the exclusive prefixes of cand_scan_kernel.
template <bool WRITE>
__global__ __launch_bounds__(DEC_THREADS) void candidates_kernel(const CandLaunch L, int32_t *__restrict__ counts,
                                                                 float *__restrict__ cand_boxes, int64_t *__restrict__ cand_cls,
                                                                 float *__restrict__ cand_scores, int32_t *__restrict__ cand_src)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_cnt[DEC_BOXES];      // candidates of box j
    __shared__ int s_first[DEC_BOXES];    // candidates of the workgroup's boxes before j
    __shared__ int s_base[DEC_BOXES];     // candidates of the image's boxes before j (the scan's prefix)
    __shared__ int s_img[DEC_BOXES];      // image of box j
    __shared__ int s_n[DEC_BOXES];        // its row in the image
    const DecodeArgs &A = L.d.a;
    const int nc = A.nc, F = 5 + nc;
    const DecodeTile T = decode_tile_load(L.d, lds);
    const int tid = threadIdx.x, j = T.j, q = T.q, lane = tid & 63, nbox = T.nbox;
    const bool live = T.live;
    float *t = T.t;
    f32x4 bb;
    float c, best;
    int besti;
    // the lane's class probabilities replace their logits in LDS; bb / c are valid in lane q == 0
    decode_box_lanes<true, false>(t, q, lane, nc, T.gh, T.gw, T.row, T.col, q >= 2 ? A.anchors[T.s][T.a][q - 2] : 0.0f, live, bb, c, best, besti);
    const float cf = __shfl(c, lane & ~3);
    int mine = 0;
    if (live)
        for (int k = q; k < nc; k += 4) mine += (cf * t[5 + k] > L.S) ? 1 : 0;    // NaN: not a candidate
    mine += __shfl_xor(mine, 1);
    mine += __shfl_xor(mine, 2);
    const long long out_row = T.out_row;
    if (!WRITE) {
        if (q == 0 && live) counts[out_row] = mine;
        return;
    }
    if (q == 0) {
        if (live) {   // the box and its confidence over the logits the four lanes have consumed
            t[0] = bb[0], t[1] = bb[1], t[2] = bb[2], t[3] = bb[3];
            t[4] = c;
            s_base[j] = counts[out_row];
        }
        s_cnt[j] = mine;                 // 0 for a box behind the end
        s_img[j] = T.b;
        s_n[j] = A.off[T.s] + T.r;
    }
    __syncthreads();
    if (tid < DEC_BOXES) {               // wave 0: exclusive prefix over the 64 boxes
        const int v = s_cnt[tid];
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (tid >= d) incl += o;
        }
        s_first[tid] = incl - v;
    }
    __syncthreads();
    // wave w walks the pairs of boxes [16 w, 16 w + 16) in (box, class) order, 64 pairs per step
    const int w = tid >> 6, jb0 = w * CAND_WAVE_BOXES;
    const int nb = nbox - jb0 < 0 ? 0 : (nbox - jb0 < CAND_WAVE_BOXES ? nbox - jb0 : CAND_WAVE_BOXES);
    const int P = nb * nc;
    // a wave none of whose boxes has a candidate has nothing to place (wave-uniform; no barrier follows): with a trained network's few
    // hundred survivors among the N x nc pairs that is nearly every wave
    if (nb == 0 || s_first[jb0 + nb - 1] + s_cnt[jb0 + nb - 1] == s_first[jb0]) return;
    int running = s_first[jb0];          // candidates of the workgroup before this step's first pair
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int p = p0 + lane;
        const bool valid = p < P;
        const int pj = valid ? p / nc : 0;
        const int k = valid ? p - pj * nc : 0;
        const int jb = jb0 + pj;
        const float *tt = lds + jb * F;
        const float sc = tt[4] * tt[5 + k];
        const bool cand = valid && sc > L.S;
        const unsigned long long mask = __ballot(cand);
        const int rank = running + __popcll(mask & ((1ull << lane) - 1ull));
        running += __popcll(mask);
        if (cand) {
            const int slot = s_base[jb] + (rank - s_first[jb]);     // position among the image's candidates
            if (slot < L.K) {
                const size_t g = (size_t)s_img[jb] * L.K + slot;
                f32x4 bx;
                bx[0] = tt[0], bx[1] = tt[1], bx[2] = tt[2], bx[3] = tt[3];
                *reinterpret_cast<f32x4 *>(cand_boxes + g * 4) = bx;
                cand_cls[g] = (int64_t)k;
                cand_scores[g] = sc;
                cand_src[g] = s_n[jb];
            }
        }
    }
}

// One workgroup per image: counts [N] -> exclusive prefixes in place, total[b], and the filler rows k >= min(total, K)
// (box (0,0,0,0), score 0, class 0, source 0: what merge_tiles_kernel writes; the padded NMS never selects such a row).
__global__ __launch_bounds__(256) void cand_scan_kernel(int32_t *__restrict__ counts, int N, int K, int32_t *__restrict__ totals,
                                                        float *__restrict__ cand_boxes, int64_t *__restrict__ cand_cls,
                                                        float *__restrict__ cand_scores, int32_t *__restrict__ cand_src)
{
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int32_t *c = counts + (size_t)b * N;
    int carry = 0;
    for (int base = 0; base < N; base += 1024) {     // four consecutive boxes per lane
        const int i0 = base + tid * 4;
        int v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i0 + u < N ? c[i0 + u] : 0;
        const int sum = v[0] + v[1] + v[2] + v[3];
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u < w) before += wsum[u];
            all += wsum[u];
        }
        int ex = carry + before + incl - sum;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < N) {
                c[i0 + u] = ex;
                ex += v[u];
            }
        carry += all;
        __syncthreads();
    }
    if (tid == 0) totals[b] = carry;
    for (int k = (carry < K ? carry : K) + tid; k < K; k += 256) {
        const size_t g = (size_t)b * K + k;
        f32x4 z;
        z[0] = z[1] = z[2] = z[3] = 0.0f;
        *reinterpret_cast<f32x4 *>(cand_boxes + g * 4) = z;
        cand_cls[g] = 0;
        cand_scores[g] = 0.0f;
        cand_src[g] = 0;
    }
}

hipError_t launch_candidates(const DecodeArgs &a, float S, int K, float *cand_boxes, int64_t *cand_cls, float *cand_scores,
                             int32_t *cand_src, int32_t *totals, int32_t *counts, hipStream_t s)
{
    CandLaunch L;
    L.d.a = a;
    L.S = S;
    L.K = K;
    const int blocks = decode_blocks(L.d);
    const size_t lds = decode_lds_bytes(a.nc);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static LdsAttrOnce attr_count, attr_write;
    if (hipError_t e = set_max_lds_once(attr_count, reinterpret_cast<const void *>(candidates_kernel<false>), (int)lds); e != hipSuccess) return e;
    if (hipError_t e = set_max_lds_once(attr_write, reinterpret_cast<const void *>(candidates_kernel<true>), (int)lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(candidates_kernel<false>, dim3(blocks), dim3(DEC_THREADS), lds, s, L, counts, cand_boxes, cand_cls, cand_scores, cand_src);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cand_scan_kernel, dim3(a.B), dim3(256), 0, s, counts, a.N, K, totals, cand_boxes, cand_cls, cand_scores, cand_src);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(candidates_kernel<true>, dim3(blocks), dim3(DEC_THREADS), lds, s, L, counts, cand_boxes, cand_cls, cand_scores, cand_src);
    return hipGetLastError();
}

// The stand-alone form for callers that hold the decoded [B,N,nc] probabilities (include/y3.h, y3_class_candidates), as class_scores_kernel
// is to decode_kernel: one lane per box, the same count / prefix / write passes and the same multiply and compare.
__global__ __launch_bounds__(256) void class_candidates_count_kernel(const float *__restrict__ conf, const float *__restrict__ probs,
                                                                     size_t n, int nc, float S, int32_t *__restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *p = probs + i * nc;
    const float c = conf[i];
    int mine = 0;
    for (int k = 0; k < nc; ++k) mine += (c * p[k] > S) ? 1 : 0;
    counts[i] = mine;
}

__global__ __launch_bounds__(256) void class_candidates_write_kernel(const float *__restrict__ bboxes, const float *__restrict__ conf,
                                                                     const float *__restrict__ probs, size_t n, int N, int nc, float S, int K,
                                                                     const int32_t *__restrict__ base, float *__restrict__ cand_boxes,
                                                                     int64_t *__restrict__ cand_cls, float *__restrict__ cand_scores,
                                                                     int32_t *__restrict__ cand_src)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t b = i / N;
    const float *p = probs + i * nc;
    const float c = conf[i];
    int slot = base[i];
    for (int k = 0; k < nc && slot < K; ++k) {
        const float sc = c * p[k];
        if (!(sc > S)) continue;
        const size_t g = b * K + slot++;
        *reinterpret_cast<f32x4 *>(cand_boxes + g * 4) = *reinterpret_cast<const f32x4 *>(bboxes + i * 4);
        cand_cls[g] = (int64_t)k;
        cand_scores[g] = sc;
        cand_src[g] = (int32_t)(i - b * N);
    }
}

hipError_t launch_class_candidates(const float *bboxes, const float *conf, const float *probs, int B, int N, int nc, float S, int K,
                                   float *cand_boxes, int64_t *cand_cls, float *cand_scores, int32_t *cand_src, int32_t *totals,
                                   int32_t *counts, hipStream_t s)
{
    const size_t n = (size_t)B * N;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(class_candidates_count_kernel, grid, block, 0, s, conf, probs, n, nc, S, counts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cand_scan_kernel, dim3(B), dim3(256), 0, s, counts, N, K, totals, cand_boxes, cand_cls, cand_scores, cand_src);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(class_candidates_write_kernel, grid, block, 0, s, bboxes, conf, probs, n, N, nc, S, K, counts, cand_boxes, cand_cls,
                       cand_scores, cand_src);
    return hipGetLastError();
}

// The index word (word 6) of every valid packed row: candidate k -> the box it came from, cand_src[b, k].
__global__ __launch_bounds__(256) void candidate_sources_kernel(unsigned *__restrict__ packed, const int32_t *__restrict__ nv,
                                                                const int32_t *__restrict__ cand_src, int B, int K, int M)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * M) return;
    const int b = i / M, r = i - b * M;
    if (r >= nv[b]) return;
    unsigned *o = packed + (size_t)i * 7 + 6;
    const unsigned k = *o;
    if (k < (unsigned)K) *o = (unsigned)cand_src[(size_t)b * K + k];
}

hipError_t launch_candidate_sources(void *packed, const int32_t *nv, const int32_t *cand_src, int B, int K, int M, hipStream_t s)
{
    hipLaunchKernelGGL(candidate_sources_kernel, dim3((B * M + 255) / 256), dim3(256), 0, s, static_cast<unsigned *>(packed), nv, cand_src, B, K, M);
    return hipGetLastError();
}

}  // namespace y3
