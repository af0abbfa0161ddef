// Sliced inference, the merge (include/y3.h, y3_merge_tile_detections; no reference counterpart): the packed rows y3_net_detect leaves on a
// batch of tile images -> the candidate arrays of a second NMS over each frame.  Tile image gi = f * tiles + t owns the candidates
// [gi * M, (gi + 1) * M) of the flat arrays, which is candidate n = t * M + r of frame f: the kernel needs neither f nor t.
// The suppression itself is nms_kernel's and the packing pack_kernel's (nms.hip), launched behind this kernel by the host: there is no second
// suppression loop.  HBM-bound and tiny: one thread per packed row, seven words in, seven out.
// Box mapping, per axis, four separately rounded fp32 operations at most (the library is built with -ffp-contract=off):
//   canvas -> window   u  = (x * Wc - left) / sw     unletterbox_kernel's expression; copied where the window fills the canvas on this axis
//   window -> frame    x' = (x0 + u * cw) / w        copied where the window spans the frame on this axis
// Host restatement: tiles.merge_tile_detections_ref.
#include "y3_kernels.h"

namespace y3 {

__device__ __forceinline__ float tile_axis(float x, int canvas, int lb_len, int lb_off, int win_off, int win_len, int frame_len)
{
    float u = x;
    if (!(lb_len == canvas && lb_off == 0)) u = (x * (float)canvas - (float)lb_off) / (float)lb_len;
    if (win_off == 0 && win_len == frame_len) return u;
    return ((float)win_off + u * (float)win_len) / (float)frame_len;
}

__global__ __launch_bounds__(256) void merge_tiles_kernel(const unsigned *__restrict__ packed, const int32_t *__restrict__ nv, MergeTable table,
                                                          int M, int Hc, int Wc, float *__restrict__ boxes, float *__restrict__ scores,
                                                          int64_t *__restrict__ cls)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const MergeTile e = table.t[blockIdx.y];              // uniform per workgroup: scalar loads from the kernel arguments
    const size_t n = (size_t)blockIdx.y * M + r;
    const int valid = min(max(nv[blockIdx.y], 0), M);     // a count outside [0, M] cannot send a read past the tile's rows
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float score = 0.0f;
    int64_t c = 0;
    if (r < valid) {
        const unsigned *o = packed + n * 7;
        b.x = tile_axis(__uint_as_float(o[0]), Wc, e.g.sw, e.g.left, e.x0, e.cw, e.w);
        b.y = tile_axis(__uint_as_float(o[1]), Hc, e.g.sh, e.g.top, e.y0, e.ch, e.h);
        b.z = tile_axis(__uint_as_float(o[2]), Wc, e.g.sw, e.g.left, e.x0, e.cw, e.w);
        b.w = tile_axis(__uint_as_float(o[3]), Hc, e.g.sh, e.g.top, e.y0, e.ch, e.h);
        score = __uint_as_float(o[4]);
        c = (int64_t)(int)o[5];
    }
    *reinterpret_cast<float4 *>(boxes + n * 4) = b;
    scores[n] = score;
    cls[n] = c;
}

hipError_t launch_merge_tiles(const void *packed, const int32_t *nv, const MergeTile *entries, int n, int M, int Hc, int Wc, float *boxes,
                              float *scores, int64_t *cls, hipStream_t s)
{
    MergeTable table{};
    for (int i = 0; i < n; ++i) table.t[i] = entries[i];
    dim3 grid((unsigned)((M + 255) / 256), (unsigned)n), block(256);
    hipLaunchKernelGGL(merge_tiles_kernel, grid, block, 0, s, static_cast<const unsigned *>(packed), nv, table, M, Hc, Wc, boxes, scores, cls);
    return hipGetLastError();
}

}  // namespace y3
