// The workgroup shape of the stand-alone decode-shaped kernels (decode.hip: decode_kernel; candidates.hip: candidates_kernel), once:
// 256 lanes copy 64 boxes (contiguous 64 * (5 + nc) floats of one scale) into LDS with 16-B coalesced loads, then four lanes share one
// box.  decode_box.h holds the arithmetic of a box; this header holds what surrounds it -- which boxes a workgroup owns, their copy, and
// where box j of the workgroup lies in its image -- and the launch geometry that goes with it.
#pragma once
#include "y3_device.h"
#include "y3_kernels.h"
#include "decode_box.h"

namespace y3 {

constexpr int DEC_BOXES = 64;    // boxes per workgroup
constexpr int DEC_LANES = 4;     // lanes per box
constexpr int DEC_THREADS = DEC_BOXES * DEC_LANES;

struct DecodeLaunch {
    DecodeArgs a;
    int blk_start[4];  // first workgroup of each scale (prefix sums), [3] = total
};

// L.a -> L.blk_start; returns the grid size
inline int decode_blocks(DecodeLaunch &L)
{
    int acc = 0;
    for (int i = 0; i < 3; ++i) {
        L.blk_start[i] = acc;
        const long long total = (long long)L.a.B * L.a.gh[i] * L.a.gw[i] * 3;
        acc += (int)((total + DEC_BOXES - 1) / DEC_BOXES);
    }
    L.blk_start[3] = acc;
    return acc;
}

// What a lane knows after the prologue: the workgroup's boxes [box0, box0 + nbox) of scale s, and its own box j (lane q of its four).
// A lane behind the last box (live == false) computes on box 0 of the workgroup and stores nothing.
struct DecodeTile {
    int s, gh, gw, per_img;       // scale, its grid, its boxes per image
    long long box0;               // first box of the workgroup among the scale's boxes over the batch
    int nbox;
    int j, q;                     // box within the workgroup, lane within the box
    bool live;
    int b, r, a, row, col;        // image, row of the box inside the scale's part of the image, anchor, cell
    long long out_row;            // b * N + off[s] + r
    float *t;                     // the box's 5 + nc logits in LDS
};

// Copies the workgroup's logits into lds (barrier included) and fills the tile.  Every lane of the workgroup must call it.
__device__ __forceinline__ DecodeTile decode_tile_load(const DecodeLaunch &L, float *lds)
{
    DecodeTile T;
    const int F = 5 + L.a.nc;
    int s = 0;
    if ((int)blockIdx.x >= L.blk_start[1]) s = 1;
    if ((int)blockIdx.x >= L.blk_start[2]) s = 2;
    T.s = s;
    T.gh = L.a.gh[s], T.gw = L.a.gw[s];
    T.per_img = T.gh * T.gw * 3;
    const long long total = (long long)L.a.B * T.per_img;            // boxes of this scale over the batch
    T.box0 = (long long)((int)blockIdx.x - L.blk_start[s]) * DEC_BOXES;
    T.nbox = (int)((total - T.box0) < DEC_BOXES ? (total - T.box0) : DEC_BOXES);
    const float *src = L.a.grid[s] + T.box0 * F;
    const int nfl = T.nbox * F;
    const int tid = threadIdx.x;
    // coalesced copy (16 B per lane; box0 * F * 4 is a multiple of 16 because DEC_BOXES * 4 is)
    const int nvec = nfl >> 2;
    for (int i = tid; i < nvec; i += DEC_THREADS) reinterpret_cast<f32x4 *>(lds)[i] = reinterpret_cast<const f32x4 *>(src)[i];
    for (int i = (nvec << 2) + tid; i < nfl; i += DEC_THREADS) lds[i] = src[i];
    __syncthreads();

    T.j = tid >> 2, T.q = tid & 3;
    T.live = T.j < T.nbox;
    const int jj = T.live ? T.j : 0;
    const long long gi = T.box0 + jj;
    T.b = (int)(gi / T.per_img);
    T.r = (int)(gi - (long long)T.b * T.per_img);
    T.a = T.r % 3;
    const int cell = T.r / 3;
    T.row = cell / T.gw, T.col = cell - T.row * T.gw;
    T.out_row = (long long)T.b * L.a.N + L.a.off[s] + T.r;
    T.t = lds + jj * F;
    return T;
}

}  // namespace y3
