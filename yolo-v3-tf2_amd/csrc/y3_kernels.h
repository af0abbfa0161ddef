// Internal launch interface between the C-ABI layer (y3_net.cpp, y3_plan.cpp, y3_forward.cpp, y3_ops.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/y3.h"
#include "decode_box.h"

namespace y3 {

// One fused conv launch: Conv2D [+BN] [+LeakyReLU(0.1)] [+shortcut add], optional
// (nearest-x2-upsampled src0) (+) src1 channel concat in the A-operand gather.
struct ConvArgs {
    const void *src0;      // [B,H0,W0,C0]  (H0 = H/2 when up0)
    const void *src1;      // [B,H,W,Cin-C0] or nullptr
    const void *wpk;       // packed weights [CoutPad][K], K = taps*Cin, k = tap*Cin + c
    const float *scale;    // [CoutPad] BN scale (1 for bias convs)
    const float *shift;    // [CoutPad] BN shift / bias
    const void *residual;  // [B,Ho,Wo,Cout] or nullptr
    void *dst;             // [B,Ho,Wo,Cout]
    int B, H, W;           // logical input spatial size
    int Ho, Wo;
    int Cin, C0;
    int Cout, CoutPad;
    int ksize, stride, pad;
    int up0;
    int leaky;
    int M;                 // B*Ho*Wo
    int K;                 // ksize*ksize*Cin
    unsigned src0_bytes, src1_bytes, w_bytes, dst_bytes;
    // fp32 tile order: 0 = every XCD takes a contiguous run of tiles (N fastest); gn in {1,2,4,8} = the XCDs form
    // an (8/gn) x gn grid over the (M-tile, N-tile) matrix (see conv_f32.hip)
    int xcd_gn;
    // head convs only (conv_head.hip, the fp32-output epilogue of conv_bf16.hip): dec.boxes != nullptr -> the launch decodes
    // its own output tile (y3_net_forward_decode); dst may then be nullptr (the raw grid is not wanted)
    DecodeHead dec;
    int k_chunk;           // fp32 MFMA kernel, 3x3 convs: > 0 walks K chunk-major, k_chunk input channels at a time (conv_f32.hip); 0: tap-major
    // measurement only (y3_net_measure_sclk): when non-null, thread 0 of the middle workgroup stores {s_memtime, s_memrealtime}
    // at its entry and after its epilogue -> the shader clock held while that workgroup ran.  Null in every product launch.
    unsigned long long *clk_stamps;   // [4]
    int n_cus;             // compute units of the net's device, read once by y3_net_plan: sizes the grids of the persistent kernels (conv_res_*.hip)
    int device;            // the net's device index (the launch goes there: Y3_ENTER_DEVICE); -1 = not known, launchers ask the runtime
    // int8 convs only (conv_i8.hip; `scale` is then (s_in * s_w[c]) * bn_scale[c]): the scale of the int8 shortcut tensor, and 1 / the scale
    // of the int8 output tensor.  Behind everything the other launches read: their kernel arguments keep their offsets.
    float q_res, q_inv;
    // fp32 MFMA kernel, 3x3 single-source convs with B % 32 == 0 (border skip): the conv geometry's position table on the
    // device (border_order below; kPosTabPad zero entries behind the Ho * Wo positions) -> GEMM rows are batch-minor, m = j * B + b with
    // j an index into the table, and a tile's K walk leaves out the taps that are padding for all of its positions.  Null: raster rows,
    // every tap.  After q_res / q_inv for the same reason as they are where they are.
    const uint32_t *pos_tab;
    // ... with pos_tab: the leading M-tiles that hold a border position (the table's sort puts them first), for the balanced tile -> XCD
    // mapping (balanced_mtile below); -1: the mapping of the raster launches.  Behind pos_tab as pos_tab is behind q_res / q_inv.
    int border_tiles;
};

// Balanced tile -> XCD mapping of the batch-minor launches (conv_f32.hip; DESIGN.md section 4, "Border skip").  The T M-tiles of a launch are
// the Tb border tiles, whose K walks are short, and the T - Tb interior ones; a launch ends when its slowest XCD does, so each of the gm XCD
// M-ranges takes an equal share of both kinds: range xm owns border tiles [xm Tb / gm, (xm + 1) Tb / gm) and interior tiles
// [Tb + xm Ti / gm, Tb + (xm + 1) Ti / gm).  balanced_range: how many tiles that is.  balanced_mtile: the M-tile of local index lm of the
// range -- the interior tiles first, so the short ones end the range's work -- or -1 behind its end (a padding workgroup).
// -DY3_BORDER_FIRST (tools/ab_libs.py variant): the other order.
__host__ __device__ inline int balanced_range(int xm, int gm, int Tb, int T)
{
    return ((xm + 1) * Tb / gm - xm * Tb / gm) + ((xm + 1) * (T - Tb) / gm - xm * (T - Tb) / gm);
}
__host__ __device__ inline int balanced_mtile(int lm, int xm, int gm, int Tb, int T)
{
    const int blo = xm * Tb / gm, nb = (xm + 1) * Tb / gm - blo;
    const int ilo = Tb + xm * (T - Tb) / gm, ni = Tb + (xm + 1) * (T - Tb) / gm - ilo;
    if (lm >= nb + ni) return -1;
#ifdef Y3_BORDER_FIRST
    return lm < nb ? blo + lm : ilo + (lm - nb);
#else
    return lm < ni ? ilo + lm : blo + (lm - ni);
#endif
}
// Workgroups of such a launch: the 8 XCDs form a gm x gn grid (gn = 8 / gm divides tilesN), XCD bid & 7 = (xm, xn) takes local index bid >> 3
// of its block, N fastest; the grid is sized for the largest range.  balanced_tile: workgroup bid -> (M-tile, N-tile), mt = -1: padding.
struct TileMN { int mt, nt; };
__host__ __device__ inline TileMN balanced_tile(int bid, int gn, int tilesN, int Tb, int T)
{
    const int gm = 8 / gn, xcd = bid & 7, xm = xcd / gn, xn = xcd - xm * gn;
    const int nb = tilesN / gn, j = bid >> 3, lm = j / nb;
    return {balanced_mtile(lm, xm, gm, Tb, T), xn * nb + (j - lm * nb)};
}
inline int balanced_grid(int gn, int tilesN, int Tb, int T)
{
    const int gm = 8 / gn;
    int rows = 0;
    for (int xm = 0; xm < gm; ++xm) rows = rows > balanced_range(xm, gm, Tb, T) ? rows : balanced_range(xm, gm, Tb, T);
    return 8 * rows * (tilesN / gn);
}

// One position of a 3x3 conv's output grid: (ho, wo) and mask9, bit t = tap t = (u, v) = (t / 3, t % 3) reads inside the image.
constexpr int kPosMaxGrid = 2047;   // ho, wo in 11 bits each
constexpr int kPosTabPad = 8;       // zero entries behind the table: the blocks of a tile's rows >= M (at most 256 / 32) read them
constexpr uint32_t pos_pack(int ho, int wo, uint32_t mask9) { return ((uint32_t)ho << 20) | ((uint32_t)wo << 9) | mask9; }
constexpr int pos_ho(uint32_t e) { return (int)(e >> 20); }
constexpr int pos_wo(uint32_t e) { return (int)((e >> 9) & 0x7ffu); }
constexpr uint32_t pos_mask(uint32_t e) { return e & 0x1ffu; }
// The table of one geometry: all Ho * Wo positions, stably sorted by (live taps, mask9) (positions of one mask keep raster order).  Host only (y3_plan.cpp).
void border_order(int Ho, int Wo, int H, int W, int stride, int pad, uint32_t *out);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device): the attribute belongs to the
// device's copy of the code object, so a process driving several GPUs must set it on each.
struct LdsAttrOnce { unsigned long long done = 0; };   // bit d: set on device d (d < 64)
// `dev`: the device the launch goes to, when the caller knows it (ConvArgs::device, set from the net at plan time) -- then a launch
// makes no runtime call here at all once the attribute is set; -1: ask the runtime (stand-alone launches outside a net).
inline hipError_t set_max_lds_once(LdsAttrOnce &st, const void *fn, int bytes, int dev = -1)
{
    hipError_t e = hipSuccess;
    if (dev < 0 && (e = hipGetDevice(&dev)) != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && ((st.done >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) st.done |= 1ull << dev;
    return e;
}

// Grids of the persistent kernels (a fixed number of workgroups walks the tiles, tile += gridDim.x): the one definition their launchers
// call and y3_persistent_grid (include/y3.h, Y3_PERSISTENT_*) answers from.  cus > 0.
// A fused stem: wg_per_cu workgroups per CU, never more than there are tiles.
constexpr int kTinyStemWgPerCu = 4;   // conv_tiny_stem.hip, all three formats
constexpr int kStemWgPerCuF32 = 1;    // conv_stem.hip, conv_stem_f32
constexpr int kStemWgPerCu16 = 2;     // conv_stem.hip, conv_stem16<bf16 / f16>
inline int persistent_stem_grid(long long n_tiles, int wg_per_cu, int cus)
{
    return n_tiles < (long long)wg_per_cu * cus ? (int)n_tiles : wg_per_cu * cus;
}
// A weight-resident conv (conv_res_f32.hip, conv_res_16bit.h): one workgroup per CU, the CUs shared out evenly among the output-channel
// slices; workgroup w keeps slice w % slices and walks the spatial tiles w / slices, + grid / slices, ...  -> workgroups per slice.
inline int persistent_res_per_slice(long long n_spatial, int slices, int cus)
{
    int per_slice = cus / slices;
    if (per_slice < 1) per_slice = 1;
    if (per_slice > n_spatial) per_slice = (int)n_spatial;
    return per_slice;
}

// The tail every MFMA conv launcher shares: the dynamic-LDS attribute once per (instantiation, device), the launch, its status.
template <auto KERNEL>
static hipError_t launch_conv_kernel(const ConvArgs &a, int grid, int threads, size_t lds, hipStream_t s, int grid_y = 1)
{
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static LdsAttrOnce attr;  // per instantiation
    if (hipError_t e = set_max_lds_once(attr, reinterpret_cast<const void *>(KERNEL), (int)lds, a.device); e != hipSuccess) return e;
    hipLaunchKernelGGL(KERNEL, dim3(grid, grid_y), dim3(threads), lds, s, a);
    return hipGetLastError();
}

// The four instantiations of a 16-bit tile: launch(concat, out_f32) gets the two flags as std::true_type / std::false_type values.
template <typename LAUNCH>
static hipError_t dispatch_concat_out(bool concat, bool out_f32, LAUNCH launch)
{
    using T = std::true_type; using F = std::false_type;
    return concat ? (out_f32 ? launch(T{}, T{}) : launch(T{}, F{})) : (out_f32 ? launch(F{}, T{}) : launch(F{}, F{}));
}

// One tile configuration of an MFMA conv kernel: block tile bm x bn, waves per workgroup, LDS stages, K tile.  Every conv file keeps one
// table of {TileInfo, launcher(s)} rows indexed by tile id; a retired id is an all-zero row with no launcher.
struct TileInfo { int bm, bn, waves, stages, bk; };
// Does the tile divide the conv?  c0: channels of the first source of a concat conv, -1 without a second source.
inline bool tile_fits(const TileInfo &t, int cin, int c0, int cout_pad)
{
    return t.bm > 0 && cin % t.bk == 0 && cout_pad % t.bn == 0 && (c0 < 0 || c0 % t.bk == 0);
}

// Split-K: one slice's slab of raw fp32 accumulators, [Mpad][CoutPad] with M padded to whole tiles
inline size_t split_slab_bytes(const TileInfo &t, long long M, int cout_pad) { return (size_t)((M + t.bm - 1) / t.bm) * t.bm * cout_pad * sizeof(float); }
// What the split launchers of conv_f32.hip and conv_16bit.h share before their kernel dispatch: S, the slab and the workspace checked,
// then the slice launch's arguments (raw accumulators into ws: no shortcut, no tile order, no stamps) and its grid.  slab = 0: refused.
struct SplitLaunch { ConvArgs c; size_t slab; int grid; };
inline SplitLaunch split_launch(const ConvArgs &a, const TileInfo &t, int S, void *ws, size_t ws_bytes)
{
    SplitLaunch l{a, 0, 0};
    const size_t slab = tile_fits(t, a.Cin, a.src1 ? a.C0 : -1, a.CoutPad) ? split_slab_bytes(t, a.M, a.CoutPad) : 0;
    if (!slab || S < 2 || S > a.K / t.bk || !ws || !a.dst || a.dec.boxes || slab > 0x7fffffffull || (size_t)S * slab > ws_bytes) return l;
    l.c.dst = ws;
    l.c.dst_bytes = (unsigned)slab;
    l.c.residual = nullptr;
    l.c.xcd_gn = 0;
    l.c.clk_stamps = nullptr;
    l.slab = slab;
    l.grid = ((a.M + t.bm - 1) / t.bm) * (a.CoutPad / t.bn);
    return l;
}

// fp32 MFMA kernel (table in conv_f32.hip; bk = 32)
static constexpr int TILE_COUNT = 34;  // 33: the weight-resident 3x3 kernel (conv_res_f32.hip); ids without a selecting plan are retired (conv_f32.hip)
TileInfo conv_tile_info(int tile);
bool conv_tile_built(int tile);        // false: retired id

hipError_t launch_conv_f32(const ConvArgs &a, int tile, hipStream_t s);
// split-K form of the same conv (conv_f32.hip): S >= 2 slices of the K walk as S times the workgroups, raw accumulators into
// ws [S][Mpad][CoutPad] fp32 (at least S * split_slab_bytes), then splitk_finish_f32 on the same stream: the slabs added in
// the order 0..S-1, the epilogue, the store to a.dst.  Tiles 10 and 11 only (conv_split_tile).
bool conv_split_tile(int tile);
hipError_t launch_conv_f32_split(const ConvArgs &a, int tile, int S, void *ws, size_t ws_bytes, hipStream_t s);
// weight-resident 3x3 / stride-1 / Cin = 32 conv (conv_res_f32.hip): tile id 33
bool conv_res_f32_fits(const ConvArgs &a);
hipError_t launch_conv_res_f32(const ConvArgs &a, hipStream_t s);
// 1x1 head conv (Cout = 3 * (5 + nc) <= 256) + bias with yolo_decode + arg-max / score fused in (conv_head.hip)
bool conv_head_decode_f32_fits(const ConvArgs &a);
hipError_t launch_conv_head_decode_f32(const ConvArgs &a, hipStream_t s);
// first layer: 3x3 stride-1 conv with Cin = 3 (direct, VALU; conv_first.hip): fp32 image in, output in the format of dtype (Y3_DTYPE_*)
hipError_t launch_conv_first(const ConvArgs &a, const float *w_hwio, int dtype, hipStream_t s);
// staged tensor in the format of dtype (Y3_DTYPE_*) -> fp32, npix pixels of C channels (fp32: a device-to-device copy)
hipError_t launch_to_f32(int dtype, const void *src, float *dst, size_t npix, int C, hipStream_t s);

// fused stem (conv_stem.hip): conv0 (3x3/1, 3->32) + conv1 (3x3/2, 32->64), both BN + optional leaky, one launch
struct StemArgs {
    const float *img;      // [B,H,W,3] fp32
    const float *w0;       // conv0 weights [28][32] fp32, row k = (u*3 + v)*3 + c, row 27 = 0 (fp32 kernel: BN scale folded in;
                           // fp16 kernel: every channel divided by a power of two 2^e_n, its largest magnitude in [1, 2))
    const float *scale0;   // [32]  (16-bit kernels only: y = acc*scale + shift like the stand-alone launches; fp16 kernel: scale * 2^e_n)
    const float *shift0;   // [32]
    const void *w1;        // conv1 packed [64][288], k = tap*32 + c: fp32 with the BN scale folded in / bf16 unscaled
    const float *scale1;   // [64]  (bf16 kernel only)
    const float *shift1;   // [64]
    void *dst;             // [B,H/2,W/2,64] fp32 / bf16
    // optional third layer: the 1x1 conv reading conv1's output (64 -> 32, BN, leaky), computed from the tile
    // while it is still on chip.  w2 = nullptr: absent.
    const void *w2;        // packed [32][64]: fp32 with the BN scale folded in / bf16 unscaled
    const float *scale2;   // [32]  (bf16 kernel only)
    const float *shift2;   // [32]
    void *dst2;            // [B,H/2,W/2,32] fp32 / bf16
    int leaky2;
    unsigned dst2_bytes;
    int B, H, W;           // image height and width, each % 32 == 0
    int leaky0, leaky1;
    unsigned img_bytes, dst_bytes;
    int tiles_y, tiles_x, n_tiles;   // filled by the launcher
    // measurement only (y3_net_measure_sclk): when non-null, wave 0 of workgroup 0 stores {s_memtime, s_memrealtime} at
    // kernel entry and exit -> shader clock held during the kernel = d(memtime) / d(memrealtime) x 100 MHz.  Null in
    // every product launch: no stamp instruction executes then.
    unsigned long long *clk_stamps;  // [4]
    int device;            // as ConvArgs::device
    int n_cus;             // as ConvArgs::n_cus (one / two persistent workgroups per CU)
};
hipError_t launch_conv_stem_f32(const StemArgs &a, hipStream_t s);
hipError_t launch_conv_stem_bf16(const StemArgs &a, hipStream_t s);   // conv0 on bf16 MFMA from split (hi + lo) operands (~2^-16 per product), bf16 patch, conv1 on bf16 MFMA
hipError_t launch_conv_stem_f16(const StemArgs &a, hipStream_t s);    // the same kernel on f16 MFMA: conv0 from (hi + lo' 2^-11) operands (~2^-22 per product), fp16 patch

// fused stem of YOLOv3-tiny (conv_tiny_stem.hip): conv0 (3x3/1, 3->16) + max-pool 2x2/2 + conv1 (3x3/1, 16->32) + max-pool 2x2/2, both convs
// BN + optional leaky, one launch at the real widths; only pool 1's tensor reaches memory
struct TinyStemArgs {
    const float *img;      // [B,H,W,3] fp32
    const float *w0;       // conv0 weights [27][16] fp32, row k = (u*3 + v)*3 + c, unscaled
    const float *scale0;   // [16]  y = acc*scale + shift, as the stand-alone first-layer launch
    const float *shift0;   // [16]
    const void *w1;        // conv1 weights [144][32], row k = tap*16 + c, unscaled: fp32 / bf16 / fp16
    const float *scale1;   // [32]
    const float *shift1;   // [32]
    void *dst;             // [B,H/4,W/4,32] fp32 / bf16 / fp16
    int B, H, W;           // image height and width, each % 32 == 0
    int leaky0, leaky1;
    int tiles_y, tiles_x, n_tiles;   // filled by the launcher
    int device;            // as ConvArgs::device
    int n_cus;             // as ConvArgs::n_cus (persistent workgroups)
};
hipError_t launch_conv_tiny_stem_f32(const TinyStemArgs &a, hipStream_t s);
hipError_t launch_conv_tiny_stem_bf16(const TinyStemArgs &a, hipStream_t s);
hipError_t launch_conv_tiny_stem_f16(const TinyStemArgs &a, hipStream_t s);

// bf16 path (conv_bf16.hip; the kernel body, shared with the fp16 path: conv_16bit.h)
static constexpr int BF16_TILE_COUNT = 37;   // 32: the weight-resident 3x3 kernel (conv_res_bf16.hip); 20, 33..36: retired ids
TileInfo conv_bf16_tile_info(int tile);
bool conv_bf16_tile_built(int tile);
hipError_t launch_conv_bf16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s);
// split-K form of the same conv (conv_bf16.hip): S >= 2 slices of the K walk (K tiles of 64) as S times the workgroups, raw fp32
// accumulators into ws [S][Mpad][CoutPad] (at least S * split_slab_bytes), then splitk_finish16 on the same stream: the
// slabs added in the order 0..S-1, the epilogue, the store to a.dst (bf16, or fp32 with out_f32).  Tiles 11 and 12 only.
// launch_conv_f16_split (conv_f16.hip): the same for fp16 plans; conv_bf16_split_tile answers for both.
bool conv_bf16_split_tile(int tile);
hipError_t launch_conv_bf16_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s);
// weight-resident 3x3 / stride-1 conv for Cin = 32 / 64 (conv_res_bf16.hip): the early short-K layers of the bf16 path
bool conv_res_bf16_fits(const ConvArgs &a);
hipError_t launch_conv_res_bf16(const ConvArgs &a, hipStream_t s);
// fp16 path (conv_f16.hip, conv_res_f16.hip; Y3_DTYPE_F16): the same kernels on the f16 forms of the two MFMA instructions, the bf16
// path's tile ids and table (conv_bf16_tile_info / conv_bf16_tile_built / conv_res_bf16_fits / conv_bf16_split_tile answer for both)
hipError_t launch_conv_f16(const ConvArgs &a, int tile, bool out_f32, hipStream_t s);
hipError_t launch_conv_f16_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s);
hipError_t launch_conv_res_f16(const ConvArgs &a, hipStream_t s);

// int8 path (conv_i8.hip; Y3_DTYPE_I8): int8 operands, exact i32 accumulate, the ids of the bf16 table for the tiles that have an int8 form
// (LDS-DMA, 128-byte rows: 8, 10, 11, 12, 17, 19 and 24, 26, 27, 29 on the 16x16x64 form); bk = 128 channels.  out_f32: a.dst is an fp32 grid.
TileInfo conv_i8_tile_info(int tile);
bool conv_i8_tile_built(int tile);
hipError_t launch_conv_i8(const ConvArgs &a, int tile, bool out_f32, hipStream_t s);
// split-K form of the same conv (conv_i8.hip): S >= 2 slices of the K walk (K tiles of 128) as S times the workgroups, raw i32
// accumulators into ws [S][Mpad][CoutPad] of 4-byte elements (at least S * split_slab_bytes), then splitk_finish_i8 on the same stream:
// the slabs added as integers (exact: the unsplit launch's bits at every S), the int8 epilogue, the store to a.dst (int8, or fp32 with
// out_f32).  Tiles 11 and 12 only (conv_i8_split_tile); the checks of launch_conv_i8.
bool conv_i8_split_tile(int tile);
hipError_t launch_conv_i8_split(const ConvArgs &a, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t s);
// n fp16 values (n % 16 == 0) -> int8: q = clamp(rintf((float)x * inv_s), -127, 127); and int8 -> fp32: (float)q * s  (elementwise.hip)
hipError_t launch_quantize16_to_i8(const void *src_f16, void *dst_i8, size_t n, float inv_s, hipStream_t s);
hipError_t launch_i8_to_f32(const void *src_i8, float *dst, size_t n, float scale, hipStream_t s);

// fp32-accurate path on the bf16 matrix cores, three bf16 planes per value (conv_f32x3.hip)
static constexpr int X3_TILE_COUNT = 34;
TileInfo conv_x3_tile_info(int tile);
hipError_t launch_conv_f32x3(const ConvArgs &a, int tile, bool out_f32, hipStream_t s);
// two fp16 planes per value on the fp16 matrix cores (same kernel, same tile ids; a subset is instantiated)
hipError_t launch_conv_f32x2(const ConvArgs &a, int tile, bool out_f32, hipStream_t s);
bool conv_x3_tile_built(int tile);     // 9, 13, 14: three planes only
bool conv_x2_tile_built(int tile);     // 26, 27: two planes only

hipError_t launch_add(const float *a, const float *b, float *y, size_t n, hipStream_t s);
hipError_t launch_upsample2x(const float *x, int B, int H, int W, int C, float *y, hipStream_t s);
hipError_t launch_concat(const float *a, int Ca, const float *b, int Cb, size_t npix, float *y, hipStream_t s);
// MaxPooling2D(2, stride 1 | 2, 'same') on [B,H,W,C] elements of dtype Y3_DTYPE_F32 / _BF16 / _F16 / _I8 (maxpool.hip)
hipError_t launch_maxpool2x2(const void *src, void *dst, int B, int H, int W, int C, int stride, int dtype, hipStream_t s);

struct DecodeArgs {   // of one to three scales: an absent scale has gh = gw = 0, no boxes and no workgroup
    const float *grid[3];
    int gh[3], gw[3];   // grid rows and columns of each scale
    int off[3];     // first box index of each scale
    float anchors[3][3][2];
    int B, N, nc;
};
size_t decode_lds_bytes(int nc);   // dynamic LDS of a decode-shaped workgroup (decode_tile.h): decode_kernel and candidates_kernel
hipError_t launch_decode(const DecodeArgs &a, float *bboxes, float *conf, float *probs, int64_t *cls,
                         float *scores, hipStream_t s);
hipError_t launch_class_scores(const float *conf, const float *probs, size_t n, int nc, int64_t *cls,
                               float *scores, hipStream_t s);
// Multi-label candidates (candidates.hip; include/y3.h, y3_yolo_decode_candidates_hw): count, per-image prefix, write.  counts: [B,N] i32 scratch.
hipError_t launch_candidates(const DecodeArgs &a, float S, int K, float *cand_boxes, int64_t *cand_cls, float *cand_scores,
                             int32_t *cand_src, int32_t *totals, int32_t *counts, hipStream_t s);
// ... from decoded tensors: bboxes [B,N,4], conf [B,N], probs [B,N,nc]
hipError_t launch_class_candidates(const float *bboxes, const float *conf, const float *probs, int B, int N, int nc, float S, int K,
                                   float *cand_boxes, int64_t *cand_cls, float *cand_scores, int32_t *cand_src, int32_t *totals,
                                   int32_t *counts, hipStream_t s);
// word 6 of every valid packed row: candidate k -> cand_src[b, k]
hipError_t launch_candidate_sources(void *packed, const int32_t *nv, const int32_t *cand_src, int B, int K, int M, hipStream_t s);

// Letterbox geometry (include/y3.h, Y3_IMAGE_LETTERBOX): the aspect-preserving resize is to sh x sw, placed at (top, left) of
// the Hc x Wc canvas (square entry points: Hc = Wc = S).  Layout of the int32[4] rows of y3_letterbox_geometry / y3_unletterbox_detections.
struct LetterboxGeom { int32_t sh, sw, top, left; };
// The one definition of the geometry: fp32, round half to even (reference core/utils.py:17-28 through tf.image.resize(
// preserve_aspect_ratio=True)); host only.  The same formula in double gives another (sh, sw) for some sizes.
LetterboxGeom letterbox_geom(int h, int w, int Hc, int Wc);
inline bool letterbox_geom_fits(const LetterboxGeom &g, int Hc, int Wc)
{
    return g.sh >= 1 && g.sw >= 1 && g.top >= 0 && g.left >= 0 && g.top <= Hc - g.sh && g.left <= Wc - g.sw;
}

// mode: 0, 1, 2 (y3_preprocess_image's is_uint8), optionally | Y3_IMAGE_LETTERBOX with the geometry g
hipError_t launch_resize(const void *src, int mode, int H, int W, int pix_stride, float *dst, int Hc, int Wc, const LetterboxGeom &g,
                         hipStream_t s);
// What preprocess_batch_kernel resizes into one slot: a strided view of the pixel blob and where it lands on the canvas.  The kernel knows
// nothing of images or tiles: an image is the whole-frame view of itself (pitch_px == cols), a tile a window of its frame (pitch_px == the
// frame's width).  first: byte offset of the view's first pixel in the blob, computed on the host.  mode: y3_image_desc.mode.
struct ResizeView { uint64_t first; int32_t rows, cols, pitch_px, channels, mode; LetterboxGeom g; };
// The views of one launch, passed by value in the kernel arguments (the limit is 4 KB).
constexpr int kResizeTableViews = 72;
struct ResizeTable { ResizeView v[kResizeTableViews]; };
static_assert(sizeof(ResizeView) == 48 && sizeof(ResizeTable) + 64 <= 4096, "view table must fit the kernel arguments");
// table.v[0 .. n): validated views, n in 1..kResizeTableViews; dst: slot of the first one
hipError_t launch_preprocess_batch(const void *pixels, const ResizeTable &table, int n, float *dst, int Hc, int Wc, hipStream_t s);

// Sliced inference, the merge (tiles.hip; include/y3.h, y3_merge_tile_detections).  One entry per tile image: its window of the frame, its
// letterbox geometry on the canvas and the frame's extent; 64 entries per merge_tiles_kernel launch, by value in the kernel arguments.
constexpr int kMergeTableTiles = 64, kMergeMaxTiles = 64;
struct MergeTile { int32_t y0, x0, ch, cw; LetterboxGeom g; int32_t h, w; };
struct MergeTable { MergeTile t[kMergeTableTiles]; };
static_assert(sizeof(MergeTile) == 40 && sizeof(MergeTable) + 64 <= 4096, "merge table must fit the kernel arguments");
// packed / nv: the first tile image of the launch; boxes / scores / cls: its first candidate (image i of the launch owns candidates
// [i * M, (i + 1) * M)); n: 1..kMergeTableTiles entries
hipError_t launch_merge_tiles(const void *packed, const int32_t *nv, const MergeTile *entries, int n, int M, int Hc, int Wc, float *boxes,
                              float *scores, int64_t *cls, hipStream_t s);

// The geometries of one unletterbox_kernel launch, by value in the kernel arguments like ResizeTable.
constexpr int kUnletterboxTableImages = 64;
struct UnletterboxTable { LetterboxGeom g[kUnletterboxTableImages]; };
hipError_t launch_unletterbox(void *packed, const int32_t *nv, const LetterboxGeom *geoms, int n, int M, int Hc, int Wc, hipStream_t s);

// Evaluation counters (evaluate.hip; include/y3.h, y3_evaluate_detections).  The score thresholds of one launch travel by value in the
// kernel arguments, like the letterbox geometries.
constexpr int kEvalMaxBoxes = 1024, kEvalMaxGt = 1024, kEvalMaxClasses = 4096, kEvalMaxThresholds = 16;
struct EvalThresholds { float s[kEvalMaxThresholds]; };
size_t evaluate_lds_bytes(int max_gt, int nclasses);
hipError_t launch_evaluate(const void *packed, const int32_t *nv, int B, int M, const float *gt_boxes, const int32_t *gt_classes,
                           const int32_t *gt_count, int G, int nc, float iou_thr, const EvalThresholds &thr, int T, int one_class,
                           int64_t *counters, hipStream_t s);

// Matching for average precision (ap_match.hip; include/y3.h, y3_match_detections): the same inputs and limits, the IoU thresholds
// of one launch by value in the kernel arguments (thr.s[0 .. K)), one wave per threshold.
size_t ap_match_lds_bytes(int max_boxes, int max_gt, int nclasses);
hipError_t launch_ap_match(const void *packed, const int32_t *nv, int B, int M, const float *gt_boxes, const int32_t *gt_classes,
                           const int32_t *gt_count, int G, int nc, const EvalThresholds &thr, int K, int one_class, uint32_t *records,
                           int64_t *totals, hipStream_t s);

// Validation loss (loss.hip; include/y3.h, y3_yolo_assign_targets / y3_yolo_loss).  Grid sizes, the first decode row of each scale and the
// anchors travel by value in the kernel arguments.  A grid side is at most kLossMaxGrid: row indices stay far inside an int and the
// bitmap of a scale's rows inside LDS.
constexpr int kLossMaxGrid = 256;
struct LossGeom { int g[3]; int off[3]; float anchors[3][3][2]; };
struct LossGrids { const float *p[3]; };
size_t loss_lds_bytes(int max_gt, int g);
hipError_t launch_assign_targets(const float *gt_boxes, const int32_t *gt_classes, const int32_t *gt_count, int B, int G, int nc,
                                 const LossGeom &geo, int32_t *cells, hipStream_t s);
hipError_t launch_yolo_loss(const LossGrids &grids, const LossGeom &geo, int B, int nc, const float *gt_boxes,
                            const int32_t *gt_classes, const int32_t *cells, int G, double *loss, hipStream_t s);

size_t nms_workspace_bytes(int B, int N);
size_t nms_per_class_workspace_bytes(int B, int N);   // the above + B * N * 4: the class ids of the spilled kept boxes
// cls: null for the class-agnostic rule; the class ids [B,N] for the per-class one, ws then holding nms_per_class_workspace_bytes
hipError_t launch_nms(const float *boxes, const float *scores, const int64_t *cls, int B, int N, int M, float T, float S,
                      int32_t *sel, int32_t *num_valid, void *ws, hipStream_t s);
hipError_t launch_pack(const float *boxes, const int64_t *cls, const float *scores, const int32_t *sel,
                       const int32_t *nv, int B, int N, int M, void *packed, hipStream_t s);

}  // namespace y3
