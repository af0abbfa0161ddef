// Image input stage on the GPU (SURVEY.md 8f "n2"): uint8 HWC image -> float32 in [0,1] -> bilinear resize to
// Hc x Wc (a square S x S for the entry points without _hw), written straight into slot b of the NHWC batch the conv program reads.
// Replaces, for the image_file / images_dir sources of reference inference.py:157-158,
//   tf.image.decode_image(..., channels=3, dtype=tf.float32)   (uint8 -> float: cast * (1/255), alpha dropped)
//   tf.image.resize(image, (S, S))                              (bilinear, antialias=False, half-pixel centres)
// and, for the tfrecords source (reference core/load_tfrecords.py:46-48),
//   tf.image.resize(decode_jpeg(...), (S, S)) / 255            (uint8 values resized as floats, then a true divide)
// which is mode 2 below.
// Arithmetic restated from TF's ResizeBilinear CPU kernel: in = (out + 0.5) * (in_size / out_size) - 0.5,
// lower = max(floor(in), 0), upper = min(ceil(in), in_size - 1), lerp = in - floor(in); interpolate along x first
// (top, bottom) then along y; fp32, no contraction.  HBM-bound and tiny.  resize_kernel: one image per launch, one thread per
// output pixel; preprocess_batch_kernel: up to 72 unlike views per launch, four pixels per thread -- a view is a whole image or a window of
// one, each window an image of its own (sliced inference; include/y3.h, y3_preprocess_tiles_hw).
// Both also serve the aspect-preserving form of reference core/utils.py:17-28 (resize_image: tf.image.resize(
// preserve_aspect_ratio=True) + pad_to_bounding_box), flag Y3_IMAGE_LETTERBOX: resize to sh x sw, centred on a zero canvas.
#include <type_traits>

#include "y3_kernels.h"

namespace y3 {

template <typename T>
__device__ __forceinline__ float px(const T *p);
template <>
__device__ __forceinline__ float px<unsigned char>(const unsigned char *p) { return (float)(*p) * (1.0f / 255.0f); }
template <>
__device__ __forceinline__ float px<float>(const float *p) { return *p; }

struct RawU8 { unsigned char v; };   // uint8 taken as 0..255, divided by 255 after the resize (mode 2)
template <>
__device__ __forceinline__ float px<RawU8>(const RawU8 *p) { return (float)p->v; }

// One output pixel (3 floats) of the resize: the per-pixel body of both kernels below, so that the per-image and the
// batched launch cannot drift apart.  i = oy * Wc + ox on the Hc x Wc canvas.
// LB (Y3_IMAGE_LETTERBOX): the resize is to g.sh x g.sw and sits at (g.top, g.left) of the canvas; a pixel outside that
// block is 0.0f -- it is written like any other, a reused slot keeps nothing of its last image.  Inside, the same operations in
// the same order with (sh, sw) in the place of (Hc, Wc).  LB = false compiles to what it was before the flag existed.
// row_pitch: elements of T from one source row to the next -- W * pix_stride for an image of its own, the frame's pitch for a window
// of a frame (ResizeView), whose taps clamp at the window's edges like any image's.
template <typename T, bool LB>
__device__ __forceinline__ void resize_pixel(const T *__restrict__ src, int H, int W, int pix_stride, size_t row_pitch, int Hc, int Wc,
                                             LetterboxGeom g, int i, float *out)
{
    int oy = i / Wc, ox = i - oy * Wc;
    if (LB) {
        oy -= g.top;
        ox -= g.left;
        if ((unsigned)oy >= (unsigned)g.sh || (unsigned)ox >= (unsigned)g.sw) {
            out[0] = out[1] = out[2] = 0.0f;
            return;
        }
    }
    const int OH = LB ? g.sh : Hc, OW = LB ? g.sw : Wc;
    const float sy = (float)H / (float)OH, sx = (float)W / (float)OW;
    const float fy = ((float)oy + 0.5f) * sy - 0.5f, fx = ((float)ox + 0.5f) * sx - 0.5f;
    const float fly = floorf(fy), flx = floorf(fx);
    const int y0 = max((int)fly, 0), y1 = min((int)ceilf(fy), H - 1);
    const int x0 = max((int)flx, 0), x1 = min((int)ceilf(fx), W - 1);
    const float ly = fy - fly, lx = fx - flx;
    const T *r0 = src + (size_t)y0 * row_pitch, *r1 = src + (size_t)y1 * row_pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tl = px<T>(r0 + x0 * pix_stride + c), tr = px<T>(r0 + x1 * pix_stride + c);
        const float bl = px<T>(r1 + x0 * pix_stride + c), br = px<T>(r1 + x1 * pix_stride + c);
        const float top = tl + (tr - tl) * lx;
        const float bot = bl + (br - bl) * lx;
        const float v = top + (bot - top) * ly;
        out[c] = std::is_same<T, RawU8>::value ? v / 255.0f : v;
    }
}

template <typename T, bool LB>
__global__ __launch_bounds__(256) void resize_kernel(const T *__restrict__ src, int H, int W, int pix_stride,
                                                     float *__restrict__ dst, int Hc, int Wc, LetterboxGeom g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Hc * Wc) return;
    float v[3];
    resize_pixel<T, LB>(src, H, W, pix_stride, (size_t)W * pix_stride, Hc, Wc, g, i, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(size_t)i * 3 + c] = v[c];
}

// A batch of unlike views in one launch: blockIdx.y is the view within the launch, blockIdx.x tiles its Hc*Wc output pixels.
// The views travel by value in the kernel arguments (ResizeTable, 3.4 KB of the 4 KB limit): nothing extra is copied, they have
// no lifetime to manage, and the launch can be captured into a graph.  A tile has the bits a contiguous copy of its window gets: the
// same pixel body, reading the frame with the frame's row pitch from the window's first pixel.
// VEC: every thread produces four consecutive pixels (12 floats) and writes them as three 16-byte stores; needs
// Hc*Wc % 4 == 0 and a 16-byte aligned destination, which holds for every network size (sides multiples of 32).  Otherwise one
// pixel and three scalar stores per thread.  Each of the four pixels decides on its own whether it is padding: a thread may
// straddle the edge of the letterboxed block.
template <typename T, bool VEC, bool LB>
__device__ __forceinline__ void preprocess_batch_body(const T *__restrict__ src, int H, int W, int pix_stride, size_t row_pitch,
                                                      float *__restrict__ dst, int Hc, int Wc, LetterboxGeom g)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (q * 4 >= Hc * Wc) return;
        float v[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) resize_pixel<T, LB>(src, H, W, pix_stride, row_pitch, Hc, Wc, g, q * 4 + p, v + 3 * p);
        float4 *o = reinterpret_cast<float4 *>(dst + (size_t)q * 12);
        o[0] = make_float4(v[0], v[1], v[2], v[3]);
        o[1] = make_float4(v[4], v[5], v[6], v[7]);
        o[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
        if (q >= Hc * Wc) return;
        float v[3];
        resize_pixel<T, LB>(src, H, W, pix_stride, row_pitch, Hc, Wc, g, q, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[(size_t)q * 3 + c] = v[c];
    }
}

// src: the first pixel of the H x W image (or window); pix_stride channels per pixel, pitch_px pixels from one row to the next
template <bool VEC, bool LB>
__device__ __forceinline__ void preprocess_batch_modes(const unsigned char *__restrict__ src, int H, int W, int pix_stride, int pitch_px,
                                                       int mode, float *__restrict__ dst, int Hc, int Wc, LetterboxGeom g)
{
    const size_t row_pitch = (size_t)pitch_px * pix_stride;
    if (mode == 2)
        preprocess_batch_body<RawU8, VEC, LB>(reinterpret_cast<const RawU8 *>(src), H, W, pix_stride, row_pitch, dst, Hc, Wc, g);
    else if (mode == 1)
        preprocess_batch_body<unsigned char, VEC, LB>(src, H, W, pix_stride, row_pitch, dst, Hc, Wc, g);
    else
        preprocess_batch_body<float, VEC, LB>(reinterpret_cast<const float *>(src), H, W, pix_stride, row_pitch, dst, Hc, Wc, g);
}

template <bool VEC>
__global__ __launch_bounds__(256) void preprocess_batch_kernel(const unsigned char *__restrict__ pixels, ResizeTable table,
                                                               float *__restrict__ batch, int Hc, int Wc)
{
    const ResizeView v = table.v[blockIdx.y];             // uniform per workgroup: scalar loads from the kernel arguments
    const unsigned char *src = pixels + v.first;
    float *dst = batch + (size_t)blockIdx.y * Hc * Wc * 3;
    const int mode = v.mode & ~Y3_IMAGE_LETTERBOX;
    if (v.mode & Y3_IMAGE_LETTERBOX)                      // one branch per workgroup each, outside the pixel body
        preprocess_batch_modes<VEC, true>(src, v.rows, v.cols, v.channels, v.pitch_px, mode, dst, Hc, Wc, v.g);
    else
        preprocess_batch_modes<VEC, false>(src, v.rows, v.cols, v.channels, v.pitch_px, mode, dst, Hc, Wc, LetterboxGeom{});
}

template <typename T>
static void launch_resize_as(bool lb, dim3 grid, hipStream_t s, const void *src, int H, int W, int pix_stride, float *dst, int Hc, int Wc,
                             const LetterboxGeom &g)
{
    if (lb)
        hipLaunchKernelGGL((resize_kernel<T, true>), grid, dim3(256), 0, s, static_cast<const T *>(src), H, W, pix_stride, dst, Hc, Wc, g);
    else
        hipLaunchKernelGGL((resize_kernel<T, false>), grid, dim3(256), 0, s, static_cast<const T *>(src), H, W, pix_stride, dst, Hc, Wc, g);
}

hipError_t launch_resize(const void *src, int mode, int H, int W, int pix_stride, float *dst, int Hc, int Wc, const LetterboxGeom &g,
                         hipStream_t s)
{
    dim3 grid((Hc * Wc + 255) / 256);
    const bool lb = (mode & Y3_IMAGE_LETTERBOX) != 0;
    const int m = mode & ~Y3_IMAGE_LETTERBOX;
    if (m == 2)
        launch_resize_as<RawU8>(lb, grid, s, src, H, W, pix_stride, dst, Hc, Wc, g);
    else if (m)
        launch_resize_as<unsigned char>(lb, grid, s, src, H, W, pix_stride, dst, Hc, Wc, g);
    else
        launch_resize_as<float>(lb, grid, s, src, H, W, pix_stride, dst, Hc, Wc, g);
    return hipGetLastError();
}

// Vector stores when the geometry allows.
hipError_t launch_preprocess_batch(const void *pixels, const ResizeTable &table, int n, float *dst, int Hc, int Wc, hipStream_t s)
{
    const bool vec = ((size_t)Hc * Wc) % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const int per_block = vec ? 1024 : 256;
    dim3 grid((unsigned)(((size_t)Hc * Wc + per_block - 1) / per_block), (unsigned)n), block(256);
    const unsigned char *p = static_cast<const unsigned char *>(pixels);
    if (vec)
        hipLaunchKernelGGL(preprocess_batch_kernel<true>, grid, block, 0, s, p, table, dst, Hc, Wc);
    else
        hipLaunchKernelGGL(preprocess_batch_kernel<false>, grid, block, 0, s, p, table, dst, Hc, Wc);
    return hipGetLastError();
}

}  // namespace y3
