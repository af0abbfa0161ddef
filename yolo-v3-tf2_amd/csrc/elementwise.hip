// Stand-alone Add / UpSampling2D(2) / Concatenate(axis=3) (reference: core/parse_model.py:155-156,72,134).
// YOLOv3's own graph never launches these (the lowering folds all of them into conv launches); they exist
// so that a model description whose pattern does not fold still runs.  HBM-bound, 16-B accesses.
// Also the conversion of a staged tensor (held in the plan's format) to fp32.
#include "../../include/y3.h"
#include "y3_device.h"
#include "y3_kernels.h"

namespace y3 {

__global__ __launch_bounds__(256) void add_kernel(const f32x4 *a, const f32x4 *b, f32x4 *y, size_t n4)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) y[i] = a[i] + b[i];
}

hipError_t launch_add(const float *a, const float *b, float *y, size_t n, hipStream_t s)
{
    if (n & 3) return hipErrorInvalidValue;
    const size_t n4 = n >> 2;
    const unsigned blocks = (unsigned)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(add_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, (const f32x4 *)a, (const f32x4 *)b,
                       (f32x4 *)y, n4);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void upsample2x_kernel(const f32x4 *x, int B, int H, int W, int C4, f32x4 *y)
{
    const size_t total = (size_t)B * 2 * H * 2 * W * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        size_t pix = i / C4;
        const int w2 = (int)(pix % (2 * W));
        pix /= (2 * W);
        const int h2 = (int)(pix % (2 * H));
        const int b = (int)(pix / (2 * H));
        y[i] = x[(((size_t)b * H + (h2 >> 1)) * W + (w2 >> 1)) * C4 + c];
    }
}

hipError_t launch_upsample2x(const float *x, int B, int H, int W, int C, float *y, hipStream_t s)
{
    if (C & 3) return hipErrorInvalidValue;
    const size_t total = (size_t)B * 4 * H * W * (C >> 2);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(upsample2x_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, (const f32x4 *)x, B, H, W,
                       C >> 2, (f32x4 *)y);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void concat_kernel(const f32x4 *a, int Ca4, const f32x4 *b, int Cb4, size_t npix,
                                                     f32x4 *y)
{
    const int C4 = Ca4 + Cb4;
    const size_t total = npix * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const size_t pix = i / C4;
        y[i] = (c < Ca4) ? a[pix * Ca4 + c] : b[pix * Cb4 + (c - Ca4)];
    }
}

hipError_t launch_concat(const float *a, int Ca, const float *b, int Cb, size_t npix, float *y, hipStream_t s)
{
    if ((Ca | Cb) & 3) return hipErrorInvalidValue;
    const size_t total = npix * ((Ca + Cb) >> 2);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(concat_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, (const f32x4 *)a, Ca >> 2,
                       (const f32x4 *)b, Cb >> 2, npix, (f32x4 *)y);
    return hipGetLastError();
}

// staged tensor -> fp32 (the end of a forward in a non-fp32 plan, y3_net_read_tensor): bf16, fp16, or FMT's planes of each pixel rebuilt
// with join_planes -- the summation order of the conv kernels' shortcut operand
template <int FMT>
__global__ __launch_bounds__(256) void to_f32_kernel(const unsigned short *x, float *y, size_t npix, int C)
{
    const size_t n = npix * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if constexpr (FMT == Y3_DTYPE_BF16) {
            y[i] = __uint_as_float((unsigned)x[i] << 16);
        } else if constexpr (FMT == Y3_DTYPE_F16) {
            y[i] = (float)__builtin_bit_cast(_Float16, x[i]);
        } else {
            constexpr int NPL = FMT == Y3_DTYPE_F32X3 ? 3 : 2;
            const size_t px = i / C;
            const int c = (int)(i - px * C);
            const unsigned short *q = x + px * NPL * C + c;
            u32x4 planes[NPL];
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) planes[pl] = u32x4{q[pl * C], 0u, 0u, 0u};
            float lo, hi;
            join_planes<NPL>(planes, 0, lo, hi);
            y[i] = lo;
        }
    }
}

hipError_t launch_to_f32(int dtype, const void *src, float *dst, size_t npix, int C, hipStream_t s)
{
    const size_t n = npix * C;
    if (dtype == Y3_DTYPE_F32) return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    const dim3 grid(blocks ? blocks : 1), block(256);
    const unsigned short *x = static_cast<const unsigned short *>(src);
    switch (dtype) {
        case Y3_DTYPE_BF16: hipLaunchKernelGGL(to_f32_kernel<Y3_DTYPE_BF16>, grid, block, 0, s, x, dst, npix, C); break;
        case Y3_DTYPE_F32X3: hipLaunchKernelGGL(to_f32_kernel<Y3_DTYPE_F32X3>, grid, block, 0, s, x, dst, npix, C); break;
        case Y3_DTYPE_F32X2: hipLaunchKernelGGL(to_f32_kernel<Y3_DTYPE_F32X2>, grid, block, 0, s, x, dst, npix, C); break;
        case Y3_DTYPE_F16: hipLaunchKernelGGL(to_f32_kernel<Y3_DTYPE_F16>, grid, block, 0, s, x, dst, npix, C); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- int8 plans: the boundary copy of a tensor written before the cut (fp16 -> int8) and a stored int8 net output -> fp32 ----
// q = clamp(rintf((float)x * inv_s), -127, 127): sixteen values per thread, two 16-byte loads and one 16-byte store
__global__ __launch_bounds__(256) void quantize16_to_i8(const u32x4 *x, u32x4 *y, size_t n16, float inv_s)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        const u32x4 a = x[2 * i], b = x[2 * i + 1];
        u32x4 out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned w0 = k < 2 ? a[2 * k] : b[2 * k - 4], w1 = k < 2 ? a[2 * k + 1] : b[2 * k - 3];
            const float v[4] = {f16lo(w0), f16hi(w0), f16lo(w1), f16hi(w1)};
            unsigned w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= ((unsigned)(int)fminf(fmaxf(rintf(v[j] * inv_s), -127.0f), 127.0f) & 0xffu) << (8 * j);
            out[k] = w;
        }
        y[i] = out;
    }
}

hipError_t launch_quantize16_to_i8(const void *src_f16, void *dst_i8, size_t n, float inv_s, hipStream_t s)
{
    if ((n & 15) || ((uintptr_t)src_f16 & 15) || ((uintptr_t)dst_i8 & 15)) return hipErrorInvalidValue;
    const size_t n16 = n >> 4;
    const unsigned blocks = (unsigned)((n16 + 255) / 256 < 4096 ? (n16 + 255) / 256 : 4096);
    hipLaunchKernelGGL(quantize16_to_i8, dim3(blocks ? blocks : 1), dim3(256), 0, s, static_cast<const u32x4 *>(src_f16),
                       static_cast<u32x4 *>(dst_i8), n16, inv_s);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void i8_to_f32(const signed char *x, float *y, size_t n, float scale)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = (float)x[i] * scale;
}

hipError_t launch_i8_to_f32(const void *src_i8, float *dst, size_t n, float scale, hipStream_t s)
{
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(i8_to_f32, dim3(blocks ? blocks : 1), dim3(256), 0, s, static_cast<const signed char *>(src_i8), dst, n, scale);
    return hipGetLastError();
}

}  // namespace y3
