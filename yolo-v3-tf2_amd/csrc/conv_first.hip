// First layer: 3x3 / stride 1 / Cin = 3 / Cout = 32 conv + BN + LeakyReLU (reference: core/parse_model.py:27-52 applied to
// config/models/yolov3/backbone.yaml layer 1), direct on the VALU: K = 27 is too thin for the MFMA tile and the layer is bound by
// its output bytes.  Runs when the stem is not fused (keep_activations, early chunks, the plane-split plans).
// One thread = one output pixel x all output channels; fp32 image in, fp32 arithmetic in every mode; weights are wave-uniform
// (scalar loads), accumulation order (u,v,c) like the GEMM kernel's k order.  The output leaves in the plan's format (FMT =
// Y3_DTYPE_*): fp32, bf16, fp16, three bf16 planes or two fp16 planes per value.
#include "../../include/y3.h"
#include "y3_device.h"
#include "y3_kernels.h"

namespace y3 {

template <int COUT, int FMT>
__global__ __launch_bounds__(256) void conv_first(const ConvArgs p, const float *__restrict__ w)
{
    // per-wave transpose buffer: 64 pixels x (COUT + 4) floats (row stride 9 x 16 B -> conflict-free b128 access)
    constexpr int ROW = COUT + 4;
    __shared__ __attribute__((aligned(16))) float tr[4][64 * ROW];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int mw = blockIdx.x * 256 + wave * 64;  // first pixel of this wave
    const int m = mw + lane;
    const int HW = p.H * p.W;
    const bool live = m < p.M;
    const int mm = live ? m : 0;
    const int b = mm / HW;
    const int r = mm - b * HW;
    const int ho = r / p.W, wo = r - ho * p.W;
    const float *x = static_cast<const float *>(p.src0);
    f32x2 acc2[COUT / 2];   // packed pairs: v_pk_fma_f32 retires two MACs per VALU instruction
#pragma unroll
    for (int n = 0; n < COUT / 2; ++n) acc2[n] = f32x2{0.0f, 0.0f};
#pragma unroll 1
    for (int u = 0; u < 3; ++u) {
        const int hi = ho - 1 + u;
#pragma unroll 1
        for (int v = 0; v < 3; ++v) {
            const int wi = wo - 1 + v;
            const bool ok = live && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            const float *xp = x + ((size_t)(b * p.H + (ok ? hi : 0)) * p.W + (ok ? wi : 0)) * 3;
            float xv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) xv[c] = ok ? xp[c] : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *wr = w + ((u * 3 + v) * 3 + c) * COUT;  // HWIO, wave-uniform address -> scalar loads
#pragma unroll
                for (int n = 0; n < COUT; n += 2)
                    acc2[n / 2] = __builtin_elementwise_fma(f32x2{xv[c], xv[c]}, f32x2{wr[n], wr[n + 1]}, acc2[n / 2]);
            }
        }
    }
    // epilogue into LDS (lane = pixel), then 16-B stores with several lanes per pixel: every wave store instruction writes
    // contiguous NHWC output (the lane-per-pixel store wrote 16 B per 128-B line and cost 2.2x the bytes at the memory side:
    // WRITE_SIZE in profiles/r01_derived.txt)
    float *t = tr[wave];
#pragma unroll
    for (int n = 0; n < COUT; n += 4) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = acc2[(n + e) / 2][(n + e) & 1] * p.scale[n + e] + p.shift[n + e];
            if (p.leaky) v = fmaxf(v, 0.1f * v);
            o[e] = v;
        }
        *reinterpret_cast<f32x4 *>(t + lane * ROW + n) = o;
    }
    // same wave wrote and reads: no barrier needed, only the LDS counter (compiler inserts the wait)
    if constexpr (FMT == Y3_DTYPE_F32) {
        float *dst = static_cast<float *>(p.dst);
        constexpr int CH = COUT / 4;           // 16-B chunks (4 floats) per pixel
        constexpr int PPI = 64 / CH;           // pixels per store instruction
        const int c4 = lane % CH, pl = lane / CH;
#pragma unroll
        for (int it = 0; it < CH; ++it) {
            const int px = it * PPI + pl;
            const f32x4 o = *reinterpret_cast<const f32x4 *>(t + px * ROW + c4 * 4);
            if (mw + px < p.M) *reinterpret_cast<f32x4 *>(dst + (size_t)(mw + px) * COUT + c4 * 4) = o;
        }
    } else {
        unsigned short *dst = static_cast<unsigned short *>(p.dst);
        constexpr int CH = COUT / 8;           // 16-B pieces (8 channels of one plane) per pixel
        constexpr int PPI = 64 / CH;
        const int c8 = lane % CH, pl = lane / CH;
#pragma unroll
        for (int it = 0; it < CH; ++it) {
            const int px = it * PPI + pl;
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(t + px * ROW + c8 * 8);
            const f32x4 v1 = *reinterpret_cast<const f32x4 *>(t + px * ROW + c8 * 8 + 4);
            if constexpr (FMT == Y3_DTYPE_BF16) {
                u32x4 o;
                o[0] = pack_bf16(v0[0], v0[1]);
                o[1] = pack_bf16(v0[2], v0[3]);
                o[2] = pack_bf16(v1[0], v1[1]);
                o[3] = pack_bf16(v1[2], v1[3]);
                if (mw + px < p.M) *reinterpret_cast<u32x4 *>(dst + (size_t)(mw + px) * COUT + c8 * 8) = o;
            } else if constexpr (FMT == Y3_DTYPE_F16) {
                u32x4 o;
                o[0] = pack_f16(v0[0], v0[1]);
                o[1] = pack_f16(v0[2], v0[3]);
                o[2] = pack_f16(v1[0], v1[1]);
                o[3] = pack_f16(v1[2], v1[3]);
                if (mw + px < p.M) *reinterpret_cast<u32x4 *>(dst + (size_t)(mw + px) * COUT + c8 * 8) = o;
            } else {
                constexpr int NPL = FMT == Y3_DTYPE_F32X3 ? 3 : 2;
                const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                u32x4 o[NPL];
                split_planes<NPL>(v, o);
                if (mw + px < p.M) {
#pragma unroll
                    for (int q = 0; q < NPL; ++q)
                        *reinterpret_cast<u32x4 *>(dst + (size_t)(mw + px) * NPL * COUT + q * COUT + c8 * 8) = o[q];
                }
            }
        }
    }
}

hipError_t launch_conv_first(const ConvArgs &a, const float *w_hwio, int dtype, hipStream_t s)
{
    if (a.Cin != 3 || a.ksize != 3 || a.stride != 1 || a.Cout != 32 || a.residual || a.src1) return hipErrorInvalidValue;
    const dim3 grid((a.M + 255) / 256), block(256);
    switch (dtype) {
        case Y3_DTYPE_F32: hipLaunchKernelGGL((conv_first<32, Y3_DTYPE_F32>), grid, block, 0, s, a, w_hwio); break;
        case Y3_DTYPE_BF16: hipLaunchKernelGGL((conv_first<32, Y3_DTYPE_BF16>), grid, block, 0, s, a, w_hwio); break;
        case Y3_DTYPE_F32X3: hipLaunchKernelGGL((conv_first<32, Y3_DTYPE_F32X3>), grid, block, 0, s, a, w_hwio); break;
        case Y3_DTYPE_F32X2: hipLaunchKernelGGL((conv_first<32, Y3_DTYPE_F32X2>), grid, block, 0, s, a, w_hwio); break;
        case Y3_DTYPE_F16: hipLaunchKernelGGL((conv_first<32, Y3_DTYPE_F16>), grid, block, 0, s, a, w_hwio); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace y3
