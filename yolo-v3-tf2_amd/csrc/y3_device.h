// Device helpers shared by the gfx950 kernel sources (included by the .hip files only).
#pragma once
#include <hip/hip_runtime.h>

namespace y3 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void *lds_ptr;   // LDS destination of __builtin_amdgcn_raw_ptr_buffer_load_lds

// buffer resource over `bytes` bytes at p: a load at a voffset >= bytes returns 0 and a store there is dropped (the range check
// the kernels use for zero padding and ragged tiles)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000);
}

// XCD-aware tile order: workgroups b and b+8 share an XCD (and its L2); give each XCD a contiguous run of logical tiles so that
// the N-tiles of one pixel tile and neighbouring pixel tiles meet in one L2.  Returns the logical tile of workgroup bid of nwg;
// bijective for any grid size.
__device__ __forceinline__ int xcd_contiguous_tile(int bid, int nwg)
{
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// Shader-clock stamps of the measurement launches (y3_net_measure_sclk*: ConvArgs / StemArgs.clk_stamps, null in every product
// launch): thread 0 of the launch's middle workgroup (MIDDLE: one of its steady state) or of workgroup 0 stores
// {s_memtime, s_memrealtime} at out[slot], out[slot + 1].  (gridDim is read behind the null test, as the kernels did inline: a
// workgroup index passed in as an argument reordered the prologue of conv_f32_mfma and conv3x3_res_f32.)
template <bool MIDDLE>
__device__ __forceinline__ void clk_stamp(unsigned long long *out, int slot)
{
    if (out != nullptr && blockIdx.x == (MIDDLE ? gridDim.x >> 1 : 0) && threadIdx.x == 0) {
        out[slot] = __builtin_amdgcn_s_memtime();
        out[slot + 1] = __builtin_amdgcn_s_memrealtime();
    }
}
// conv kernels: the middle workgroup at its entry -> [0], [1]; workgroup 0 -> [4] = s_memrealtime, when the kernel began
__device__ __forceinline__ void clk_stamp_entry(unsigned long long *out)
{
    clk_stamp<true>(out, 0);
    if (out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) out[4] = __builtin_amdgcn_s_memrealtime();
}
// ... and the middle workgroup after its epilogue -> [2], [3]
__device__ __forceinline__ void clk_stamp_exit(unsigned long long *out) { clk_stamp<true>(out, 2); }

// ---- bf16 -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }
__device__ __forceinline__ unsigned short bf16_bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
// two values -> one word of two bf16 (lo in the low half)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi)
{
    const unsigned short a = bf16_bits(lo);
    const unsigned short b = bf16_bits(hi);
    return (unsigned)a | ((unsigned)b << 16);
}

// ---- fp16 (IEEE half; the conversions round to nearest even and overflow to inf, never a round-toward-zero pack) --------------
__device__ __forceinline__ unsigned short f16_bits(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
// two values -> one word of two fp16 (lo in the low half)
__device__ __forceinline__ unsigned pack_f16(float lo, float hi)
{
    const unsigned short a = f16_bits(lo);
    const unsigned short b = f16_bits(hi);
    return (unsigned)a | ((unsigned)b << 16);
}

// ---- element traits of the 16-bit MFMA conv kernels (conv_16bit.h, conv_res_16bit.h): the fragment of eight elements a lane feeds
// an MFMA, the two MFMA shapes with their accumulators, the element's size in bytes and its type as stored (conv_16bit.h is generic over
// both: I8Elem, conv_i8.hip), two floats -> one packed word (one rounding each, to nearest even), one packed word -> two floats.
// The lane maps of the operands and of the accumulators are the same for both types.  split_hi / split_lo: the two elements a value is split
// into for the fused stem's conv0 (conv_stem.hip): bf16 v = hi + lo; fp16 v = hi + lo * 2^-11 with hi = 0 below the normal range.
struct Bf16Elem {
    using frag = bf16x8;
    using acc32 = f32x16;   // accumulators of mfma32 / mfma16
    using acc16 = f32x4;
    using stored = unsigned short;
    static constexpr int BYTES = 2;
    using elem = __bf16;
    static __device__ __forceinline__ unsigned short bits(float x) { return bf16_bits(x); }
    static __device__ __forceinline__ elem split_hi(float v) { return (__bf16)v; }
    static __device__ __forceinline__ elem split_lo(float v, elem hi) { return (__bf16)(v - (float)hi); }
    static __device__ __forceinline__ f32x16 mfma32(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_bf16(lo, hi); }
    static __device__ __forceinline__ float widen_lo(unsigned w) { return __uint_as_float(w << 16); }
    static __device__ __forceinline__ float widen_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
};
struct F16Elem {
    using frag = f16x8;
    using acc32 = f32x16;   // accumulators of mfma32 / mfma16
    using acc16 = f32x4;
    using stored = unsigned short;
    static constexpr int BYTES = 2;
    using elem = _Float16;
    static __device__ __forceinline__ unsigned short bits(float x) { return f16_bits(x); }
    static __device__ __forceinline__ elem split_hi(float v) { return fabsf(v) < 6.103515625e-05f ? (_Float16)0.0f : (_Float16)v; }
    static __device__ __forceinline__ elem split_lo(float v, elem hi) { return (_Float16)((v - (float)hi) * 2048.0f); }
    static __device__ __forceinline__ f32x16 mfma32(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_f16(lo, hi); }
    static __device__ __forceinline__ float widen_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
    static __device__ __forceinline__ float widen_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
};

// ---- plane-split values (conv_f32x3.hip): three bf16 planes or two fp16 planes per fp32 value --------------------------------
// x -> (hi, mid, lo) bf16 bit patterns with hi + mid + lo == x (fp32 subtractions of nearby values are exact)
__device__ __forceinline__ void split3(float x, unsigned short &hi, unsigned short &mid, unsigned short &lo)
{
    const float h = bf16_round(x);
    const float r1 = x - h;
    const float m = bf16_round(r1);
    const float r2 = r1 - m;
    hi = bf16_bits(h);
    mid = bf16_bits(m);
    lo = bf16_bits(r2);
}

// x -> (h, l') fp16 bit patterns with h + l' * 2^-11 == x up to 2^-22 |x|
__device__ __forceinline__ void split2(float x, unsigned short &hi, unsigned short &lo)
{
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)((x - (float)h) * 2048.0f);
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
}
__device__ __forceinline__ float f16lo(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu)); }
__device__ __forceinline__ float f16hi(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }

// eight consecutive channels: fp32 -> NPL packed planes (o[plane] = 8 x 16-bit)
template <int NPL>
__device__ __forceinline__ void split_planes(const float (&v)[8], u32x4 (&o)[NPL])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (NPL == 3) {
            unsigned short h0, m0_, l0, h1, m1, l1;
            split3(v[2 * k], h0, m0_, l0);
            split3(v[2 * k + 1], h1, m1, l1);
            o[0][k] = (unsigned)h0 | ((unsigned)h1 << 16);
            o[1][k] = (unsigned)m0_ | ((unsigned)m1 << 16);
            o[NPL - 1][k] = (unsigned)l0 | ((unsigned)l1 << 16);
        } else {
            unsigned short h0, l0, h1, l1;
            split2(v[2 * k], h0, l0);
            split2(v[2 * k + 1], h1, l1);
            o[0][k] = (unsigned)h0 | ((unsigned)h1 << 16);
            o[1][k] = (unsigned)l0 | ((unsigned)l1 << 16);
        }
    }
}

// packed planes of two adjacent channels -> their fp32 values
template <int NPL>
__device__ __forceinline__ void join_planes(const u32x4 (&q)[NPL], int k, float &a0, float &a1)
{
    if (NPL == 3) {
        a0 = (__uint_as_float(q[0][k] << 16) + __uint_as_float(q[1][k] << 16)) + __uint_as_float(q[NPL - 1][k] << 16);
        a1 = (__uint_as_float(q[0][k] & 0xffff0000u) + __uint_as_float(q[1][k] & 0xffff0000u)) +
             __uint_as_float(q[NPL - 1][k] & 0xffff0000u);
    } else {
        a0 = f16lo(q[0][k]) + f16lo(q[1][k]) * (1.0f / 2048.0f);
        a1 = f16hi(q[0][k]) + f16hi(q[1][k]) * (1.0f / 2048.0f);
    }
}

}  // namespace y3
