// MaxPooling2D(2, strides = 1 | 2, 'same') on NHWC tensors (reference: core/parse_model.py:78-99; include/y3.h, y3_maxpool2x2): the
// pools of YOLOv3-tiny, an op of their own between two conv launches.  HBM-bound: every lane moves 16-byte vectors of channels, lanes
// run along the channels and then along the output row, so a wave's stores are one contiguous run and its loads two (the two input rows).
// out[y, x] = max(in[y0 .. min(y0 + 1, H - 1), x0 .. min(x0 + 1, W - 1)]), (y0, x0) = (y, x) * stride: the clamps are the whole border
// rule ('same' padding never wins a max), there is no running maximum with a start value.  Elements are compared as values and the
// winner's bits are stored; a NaN in a window and the sign of a zero result are unspecified.  An int8 plan's pools behind its cut run the
// same body on 16 signed bytes per vector (Y3_DTYPE_I8): every byte value is legal, -128 included.
#include "../../include/y3.h"
#include "y3_device.h"
#include "y3_kernels.h"

namespace y3 {

typedef short s16x2 __attribute__((ext_vector_type(2)));

// the larger of two elements of format FMT held in 32-bit words: one fp32, two bf16 / fp16 (each half on its own), or four signed bytes
// (each on its own: a byte in the high half of a 16-bit lane, the low half zero, orders as the byte does -- v_pk_max_i16 on the odd bytes,
// and on the even bytes moved up by eight bits)
template <int FMT>
__device__ __forceinline__ unsigned max_word(unsigned a, unsigned b)
{
    if constexpr (FMT == Y3_DTYPE_F32) {
        return __uint_as_float(b) > __uint_as_float(a) ? b : a;
    } else if constexpr (FMT == Y3_DTYPE_I8) {
        constexpr unsigned odd = 0xff00ff00u;
        auto pk_max = [](unsigned u, unsigned v) {
            return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, u), __builtin_bit_cast(s16x2, v)));
        };
        return pk_max(a & odd, b & odd) | (pk_max((a << 8) & odd, (b << 8) & odd) >> 8);
    } else {
        float alo, ahi, blo, bhi;
        if constexpr (FMT == Y3_DTYPE_BF16) {
            alo = __uint_as_float(a << 16), ahi = __uint_as_float(a & 0xffff0000u);
            blo = __uint_as_float(b << 16), bhi = __uint_as_float(b & 0xffff0000u);
        } else {
            alo = (float)__builtin_bit_cast(_Float16, (unsigned short)(a & 0xffffu)), ahi = (float)__builtin_bit_cast(_Float16, (unsigned short)(a >> 16));
            blo = (float)__builtin_bit_cast(_Float16, (unsigned short)(b & 0xffffu)), bhi = (float)__builtin_bit_cast(_Float16, (unsigned short)(b >> 16));
        }
        return ((blo > alo ? b : a) & 0xffffu) | ((bhi > ahi ? b : a) & 0xffff0000u);
    }
}

template <int FMT>
__device__ __forceinline__ u32x4 max_vec(const u32x4 &a, const u32x4 &b)
{
    return u32x4{max_word<FMT>(a[0], b[0]), max_word<FMT>(a[1], b[1]), max_word<FMT>(a[2], b[2]), max_word<FMT>(a[3], b[3])};
}

// x [B,H,W,V] and y [B,Ho,Wo,V] in 16-byte vectors, V per pixel.  A workgroup owns `rpb` consecutive output rows of the B * Ho there
// are (several where a row is short); its lanes walk them vector by vector.  Offsets are size_t: tensors reach 4 GiB.
template <int FMT, int STRIDE>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const u32x4 *__restrict__ x, u32x4 *__restrict__ y, int rows_out, int H, int W,
                                                         int V, int rpb)
{
    const int Ho = H / STRIDE, Wo = W / STRIDE;
    const unsigned row_len = (unsigned)Wo * (unsigned)V;
    for (long long r0 = (long long)blockIdx.x * rpb; r0 < rows_out; r0 += (long long)gridDim.x * rpb) {
        const int nr = rows_out - r0 < rpb ? (int)(rows_out - r0) : rpb;
        for (unsigned j = threadIdx.x; j < (unsigned)nr * row_len; j += 256) {
            const unsigned rr = j / row_len, jj = j - rr * row_len;
            const unsigned xo = jj / (unsigned)V, v = jj - xo * (unsigned)V;
            const unsigned r = (unsigned)r0 + rr;     // output row over the batch, b * Ho + yo (rows_out fits an int)
            const unsigned b = r / (unsigned)Ho;
            const int yo = (int)(r - b * (unsigned)Ho);
            const int y0 = yo * STRIDE, x0 = (int)xo * STRIDE;
            const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
            const size_t img = (size_t)b * H;
            const size_t top = (img + y0) * W, bot = (img + y1) * W;
            const u32x4 a = x[(top + x0) * V + v], c = x[(top + x1) * V + v];
            const u32x4 d = x[(bot + x0) * V + v], e = x[(bot + x1) * V + v];
            y[(size_t)r * row_len + jj] = max_vec<FMT>(max_vec<FMT>(a, c), max_vec<FMT>(d, e));
        }
    }
}

template <int FMT>
static hipError_t launch_fmt(const void *src, void *dst, int B, int H, int W, int V, int stride, hipStream_t s)
{
    const int Ho = H / stride, Wo = W / stride;
    const long long rows_out = (long long)B * Ho, row_len = (long long)Wo * V;
    if (rows_out > 0x7fffffffll || row_len > 0x00ffffffll) return hipErrorInvalidValue;
    // about 1024 vectors (four per lane) per workgroup where rows are short; never more than 256 rows (rr * row_len stays in 32 bits)
    long long rpb = row_len >= 1024 ? 1 : 1024 / row_len;
    if (rpb > 256) rpb = 256;
    const long long blocks = (rows_out + rpb - 1) / rpb;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    const u32x4 *x = static_cast<const u32x4 *>(src);
    u32x4 *y = static_cast<u32x4 *>(dst);
    if (stride == 2) hipLaunchKernelGGL((maxpool2x2_kernel<FMT, 2>), grid, block, 0, s, x, y, (int)rows_out, H, W, V, (int)rpb);
    else hipLaunchKernelGGL((maxpool2x2_kernel<FMT, 1>), grid, block, 0, s, x, y, (int)rows_out, H, W, V, (int)rpb);
    return hipGetLastError();
}

// dtype: Y3_DTYPE_F32, _BF16, _F16 or _I8 (the element format); C * element size a multiple of 16 bytes, both pointers 16-byte aligned;
// stride 2 on even H and W.  Only enqueues.
hipError_t launch_maxpool2x2(const void *src, void *dst, int B, int H, int W, int C, int stride, int dtype, hipStream_t s)
{
    const int eb = dtype == Y3_DTYPE_F32 ? 4 : dtype == Y3_DTYPE_I8 ? 1 : 2;
    if (B < 1 || H < 1 || W < 1 || C < 1 || (stride != 1 && stride != 2) || (stride == 2 && ((H | W) & 1)) || ((long long)C * eb) % 16 ||
        ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
        return hipErrorInvalidValue;
    const int V = C * eb / 16;
    switch (dtype) {
        case Y3_DTYPE_F32: return launch_fmt<Y3_DTYPE_F32>(src, dst, B, H, W, V, stride, s);
        case Y3_DTYPE_BF16: return launch_fmt<Y3_DTYPE_BF16>(src, dst, B, H, W, V, stride, s);
        case Y3_DTYPE_F16: return launch_fmt<Y3_DTYPE_F16>(src, dst, B, H, W, V, stride, s);
        case Y3_DTYPE_I8: return launch_fmt<Y3_DTYPE_I8>(src, dst, B, H, W, V, stride, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace y3
