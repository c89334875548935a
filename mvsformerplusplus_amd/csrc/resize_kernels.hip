// The glue of the network's eval forward (DINOv2_mvsformer_model.py:72-88):
//   mvs_resize_bicubic_fwd        images [N,3,H,W] -> [N,3,h,w], the ViT's input: F.interpolate(mode="bicubic", align_corners=False), no antialias
//   mvs_resize_bilinear_add_fwd   base [N,C,h,w] + F.interpolate(x [N,C,h',w'], (h, w), mode="bilinear", align_corners=False): conv31 + vit_feat
//
// Both are memory-bound maps with no reuse worth staging.  A wave owns consecutive output pixels of one row, a workgroup four rows; the taps
// are plain loads through the source's strides (when scaling down they skip pixels, so there is nothing to vectorise on that side).  The
// bicubic kernel takes one output pixel per work-item and loops over the channels (see there); the add takes four consecutive pixels (one
// 16-byte load of `base`, one 16-byte store) with the row coefficients computed once.  The arithmetic is ATen's upsample kernels': source
// coordinate (dst + 0.5) * (in / out) - 0.5 (bilinear: clamped at 0), cubic convolution with A = -0.75, every tap index clamped to the image,
// rows interpolated along x first and then along y, fp32 accumulation.  One difference, on purpose: the coordinate is the exact rational
// ((2 dst + 1) in - out) / (2 out), split into its floor and a once-rounded fraction with integers.  ATen's fp32 form rounds the coordinate
// itself, an absolute error of 2^-24 x the coordinate that the image's slope multiplies: 1.5e-4 on unit noise at 320 -> 140 columns against
// fp64, where this form stays at 1e-6.
#include "mvs_common.h"

namespace mvs {

constexpr int RS_PX = 4;                   // output pixels per work-item of the add kernels
constexpr int RS_ROWS = kBlock / kWave;    // output rows per workgroup (one wave each)
constexpr int RS_TILE_W = kWave * RS_PX;   // output pixels of a row per workgroup of the bilinear-add kernel

struct ResizeArgs {
    const float* src;
    long long sn, sc, sy, sx;   // element strides of src [N, C, H, W]
    const float* base;          // bilinear-add only: contiguous [N, C, h, w]
    float* dst;                 // contiguous [N, C, h, w]
    int C, H, W, h, w;
};

// source coordinate of output index d on an axis resized from `in` to `out`: floor and fraction of ((2 d + 1) in - out) / (2 out)
__device__ __forceinline__ void source_coordinate(int d, int in, int out, int& fl, float& frac) {
    const int num = (2 * d + 1) * in - out, den = 2 * out;          // |num| < 2^31: in, out <= 32768
    fl = num >= 0 ? num / den : -((den - 1 - num) / den);
    frac = (float)(num - fl * den) / (float)den;
}

// cubic convolution coefficients of the four taps around a point at fraction t past tap 1 (ATen get_cubic_upsample_coefficients)
__device__ __forceinline__ void cubic_coefficients(float t, float c[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool VEC>
__device__ __forceinline__ void store_px(float* p, const float v[RS_PX], int n) {
    if (VEC) {                             // w % 4 == 0 and a 16-byte aligned base: the four pixels are in range and aligned
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int i = 0; i < n; ++i) p[i] = v[i];
    }
}

// One work-item = one output pixel of every channel: the 64 lanes of a wave read source columns in/out apart (2.3 floats at the product's
// scale), so one tap load of a wave touches a handful of cache lines; with four pixels per work-item the lanes sit 9 floats apart, every
// lane in a line of its own, and that form traced at 82 us against ATen's 61 us at the product's sizes (V = 5); this one at 53 us.  The
// stores stay coalesced (256 contiguous bytes per wave).  The coefficients and tap offsets are computed once and serve the C channels.
__global__ __launch_bounds__(kBlock) void resize_bicubic_kernel(ResizeArgs a) {
    const int x = (int)blockIdx.x * kWave + ((int)threadIdx.x & (kWave - 1));
    const int y = (int)blockIdx.y * RS_ROWS + ((int)threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const int n = (int)blockIdx.z;

    int iy, ix;
    float ty, tx, cy[4], cx[4];
    source_coordinate(y, a.H, a.h, iy, ty);
    source_coordinate(x, a.W, a.w, ix, tx);
    cubic_coefficients(ty, cy);
    cubic_coefficients(tx, cx);
    long long row[4], col[4];
    for (int j = 0; j < 4; ++j) row[j] = (long long)clampi(iy - 1 + j, a.H - 1) * a.sy;
    for (int i = 0; i < 4; ++i) col[i] = (long long)clampi(ix - 1 + i, a.W - 1) * a.sx;

    for (int c = 0; c < a.C; ++c) {
        const float* src = a.src + n * a.sn + c * a.sc;
        float acc = 0.0f;
        for (int j = 0; j < 4; ++j) {
            const float* r = src + row[j];
            const float v = r[col[0]] * cx[0] + r[col[1]] * cx[1] + r[col[2]] * cx[2] + r[col[3]] * cx[3];
            acc += v * cy[j];
        }
        a.dst[(((long long)n * a.C + c) * a.h + y) * a.w + x] = acc;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void resize_bilinear_add_kernel(ResizeArgs a) {
    const int x0 = ((int)blockIdx.x * kWave + ((int)threadIdx.x & (kWave - 1))) * RS_PX;
    const int y = (int)blockIdx.y * RS_ROWS + ((int)threadIdx.x >> 6);
    if (x0 >= a.w || y >= a.h) return;
    const int plane = (int)blockIdx.z, n = plane / a.C, c = plane - n * a.C;
    const float* src = a.src + n * a.sn + c * a.sc;

    int y0;
    float ly1;
    source_coordinate(y, a.H, a.h, y0, ly1);
    if (y0 < 0) { y0 = 0; ly1 = 0.0f; }                              // the coordinate clamped at 0
    const float ly0 = 1.0f - ly1;
    const float* r0 = src + (long long)y0 * a.sy;
    const float* r1 = src + (long long)(y0 < a.H - 1 ? y0 + 1 : y0) * a.sy;

    const int npx = a.w - x0 < RS_PX ? a.w - x0 : RS_PX;
    const long long o = ((long long)plane * a.h + y) * a.w + x0;
    float b[RS_PX] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(a.base + o);
        b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
    } else {
        for (int p = 0; p < npx; ++p) b[p] = a.base[o + p];
    }
    float out[RS_PX];
    for (int p = 0; p < RS_PX; ++p) {
        out[p] = 0.0f;
        if (p >= npx) continue;
        int xa;
        float lx1;
        source_coordinate(x0 + p, a.W, a.w, xa, lx1);
        if (xa < 0) { xa = 0; lx1 = 0.0f; }
        const float lx0 = 1.0f - lx1;
        const long long ca = (long long)xa * a.sx, cb = (long long)(xa < a.W - 1 ? xa + 1 : xa) * a.sx;
        out[p] = b[p] + (ly0 * (lx0 * r0[ca] + lx1 * r0[cb]) + ly1 * (lx0 * r1[ca] + lx1 * r1[cb]));
    }
    store_px<VEC>(a.dst + o, out, npx);
}

// the same size on both sides: the resize is the identity and the result is base + x exactly (no 0 * x terms)
template <bool VEC>
__global__ __launch_bounds__(kBlock) void add_kernel(const float* base, const float* x, float* out, long long count) {
    const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) * RS_PX;
    if (i >= count) return;
    if (VEC && i + RS_PX <= count) {
        const float4 p = *reinterpret_cast<const float4*>(base + i), q = *reinterpret_cast<const float4*>(x + i);
        *reinterpret_cast<float4*>(out + i) = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
    } else {
        for (long long j = i; j < count && j < i + RS_PX; ++j) out[j] = base[j] + x[j];
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// sizes the launch geometry holds: N * C planes in grid.z, h / 4 row groups in grid.y; offsets are 64-bit throughout
static bool resize_dims_ok(int N, int C, int H, int W, int h, int w) {
    const int side = 32768;                // source_coordinate's 32-bit numerator
    return N >= 1 && C >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && H <= side && W <= side && h <= side && w <= side &&
           (long long)N * C <= 65535;
}

}  // namespace mvs

using namespace mvs;

extern "C" int mvs_resize_bicubic_fwd(const float* img, long long batch_stride, long long channel_stride, long long row_stride,
                                      long long col_stride, float* out, int N, int C, int H, int W, int h, int w, void* stream) {
    if (!img || !out || !resize_dims_ok(N, C, H, W, h, w) || batch_stride < 0 || channel_stride < 0 || row_stride < 0 || col_stride < 0) {
        set_error("mvs_resize_bicubic_fwd: bad arguments (1 <= sizes <= 32768, N * C <= 65535, strides >= 0)");
        return MVS_ERR_ARG;
    }
    ResizeArgs a{img, batch_stride, channel_stride, row_stride, col_stride, nullptr, out, C, H, W, h, w};
    const dim3 grid(ceil_div(w, kWave), ceil_div(h, RS_ROWS), N);
    hipLaunchKernelGGL(resize_bicubic_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("resize_bicubic_kernel");
}

extern "C" int mvs_resize_bilinear_add_fwd(const float* base, const float* x, long long batch_stride, long long channel_stride,
                                           long long row_stride, long long col_stride, float* out, int N, int C, int h, int w, int xh, int xw,
                                           void* stream) {
    if (!base || !x || !out || !resize_dims_ok(N, C, xh, xw, h, w) || batch_stride < 0 || channel_stride < 0 || row_stride < 0 || col_stride < 0) {
        set_error("mvs_resize_bilinear_add_fwd: bad arguments (1 <= sizes <= 32768, N * C <= 65535, strides >= 0)");
        return MVS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = aligned16(base) && aligned16(out);
    const bool x_dense = col_stride == 1 && row_stride == xw && channel_stride == (long long)xh * xw && batch_stride == (long long)C * xh * xw;
    if (xh == h && xw == w && x_dense) {
        const long long count = (long long)N * C * h * w;
        const dim3 grid(ceil_div(count, (long long)kBlock * RS_PX));
        if (vec && aligned16(x)) hipLaunchKernelGGL((add_kernel<true>), grid, dim3(kBlock), 0, st, base, x, out, count);
        else hipLaunchKernelGGL((add_kernel<false>), grid, dim3(kBlock), 0, st, base, x, out, count);
        return check_launch("add_kernel");
    }
    ResizeArgs a{x, batch_stride, channel_stride, row_stride, col_stride, base, out, C, xh, xw, h, w};
    const dim3 grid(ceil_div(w, RS_TILE_W), ceil_div(h, RS_ROWS), N * C);
    if ((w % RS_PX) == 0 && vec) hipLaunchKernelGGL((resize_bilinear_add_kernel<true>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((resize_bilinear_add_kernel<false>), grid, dim3(kBlock), 0, st, a);
    return check_launch("resize_bilinear_add_kernel");
}
