// FPNDecoder in train mode, forward and backward.
//
// Reference (restated, never copied): models/module.py:236-270 - out_k = Swish(BatchNorm2d(Conv2d(64, C_k, 3 | 1)(intra_k))) with batch
// statistics over all N H W samples of a channel, intra_k = up2(intra_{k-1}) + inner_k(lateral_k).
//
// The forward convolutions are the inference kernels on un-folded weights (fpn_kernels.hip); this file adds what training needs:
//   1. planar batch-statistics BatchNorm + Swish: fpn_bn_reduce_kernel (per-channel [sum z | sum z^2], or [sum du | sum du xhat] in the
//      backward, accumulated in fp64 and left as one partial per workgroup), fpn_bn_finalize_kernel (adds the partials front to back;
//      mean / biased variance / invstd and the running-statistics step, or d beta / d gamma) and fpn_bn_apply_kernel
//      (y = swish(gamma xhat + beta), or dz = gamma invstd (du - d beta / M - xhat d gamma / M));
//   2. data gradients: further instances of conv2d_split_kernel (flipped, channel-transposed taps packed by the caller), list
//      MVS_FPN_TRAIN_CONVS;
//   3. weight gradients: fpn_wgrad_kernel, dW[co][ci][ky][kx] = sum_pixels dY[co] X[ci] shifted by the tap as a GEMM on the exact-fp32
//      v_mfma_f32_16x16x4_f32 (the C_out x C_in form of fmt_smooth_wgrad_kernel).  X comes through a convolution source: a stored map
//      (PlanarSrc) or, at the last level, MergeSrc<8> - the 64-channel full-resolution intra_3 is re-evaluated in the staging and never
//      written.  ONES appends an input channel that is 1 inside the image: its column is the gradient of a bias behind the taps;
//   4. fpn_up2_adjoint_kernel: the adjoint of the x2 align_corners=True upsample as a gather, one thread per coarse pixel over the
//      fine pixels whose taps name it, with up2_axis - the function MergeSrc::at evaluates - deciding the weights.
// Per-workgroup partials are added in a fixed order (partial_reduce.h); there is no atomic anywhere, so gradients are the same bits
// from run to run.  Staged positions are clamped to the image explicitly.
#include "fpn_merge.h"
#include "partial_reduce.h"

namespace mvs {

// ---------------------------------------------------------------------------------------------------------------------------------
// BatchNorm (batch statistics) + Swish on planar fp32 [N, C, H, W]
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int FB_MAX_PARTS = 64;              // partials per channel: the finalize adds them one after the other
constexpr int FB_CHUNK = 1024;                // elements of one plane per workgroup of the apply kernel

__device__ __forceinline__ float fb_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }

// stats = [mean | biased variance | invstd], [3][C]
template <int MODE>
__global__ __launch_bounds__(256) void fpn_bn_reduce_kernel(const float* __restrict__ z, const float* __restrict__ dy, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, double* __restrict__ part,
                                                            int N, int C, int HW, int P) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    double* sh = reinterpret_cast<double*>(lds4);                 // [2][256]
    const int tid = (int)threadIdx.x, p = (int)blockIdx.x, c = (int)blockIdx.y;
    float mean = 0.0f, invstd = 0.0f, g = 0.0f, b = 0.0f;
    if (MODE == 1) { mean = stats[c]; invstd = stats[2 * C + c]; g = gamma[c]; b = beta[c]; }
    double s0 = 0.0, s1 = 0.0;
    for (int n = 0; n < N; ++n) {
        const size_t base = ((size_t)n * C + c) * HW;
        for (int i = p * 256 + tid; i < HW; i += P * 256) {
            const float v = z[base + i];
            if (MODE == 0) {
                s0 += (double)v;
                s1 += (double)v * (double)v;
            } else {
                const float xh = (v - mean) * invstd, u = xh * g + b, s = fb_sigmoid(u);
                const float du = dy[base + i] * (s + u * s * (1.0f - s));
                s0 += (double)du;
                s1 += (double)du * (double)xh;
            }
        }
    }
    sh[tid] = s0;
    sh[256 + tid] = s1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { sh[tid] += sh[tid + s]; sh[256 + tid] += sh[256 + tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        part[((size_t)c * P + p) * 2] = sh[0];
        part[((size_t)c * P + p) * 2 + 1] = sh[256];
    }
}

// MODE 0: stats from the sums; running_mean / running_var (nullable) take one momentum step with mean + conv_bias and the unbiased
// variance.  MODE 1: out0 = d beta, out1 = d gamma.  sums [2][C] (doubles) keeps the totals for the apply kernel.
template <int MODE>
__global__ __launch_bounds__(64) void fpn_bn_finalize_kernel(const double* __restrict__ part, double* __restrict__ sums, float* __restrict__ out0,
                                                             float* __restrict__ out1, const float* __restrict__ conv_bias, float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, double count, float eps, float momentum, int C, int P) {
    const int c = (int)threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int p = 0; p < P; ++p) {
        s0 += part[((size_t)c * P + p) * 2];
        s1 += part[((size_t)c * P + p) * 2 + 1];
    }
    sums[c] = s0;
    sums[C + c] = s1;
    if (MODE == 1) {
        out0[c] = (float)s0;
        out1[c] = (float)s1;
        return;
    }
    const double mean = s0 / count, m2 = s1 / count - mean * mean, var = m2 > 0.0 ? m2 : 0.0;
    out0[c] = (float)mean;
    out0[C + c] = (float)var;
    out0[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double m = (double)momentum, unbiased = var * (count / (count > 1.0 ? count - 1.0 : 1.0));
        running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * (mean + (conv_bias ? (double)conv_bias[c] : 0.0)));
        running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * unbiased);
    }
}

// MODE 0: out = swish(gamma xhat + beta).  MODE 1: out = dz = gamma invstd (du - sum du / M - xhat sum du xhat / M).
template <int MODE>
__global__ __launch_bounds__(256) void fpn_bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ dy, const float* __restrict__ stats,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, const double* __restrict__ sums,
                                                           float* __restrict__ out, double count, int C, int HW) {
    const int plane = (int)blockIdx.x, c = plane % C;
    const float mean = stats[c], invstd = stats[2 * C + c], g = gamma[c], b = beta[c];
    float k0 = 0.0f, k1 = 0.0f;
    if (MODE == 1) { k0 = (float)(sums[c] / count); k1 = (float)(sums[C + c] / count); }
    const size_t base = (size_t)plane * HW;
    const int i0 = (int)blockIdx.y * FB_CHUNK, i1 = i0 + FB_CHUNK < HW ? i0 + FB_CHUNK : HW;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) {
        const float xh = (z[base + i] - mean) * invstd, u = xh * g + b, s = fb_sigmoid(u);
        if (MODE == 0) {
            out[base + i] = u * s;
        } else {
            const float du = dy[base + i] * (s + u * s * (1.0f - s));
            out[base + i] = g * invstd * (du - k0 - xh * k1);
        }
    }
}

static int fb_parts(int HW) {
    const int p = (int)ceil_div(HW, 256);
    return p < FB_MAX_PARTS ? p : FB_MAX_PARTS;
}

static bool fb_args(const char* what, int N, int C, int H, int W) {
    if (N < 1 || N > 65535 || C < 1 || C > 64 || H < 1 || W < 1 || (long long)H * W > 0x3fffffffLL || (long long)N * C > 0x7fffffffLL ||
        ceil_div((long long)H * W, FB_CHUNK) > 65535u) {
        set_error("%s: bad arguments (1 <= C <= 64, H W <= 65535 x 1024)", what);
        return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradients on v_mfma_f32_16x16x4_f32
// ---------------------------------------------------------------------------------------------------------------------------------
// rows = co (16 per row block), columns = (ci, tap) = the weights of one output channel in memory order, K = the pixels of a TH x 64
// tile.  The source's tile and halo are staged into LDS (zero outside the image).  Wave v owns the column blocks v, v + 4, ..: its
// accumulators are final for the workgroup, which keeps them over all of its tiles and writes one partial.
template <int COUT, int CIN, int K, bool ONES>
struct FpnWgradShape {
    static constexpr int P = K / 2, TH = COUT >= 32 ? 2 : 4, TW = 64, NPIX = TH * TW;
    static constexpr int CT = CIN + (ONES ? 1 : 0);                   // staged planes: the input channels (+ the plane of ones)
    static constexpr int RS = TW + 4, PL = (TH + 2 * P) * RS + 1;     // staged row / channel-plane strides of X
    static constexpr int DSS = NPIX + 4;                              // channel stride of the staged dY: lane (co, k) reads bank 4 co + k
    static constexpr int NRB = (COUT + 15) / 16, NCOL = CT * K * K, NCB = (NCOL + 15) / 16, NCBW = (NCB + 3) / 4;
    static constexpr int LDS = (CT * PL + COUT * DSS) * (int)sizeof(float);
    static_assert(CIN % 8 == 0 && LDS <= 160 * 1024, "input channels come in octets; the tile must fit the LDS");
};

constexpr long long FW_PART_BYTES = 8 << 20;  // partials of one launch: at most this much workspace ..
constexpr int FW_MAX_PARTS = 256;             // .. and at most this many (= workgroups)

template <int COUT, int CIN, int K, bool ONES>
static int fw_parts(long long ntile) {
    typedef FpnWgradShape<COUT, CIN, K, ONES> F;
    long long cap = FW_PART_BYTES / ((long long)COUT * F::NCOL * (long long)sizeof(float));
    cap = cap < FW_MAX_PARTS ? cap : FW_MAX_PARTS;
    return (int)(ntile < cap ? ntile : cap);
}

template <int COUT, int CIN, int K, bool ONES>
static long long fw_tiles(int N, int H, int W) {
    typedef FpnWgradShape<COUT, CIN, K, ONES> F;
    return (long long)N * ceil_div(H, F::TH) * ceil_div(W, F::TW);
}

template <int COUT, int CIN, int K, bool ONES, class Src>
__global__ __launch_bounds__(256) void fpn_wgrad_kernel(Src src, const float* __restrict__ dy, float* __restrict__ part, int H, int W, int tiles_x,
                                                        int tiles_per_view, int ntile) {
    typedef FpnWgradShape<COUT, CIN, K, ONES> F;
    constexpr int P = F::P, SH = F::TH + 2 * P, SW = F::TW + 2 * P;
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* ms = reinterpret_cast<float*>(lds4);                   // [CT][TH + 2P][RS]
    float* ds = ms + F::CT * F::PL;                               // [COUT][DSS]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    int off[F::NCBW];                                             // this lane's column (ci, ky, kx) in the staged tile, -1 past the end
#pragma unroll
    for (int t = 0; t < F::NCBW; ++t) {
        const int col = (wave + 4 * t) * 16 + li, ci = col / (K * K), tap = col % (K * K);
        off[t] = col < F::NCOL ? ci * F::PL + (tap / K) * F::RS + tap % K : -1;
    }
    f32x4 acc[F::NRB][F::NCBW];
#pragma unroll
    for (int rb = 0; rb < F::NRB; ++rb)
#pragma unroll
        for (int t = 0; t < F::NCBW; ++t) acc[rb][t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < ntile; tile += (int)gridDim.x) {
        const int n = tile / tiles_per_view, tv = tile % tiles_per_view;
        const int y0 = (tv / tiles_x) * F::TH, x0 = (tv % tiles_x) * F::TW;
        __syncthreads();                                          // the previous tile's readers are done
#pragma unroll 1
        for (int pos = tid; pos < SH * SW; pos += 256) {
            const int py = pos / SW, px = pos % SW, gy = y0 - P + py, gx = x0 - P + px;
            float* m = ms + py * F::RS + px;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            if (inside) {
                Src s = src;
                s.at(n, gy, gx);
#pragma unroll 1
                for (int c0 = 0; c0 < CIN; c0 += 8) {
                    float v[8];
                    s.load8(c0, v);
#pragma unroll
                    for (int k = 0; k < 8; ++k) m[(c0 + k) * F::PL] = v[k];
                }
            } else {
#pragma unroll 8
                for (int c = 0; c < CIN; ++c) m[c * F::PL] = 0.0f;
            }
            if (ONES) m[CIN * F::PL] = inside ? 1.0f : 0.0f;
        }
#pragma unroll 1
        for (int e = tid; e < COUT * F::NPIX; e += 256) {
            const int c = e / F::NPIX, pix = e % F::NPIX, gy = y0 + pix / F::TW, gx = x0 + pix % F::TW;
            ds[c * F::DSS + pix] = gy < H && gx < W ? dy[(((size_t)n * COUT + c) * H + gy) * W + gx] : 0.0f;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < F::NPIX / 4; ++q) {
            const int pix = 4 * q + g, at = (pix / F::TW) * F::RS + pix % F::TW;
            float a[F::NRB];
#pragma unroll
            for (int rb = 0; rb < F::NRB; ++rb) a[rb] = rb * 16 + li < COUT ? ds[(rb * 16 + li) * F::DSS + pix] : 0.0f;
#pragma unroll
            for (int t = 0; t < F::NCBW; ++t) {
                if (wave + 4 * t >= F::NCB) continue;             // wave-uniform
                const float b = off[t] >= 0 ? ms[off[t] + at] : 0.0f;
#pragma unroll
                for (int rb = 0; rb < F::NRB; ++rb) acc[rb][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], b, acc[rb][t], 0, 0, 0);
            }
        }
    }
    // lane (li, g) holds rows 16 rb + 4 g + r of column 16 cb + li
    float* dst = part + (size_t)blockIdx.x * COUT * F::NCOL;
#pragma unroll
    for (int t = 0; t < F::NCBW; ++t) {
        const int col = (wave + 4 * t) * 16 + li;
        if (col >= F::NCOL) continue;
#pragma unroll
        for (int rb = 0; rb < F::NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = rb * 16 + 4 * g + r;
                if (co < COUT) dst[co * F::NCOL + col] = acc[rb][t][r];
            }
    }
}

template <int COUT, int CIN, int K, bool ONES, class Src>
static int launch_fpn_wgrad(const Src& src, const float* dy, float* dw, float* part, int N, int H, int W, hipStream_t st) {
    typedef FpnWgradShape<COUT, CIN, K, ONES> F;
    const int tiles_x = (int)ceil_div(W, F::TW), tpv = tiles_x * (int)ceil_div(H, F::TH), ntile = N * tpv;
    const int parts = fw_parts<COUT, CIN, K, ONES>(ntile);
    if (F::LDS > 48 * 1024)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fpn_wgrad_kernel<COUT, CIN, K, ONES, Src>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
    hipLaunchKernelGGL((fpn_wgrad_kernel<COUT, CIN, K, ONES, Src>), dim3(parts), dim3(256), F::LDS, st, src, dy, part, H, W, tiles_x, tpv, ntile);
    const int rc = check_launch("fpn_wgrad_kernel");
    return rc != MVS_OK ? rc : ft_reduce_partials(part, dw, parts, COUT * F::NCOL, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// adjoint of up2 (bilinear x2, align_corners=True)
// ---------------------------------------------------------------------------------------------------------------------------------
// weight with which coarse index c enters fine index gi's two taps (both, where they collapse onto the last entry)
__device__ __forceinline__ float up2_tap_weight(int gi, float s, int n, int c) {
    int i0, step;
    float l;
    up2_axis(gi, s, n, i0, step, l);
    return (i0 == c ? 1.0f - l : 0.0f) + (i0 + step == c ? l : 0.0f);
}

// fine indices that can name coarse index c: those whose source coordinate s gi lies within (c - 1, c + 1), one more on either side
// for the rounding of this estimate (up2_tap_weight decides); s = 0 (a coarse axis of one entry): all of them
__device__ __forceinline__ void up2_fine_range(int c, float s, int N, int& lo, int& hi) {
    lo = 0;
    hi = N - 1;
    if (s > 0.0f) {
        const float inv = 1.0f / s;
        const int a = (int)floorf(((float)c - 1.0f) * inv) - 1, b = (int)ceilf(((float)c + 1.0f) * inv) + 1;
        lo = a > 0 ? a : 0;
        hi = b < N - 1 ? b : N - 1;
    }
}

constexpr int UA_CH = 16;

// One thread per coarse pixel, all 64 channels: out[c] = sum over the fine pixels whose taps name it of weight x d[c].
__global__ __launch_bounds__(256) void fpn_up2_adjoint_kernel(const float* __restrict__ d, float* __restrict__ out, int H, int W, int h, int w, float sy,
                                                              float sx) {
    const int cx = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), cy = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), n = (int)blockIdx.z;
    if (cx >= w || cy >= h) return;
    const size_t HW = (size_t)H * W, hw = (size_t)h * w;
    int ylo, yhi, xlo, xhi;
    up2_fine_range(cy, sy, H, ylo, yhi);
    up2_fine_range(cx, sx, W, xlo, xhi);
    const float* dn = d + (size_t)n * 64 * HW;
    float* o = out + (size_t)n * 64 * hw + (size_t)cy * w + cx;
#pragma unroll 1
    for (int c0 = 0; c0 < 64; c0 += UA_CH) {                       // UA_CH channels at a time: the accumulators stay in few registers
        float acc[UA_CH];
#pragma unroll
        for (int c = 0; c < UA_CH; ++c) acc[c] = 0.0f;
#pragma unroll 1
        for (int gy = ylo; gy <= yhi; ++gy) {
            const float wy = up2_tap_weight(gy, sy, h, cy);
            if (wy == 0.0f) continue;
#pragma unroll 1
            for (int gx = xlo; gx <= xhi; ++gx) {
                const float wgt = wy * up2_tap_weight(gx, sx, w, cx);
                if (wgt == 0.0f) continue;
                const float* q = dn + (size_t)c0 * HW + (size_t)gy * W + gx;
#pragma unroll
                for (int c = 0; c < UA_CH; ++c) acc[c] = fmaf(wgt, q[(size_t)c * HW], acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < UA_CH; ++c) o[(size_t)(c0 + c) * hw] = acc[c];
    }
}

}  // namespace mvs

using namespace mvs;

// ---- BatchNorm + Swish ----
extern "C" size_t mvs_fpn_bn_workspace_bytes(int N, int C, int H, int W) {
    if (N < 1 || N > 65535 || C < 1 || C > 64 || H < 1 || W < 1 || (long long)H * W > 0x3fffffffLL) return 0;
    return ((size_t)C * fb_parts(H * W) * 2 + 2 * (size_t)C) * sizeof(double);
}

extern "C" int mvs_fpn_bn_swish_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, float* stats, float* y, void* workspace, size_t workspace_bytes, int N,
                                    int C, int H, int W, void* stream) {
    if (!fb_args("mvs_fpn_bn_swish_fwd", N, C, H, W)) return MVS_ERR_ARG;
    if (!z || !gamma || !beta || !stats || !y || !workspace || (running_mean == nullptr) != (running_var == nullptr)) {
        set_error("mvs_fpn_bn_swish_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_fpn_bn_workspace_bytes(N, C, H, W)) { set_error("mvs_fpn_bn_swish_fwd: workspace smaller than mvs_fpn_bn_workspace_bytes"); return MVS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, P = fb_parts(HW);
    const double count = (double)N * (double)HW;
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = part + (size_t)C * P * 2;
    hipLaunchKernelGGL(fpn_bn_reduce_kernel<0>, dim3(P, C), dim3(256), 512 * sizeof(double), st, z, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, part, N, C, HW, P);
    int rc = check_launch("fpn_bn_reduce_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(fpn_bn_finalize_kernel<0>, dim3(1), dim3(64), 0, st, (const double*)part, sums, stats, (float*)nullptr, conv_bias, running_mean,
                       running_var, count, eps, momentum, C, P);
    rc = check_launch("fpn_bn_finalize_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(fpn_bn_apply_kernel<0>, dim3(N * C, ceil_div(HW, FB_CHUNK)), dim3(256), 0, st, z, (const float*)nullptr, (const float*)stats, gamma,
                       beta, (const double*)sums, y, count, C, HW);
    return check_launch("fpn_bn_apply_kernel");
}

extern "C" int mvs_fpn_bn_swish_bwd(const float* dy, const float* z, const float* stats, const float* gamma, const float* beta, float* dz,
                                    float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, void* stream) {
    if (!fb_args("mvs_fpn_bn_swish_bwd", N, C, H, W)) return MVS_ERR_ARG;
    if (!dy || !z || !stats || !gamma || !beta || !dz || !d_gamma || !d_beta || !workspace) { set_error("mvs_fpn_bn_swish_bwd: bad arguments"); return MVS_ERR_ARG; }
    if (workspace_bytes < mvs_fpn_bn_workspace_bytes(N, C, H, W)) { set_error("mvs_fpn_bn_swish_bwd: workspace smaller than mvs_fpn_bn_workspace_bytes"); return MVS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, P = fb_parts(HW);
    const double count = (double)N * (double)HW;
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = part + (size_t)C * P * 2;
    hipLaunchKernelGGL(fpn_bn_reduce_kernel<1>, dim3(P, C), dim3(256), 512 * sizeof(double), st, z, dy, stats, gamma, beta, part, N, C, HW, P);
    int rc = check_launch("fpn_bn_reduce_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(fpn_bn_finalize_kernel<1>, dim3(1), dim3(64), 0, st, (const double*)part, sums, d_beta, d_gamma, (const float*)nullptr,
                       (float*)nullptr, (float*)nullptr, count, 0.0f, 0.0f, C, P);
    rc = check_launch("fpn_bn_finalize_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(fpn_bn_apply_kernel<1>, dim3(N * C, ceil_div(HW, FB_CHUNK)), dim3(256), 0, st, z, dy, stats, gamma, beta, (const double*)sums, dz,
                       count, C, HW);
    return check_launch("fpn_bn_apply_kernel");
}

// ---- data gradients: stride-1 convolutions without bias or activation ----
// (Cin, Cout, k): d intra_k from dz_k (3x3, and out0's 1x1), d lateral_k = W_inner^T d intra_k (1x1), and the composed 8 -> 8 3x3 that
// takes dz_3 to d conv01
#define MVS_FPN_TRAIN_CONVS(X) X(32, 64, 3) X(16, 64, 3) X(8, 64, 3) X(64, 64, 1) X(64, 32, 1) X(64, 16, 1) X(8, 8, 3)

extern "C" int mvs_fpn_train_conv_is_built(int Cin, int Cout, int k) {
#define MVS_FPN_IS(CI, CO, KK) if (Cin == CI && Cout == CO && k == KK) return 1;
    MVS_FPN_TRAIN_CONVS(MVS_FPN_IS)
#undef MVS_FPN_IS
    return 0;
}

extern "C" int mvs_fpn_train_conv_fwd(const float* x, const void* w_packed, float* y, int N, int Cin, int Cout, int k, int H, int W, void* stream) {
    if (!x || !w_packed || !y || N < 1 || N > 65535 || H < 1 || W < 1 || (long long)N * 64 * H * W >= (1LL << 40)) {
        set_error("mvs_fpn_train_conv_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    const PlanarSrc src{x, Cin, H, W, nullptr};
    const PlanarSink<false> sink{nullptr, 0, y, nullptr, 0};
#define MVS_FPN_GO(CI, CO, KK) \
    if (Cin == CI && Cout == CO && k == KK) return launch_conv2d_split<CI, CO, KK, 1>(src, w_packed, sink, N, H, W, (hipStream_t)stream, "fpn_train_conv_kernel");
    MVS_FPN_TRAIN_CONVS(MVS_FPN_GO)
#undef MVS_FPN_GO
    set_error("mvs_fpn_train_conv_fwd: built for the FPNDecoder's data gradients (mvs_fpn_train_conv_is_built); got (Cin %d, Cout %d, k %d)", Cin, Cout, k);
    return MVS_ERR_UNSUPPORTED;
}

// ---- weight gradients ----
// (Cout, Cin, k, ones): d W_out_k (32 | 16 x 64 x 3 x 3 and out0's 64 x 64), d W_inner_k | d b_inner_k (64 x Ck + the ones column), and the
// 8 x (8 + 1) x 3 x 3 correlation of dz_3 with conv01 that d W_inner_3 and d b_inner_3 are contracted from
#define MVS_FPN_WGRADS(X) X(32, 64, 3, false) X(16, 64, 3, false) X(64, 64, 1, false) X(64, 32, 1, true) X(64, 16, 1, true) X(8, 8, 3, true)

template <int COUT, int CIN, int K, bool ONES>
static size_t fw_workspace(int N, int H, int W) {
    const long long tiles = fw_tiles<COUT, CIN, K, ONES>(N, H, W);
    if (tiles > 0x7fffffffLL) return 0;
    return (size_t)fw_parts<COUT, CIN, K, ONES>(tiles) * COUT * FpnWgradShape<COUT, CIN, K, ONES>::NCOL * sizeof(float);
}

extern "C" size_t mvs_fpn_wgrad_workspace_bytes(int N, int Cin, int Cout, int k, int ones, int H, int W) {
    if (N < 1 || N > 65535 || H < 1 || W < 1) return 0;
#define MVS_FPN_WS(CO, CI, KK, ON) if (Cout == CO && Cin == CI && k == KK && (ones != 0) == ON) return fw_workspace<CO, CI, KK, ON>(N, H, W);
    MVS_FPN_WGRADS(MVS_FPN_WS)
#undef MVS_FPN_WS
    return 0;
}

extern "C" int mvs_fpn_wgrad(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int k,
                             int ones, int H, int W, void* stream) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)N * 64 * H * W >= (1LL << 40)) { set_error("mvs_fpn_wgrad: bad arguments"); return MVS_ERR_ARG; }
    const size_t need = mvs_fpn_wgrad_workspace_bytes(N, Cin, Cout, k, ones, H, W);
    if (!need) {
        set_error("mvs_fpn_wgrad: built for the FPNDecoder's weight gradients; got (Cout %d, Cin %d, k %d, ones %d)", Cout, Cin, k, ones);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!dy || !x || !dw || !workspace || workspace_bytes < need) { set_error("mvs_fpn_wgrad: bad arguments (workspace: mvs_fpn_wgrad_workspace_bytes)"); return MVS_ERR_ARG; }
    const PlanarSrc src{x, Cin, H, W, nullptr};
#define MVS_FPN_WG(CO, CI, KK, ON) \
    if (Cout == CO && Cin == CI && k == KK && (ones != 0) == ON) \
        return launch_fpn_wgrad<CO, CI, KK, ON>(src, dy, dw, reinterpret_cast<float*>(workspace), N, H, W, (hipStream_t)stream);
    MVS_FPN_WGRADS(MVS_FPN_WG)
#undef MVS_FPN_WG
    return MVS_ERR_UNSUPPORTED;
}

extern "C" size_t mvs_fpn_merge_wgrad_workspace_bytes(int N, int H, int W) {
    if (N < 1 || N > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1)) return 0;
    return fw_workspace<8, 64, 3, false>(N, H, W);
}

extern "C" int mvs_fpn_merge_wgrad(const float* dy, const float* prev, const float* lateral, const float* w_inner, const float* b_inner, float* dw,
                                   void* workspace, size_t workspace_bytes, int N, int H, int W, void* stream) {
    const size_t need = mvs_fpn_merge_wgrad_workspace_bytes(N, H, W);
    if (!dy || !prev || !lateral || !w_inner || !b_inner || !dw || !workspace || !need || workspace_bytes < need ||
        (long long)N * 64 * H * W >= (1LL << 40)) {
        set_error("mvs_fpn_merge_wgrad: bad arguments (H, W even and >= 2; workspace: mvs_fpn_merge_wgrad_workspace_bytes)");
        return MVS_ERR_ARG;
    }
    return launch_fpn_wgrad<8, 64, 3, false>(merge_src<8>(prev, lateral, w_inner, b_inner, H, W), dy, dw, reinterpret_cast<float*>(workspace), N, H, W,
                                             (hipStream_t)stream);
}

// ---- adjoint of the upsample ----
extern "C" int mvs_fpn_up2_adjoint(const float* d_fine, float* d_coarse, int N, int H, int W, void* stream) {
    if (!d_fine || !d_coarse || N < 1 || N > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1) || (long long)N * 64 * H * W >= (1LL << 40)) {
        set_error("mvs_fpn_up2_adjoint: bad arguments (H, W even and >= 2)");
        return MVS_ERR_ARG;
    }
    const int h = H / 2, w = W / 2;
    hipLaunchKernelGGL(fpn_up2_adjoint_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4), N), dim3(256), 0, (hipStream_t)stream, d_fine, d_coarse, H, W, h, w,
                       up2_scale(h, H), up2_scale(w, W));
    return check_launch("fpn_up2_adjoint_kernel");
}
