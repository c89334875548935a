// Planar batch-statistics BatchNorm + activation on fp32 [N, C, H, W], forward and backward: the three kernel templates that the FPN
// decoder's training unit (fpn_train_kernels.hip, Swish) and the encoder's (fpn_encoder_train_kernels.hip, LeakyReLU 0.1) instantiate.
//   fpn_bn_reduce_kernel    per-channel [sum z | sum z^2], or [sum du | sum du xhat] in the backward, accumulated in fp64 and left as one
//                           partial per workgroup;
//   fpn_bn_finalize_kernel  adds the partials front to back; mean / biased variance / invstd and the running-statistics step, or
//                           d beta / d gamma;
//   fpn_bn_apply_kernel     y = act(gamma xhat + beta), or dz = gamma invstd (du - d beta / M - xhat d gamma / M).
// ACT is a template parameter of all three (the finalize does not evaluate it: it keeps the instances of the two units apart).
// No atomic anywhere: results are the same bits from run to run.
#pragma once
#include "mvs_common.h"

namespace mvs {

constexpr int FB_MAX_PARTS = 64;              // partials per channel: the finalize adds them one after the other
constexpr int FB_CHUNK = 1024;                // elements of one plane per workgroup of the apply kernel
constexpr int FB_SWISH = 1, FB_LEAKY = 2;     // ACT: u sigmoid(u) | leaky_relu(u, 0.1)

__device__ __forceinline__ float fb_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }

// y = act(u)
template <int ACT>
__device__ __forceinline__ float fb_act(float u) {
    if (ACT == FB_LEAKY) return u > 0.0f ? u : 0.1f * u;
    return u * fb_sigmoid(u);
}

// du = dy act'(u); LeakyReLU: PyTorch's rule, slope 0.1 at u <= 0
template <int ACT>
__device__ __forceinline__ float fb_act_bwd(float dy, float u) {
    if (ACT == FB_LEAKY) return u > 0.0f ? dy : 0.1f * dy;
    const float s = fb_sigmoid(u);
    return dy * (s + u * s * (1.0f - s));
}

// stats = [mean | biased variance | invstd], [3][C]
template <int MODE, int ACT>
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
                const float xh = (v - mean) * invstd, u = xh * g + b;
                const float du = fb_act_bwd<ACT>(dy[base + i], u);
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
template <int MODE, int ACT>
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

// MODE 0: out = act(gamma xhat + beta).  MODE 1: out = dz = gamma invstd (du - sum du / M - xhat sum du xhat / M).
template <int MODE, int ACT>
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
        const float xh = (z[base + i] - mean) * invstd, u = xh * g + b;
        if (MODE == 0) {
            out[base + i] = fb_act<ACT>(u);
        } else {
            const float du = fb_act_bwd<ACT>(dy[base + i], u);
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

static size_t fb_workspace_bytes(int N, int C, int H, int W) {
    if (N < 1 || N > 65535 || C < 1 || C > 64 || H < 1 || W < 1 || (long long)H * W > 0x3fffffffLL) return 0;
    return ((size_t)C * fb_parts(H * W) * 2 + 2 * (size_t)C) * sizeof(double);
}

// The three launches of a forward: `what` names the entry point in error texts.
template <int ACT>
static int fb_forward(const char* what, const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, float* stats, float* y, void* workspace, size_t workspace_bytes, int N, int C, int H, int W,
                      hipStream_t st) {
    if (!fb_args(what, N, C, H, W)) return MVS_ERR_ARG;
    if (!z || !gamma || !beta || !stats || !y || !workspace || (running_mean == nullptr) != (running_var == nullptr)) {
        set_error("%s: bad arguments", what);
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < fb_workspace_bytes(N, C, H, W)) { set_error("%s: workspace smaller than mvs_fpn_bn_workspace_bytes", what); return MVS_ERR_ARG; }
    const int HW = H * W, P = fb_parts(HW);
    const double count = (double)N * (double)HW;
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = part + (size_t)C * P * 2;
    hipLaunchKernelGGL((fpn_bn_reduce_kernel<0, ACT>), dim3(P, C), dim3(256), 512 * sizeof(double), st, z, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, part, N, C, HW, P);
    int rc = check_launch("fpn_bn_reduce_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL((fpn_bn_finalize_kernel<0, ACT>), dim3(1), dim3(64), 0, st, (const double*)part, sums, stats, (float*)nullptr, conv_bias, running_mean,
                       running_var, count, eps, momentum, C, P);
    rc = check_launch("fpn_bn_finalize_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL((fpn_bn_apply_kernel<0, ACT>), dim3(N * C, ceil_div(HW, FB_CHUNK)), dim3(256), 0, st, z, (const float*)nullptr, (const float*)stats, gamma,
                       beta, (const double*)sums, y, count, C, HW);
    return check_launch("fpn_bn_apply_kernel");
}

template <int ACT>
static int fb_backward(const char* what, const float* dy, const float* z, const float* stats, const float* gamma, const float* beta, float* dz,
                       float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, hipStream_t st) {
    if (!fb_args(what, N, C, H, W)) return MVS_ERR_ARG;
    if (!dy || !z || !stats || !gamma || !beta || !dz || !d_gamma || !d_beta || !workspace) { set_error("%s: bad arguments", what); return MVS_ERR_ARG; }
    if (workspace_bytes < fb_workspace_bytes(N, C, H, W)) { set_error("%s: workspace smaller than mvs_fpn_bn_workspace_bytes", what); return MVS_ERR_ARG; }
    const int HW = H * W, P = fb_parts(HW);
    const double count = (double)N * (double)HW;
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = part + (size_t)C * P * 2;
    hipLaunchKernelGGL((fpn_bn_reduce_kernel<1, ACT>), dim3(P, C), dim3(256), 512 * sizeof(double), st, z, dy, stats, gamma, beta, part, N, C, HW, P);
    int rc = check_launch("fpn_bn_reduce_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL((fpn_bn_finalize_kernel<1, ACT>), dim3(1), dim3(64), 0, st, (const double*)part, sums, d_beta, d_gamma, (const float*)nullptr,
                       (float*)nullptr, (float*)nullptr, count, 0.0f, 0.0f, C, P);
    rc = check_launch("fpn_bn_finalize_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL((fpn_bn_apply_kernel<1, ACT>), dim3(N * C, ceil_div(HW, FB_CHUNK)), dim3(256), 0, st, z, dy, stats, gamma, beta, (const double*)sums, dz,
                       count, C, HW);
    return check_launch("fpn_bn_apply_kernel");
}

}  // namespace mvs
