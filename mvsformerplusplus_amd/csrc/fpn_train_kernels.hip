// FPNDecoder in train mode, forward and backward.
//
// Reference (restated, never copied): models/module.py:236-270 - out_k = Swish(BatchNorm2d(Conv2d(64, C_k, 3 | 1)(intra_k))) with batch
// statistics over all N H W samples of a channel, intra_k = up2(intra_{k-1}) + inner_k(lateral_k).
//
// The forward convolutions are the inference kernels on un-folded weights (fpn_kernels.hip); this file adds what training needs (the
// templates of 1. and 3. are in fpn_bn.h and fpn_wgrad.h, which the encoder's unit fpn_encoder_train_kernels.hip shares; this file
// holds the decoder's instance lists and entry points):
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
#include "fpn_bn.h"
#include "fpn_merge.h"
#include "fpn_wgrad.h"

namespace mvs {

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
extern "C" size_t mvs_fpn_bn_workspace_bytes(int N, int C, int H, int W) { return fb_workspace_bytes(N, C, H, W); }

extern "C" int mvs_fpn_bn_swish_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, float* stats, float* y, void* workspace, size_t workspace_bytes, int N,
                                    int C, int H, int W, void* stream) {
    return fb_forward<FB_SWISH>("mvs_fpn_bn_swish_fwd", z, conv_bias, gamma, beta, eps, momentum, running_mean, running_var, stats, y, workspace,
                                workspace_bytes, N, C, H, W, (hipStream_t)stream);
}

extern "C" int mvs_fpn_bn_swish_bwd(const float* dy, const float* z, const float* stats, const float* gamma, const float* beta, float* dz,
                                    float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, void* stream) {
    return fb_backward<FB_SWISH>("mvs_fpn_bn_swish_bwd", dy, z, stats, gamma, beta, dz, d_gamma, d_beta, workspace, workspace_bytes, N, C, H, W,
                                 (hipStream_t)stream);
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
