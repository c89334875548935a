// FPNEncoder in train mode, forward and backward.
//
// Reference (restated, never copied): models/module.py:47-86, 200-233 - eleven blocks leaky_relu(BatchNorm2d(Conv2d(no bias)(x)), 0.1) with
// batch statistics over all N H W samples of a channel; 7x7, 5x5 and 3x3 taps, three of the blocks at stride 2.
//
// The forward convolutions are the inference kernels on un-folded weights (fpn_kernels.hip, mvs_fpn_conv_fwd), and so are the data
// gradients of the stride-1 blocks (Cin = Cout: the same instances on flipped, channel-transposed taps).  This file adds:
//   1. BatchNorm + LeakyReLU(0.1), forward and backward: the planar fp64-partial kernels of fpn_bn.h with ACT = FB_LEAKY.  The backward
//      recomputes u = gamma xhat + beta from the saved z and statistics; du = dy (u > 0 ? 1 : 0.1);
//   2. weight gradients of the encoder's eight distinct layers: fpn_wgrad_kernel (fpn_wgrad.h) with 3 | 8 .. 64 input channels, 3x3 .. 7x7 taps
//      and stride 1 | 2 (list MVS_FPN_ENC_WGRADS), exact-fp32 MFMA, ordered partials;
//   3. data gradients of the three stride-2 blocks: dx = the stride-2 transposed convolution of dz, as four parity classes.  Row 2 i + py
//      of dx takes tap ky from row o of dz where 2 o + ky - k/2 = 2 i + py, i.e. o = i + r - 1 with ky = py + k/2 + 2 - 2 r for r = 0, 1, 2
//      (taps outside 0 .. k - 1 are zero), and the same along x: every class is a 3x3 stride-1 padding-1 convolution of dz
//      (packing.pack_fpn_enc_dgrad_weights builds the four tap sets), an instance of conv2d_split_kernel with ParitySink, which stores
//      pixel (y, x) of class (py, px) at (2 y + py, 2 x + px) of dx.  One launch per class.
// No atomic anywhere: gradients are the same bits from run to run.  Staged positions are clamped to the image explicitly.
#include "fpn_bn.h"
#include "fpn_wgrad.h"

namespace mvs {

// Planar fp32 [N, COUT, 2 OH, 2 OW], class (py, px) of a stride-2 transposed convolution: pixel (y, x) goes to (2 y + py, 2 x + px).  A
// lane group's 16 pixels of one channel are 8 bytes apart (one 128-byte line, every other float; the px ^ 1 class's launch fills the
// rest).  Like PlanarSink the stores go through __restrict__ parameters.
struct ParitySink {
    float* out;
    int py, px;
    float* ob;
    size_t ohw;
    __device__ __forceinline__ void at(int n, int y, int cout, int OH, int OW) {
        ohw = (size_t)OH * OW * 4;
        ob = out + (size_t)n * cout * ohw + (size_t)(2 * y + py) * (2 * OW) + px;
    }
    static __device__ __forceinline__ void store4_to(float* __restrict__ o, size_t ohw, const f32x4& a) {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[(size_t)k * ohw] = a[k];
    }
    __device__ __forceinline__ void store4(int xx, int co, const f32x4& a) const { store4_to(ob + (size_t)co * ohw + 2 * xx, ohw, a); }
};

// bytes of one class's packed weights: packing.pack_fpn_conv_weights(w [COUT, CIN, 3, 3], 1)
template <int CIN, int COUT>
static size_t dgrad_class_bytes() {
    typedef Conv2dShape<CIN, 3, 1> F;
    return (size_t)F::NPASS * F::NSTEP * ((COUT + 15) / 16) * 2 * 64 * sizeof(bf16x8);
}

// CI, CO: the LAYER's channels (dz has CO, dx has CI); OH, OW: dz's size
template <int CI, int CO>
static int launch_enc_dgrad(const float* dz, const void* w_packed, float* dx, int N, int OH, int OW, hipStream_t st) {
    const PlanarSrc src{dz, CO, OH, OW, nullptr};
    for (int cls = 0; cls < 4; ++cls) {
        const ParitySink sink{dx, cls >> 1, cls & 1, nullptr, 0};
        const char* wp = reinterpret_cast<const char*>(w_packed) + (size_t)cls * dgrad_class_bytes<CO, CI>();
        const int rc = launch_conv2d_split<CO, CI, 3, 1>(src, wp, sink, N, OH, OW, st, "fpn_enc_dgrad_kernel");
        if (rc != MVS_OK) return rc;
    }
    return MVS_OK;
}

}  // namespace mvs

using namespace mvs;

// ---- BatchNorm + LeakyReLU(0.1) ----
extern "C" int mvs_fpn_bn_leaky_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, float* stats, float* y, void* workspace, size_t workspace_bytes, int N,
                                    int C, int H, int W, void* stream) {
    return fb_forward<FB_LEAKY>("mvs_fpn_bn_leaky_fwd", z, conv_bias, gamma, beta, eps, momentum, running_mean, running_var, stats, y, workspace,
                                workspace_bytes, N, C, H, W, (hipStream_t)stream);
}

extern "C" int mvs_fpn_bn_leaky_bwd(const float* dy, const float* z, const float* stats, const float* gamma, const float* beta, float* dz,
                                    float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, void* stream) {
    return fb_backward<FB_LEAKY>("mvs_fpn_bn_leaky_bwd", dy, z, stats, gamma, beta, dz, d_gamma, d_beta, workspace, workspace_bytes, N, C, H, W,
                                 (hipStream_t)stream);
}

// ---- weight gradients ----
// (Cout, Cin, k, stride) of the encoder's eight distinct layers (module.py:203-216)
#define MVS_FPN_ENC_WGRADS(X) X(8, 3, 7, 1) X(8, 8, 5, 1) X(16, 8, 5, 2) X(16, 16, 3, 1) X(32, 16, 5, 2) X(32, 32, 3, 1) X(64, 32, 3, 2) X(64, 64, 3, 1)

static bool enc_dims(int N, int H, int W) { return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long long)N * 64 * H * W < (1LL << 40); }

extern "C" size_t mvs_fpn_enc_wgrad_workspace_bytes(int N, int Cin, int Cout, int k, int stride, int H, int W) {
    if (!enc_dims(N, H, W)) return 0;
#define MVS_FPN_WS(CO, CI, KK, SS) \
    if (Cout == CO && Cin == CI && k == KK && stride == SS) return fw_workspace<CO, CI, KK, false>(N, (H - 1) / SS + 1, (W - 1) / SS + 1);
    MVS_FPN_ENC_WGRADS(MVS_FPN_WS)
#undef MVS_FPN_WS
    return 0;
}

extern "C" int mvs_fpn_enc_wgrad(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int k,
                                 int stride, int H, int W, void* stream) {
    if (!enc_dims(N, H, W)) { set_error("mvs_fpn_enc_wgrad: bad arguments"); return MVS_ERR_ARG; }
    const size_t need = mvs_fpn_enc_wgrad_workspace_bytes(N, Cin, Cout, k, stride, H, W);
    if (!need) {
        set_error("mvs_fpn_enc_wgrad: built for the FPNEncoder's weight gradients; got (Cout %d, Cin %d, k %d, stride %d)", Cout, Cin, k, stride);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!dy || !x || !dw || !workspace || workspace_bytes < need) {
        set_error("mvs_fpn_enc_wgrad: bad arguments (workspace: mvs_fpn_enc_wgrad_workspace_bytes)");
        return MVS_ERR_ARG;
    }
    const PlanarSrc src{x, Cin, H, W, nullptr};
#define MVS_FPN_WG(CO, CI, KK, SS) \
    if (Cout == CO && Cin == CI && k == KK && stride == SS) \
        return launch_fpn_wgrad<CO, CI, KK, false, SS>(src, dy, dw, reinterpret_cast<float*>(workspace), N, H, W, (hipStream_t)stream);
    MVS_FPN_ENC_WGRADS(MVS_FPN_WG)
#undef MVS_FPN_WG
    return MVS_ERR_UNSUPPORTED;
}

// ---- data gradients of the stride-2 blocks ----
// (Cin, Cout, k) of downsample1 / 2 / 3
#define MVS_FPN_ENC_DGRADS(X) X(8, 16, 5) X(16, 32, 5) X(32, 64, 3)

extern "C" int mvs_fpn_enc_dgrad_is_built(int Cin, int Cout, int k, int stride) {
#define MVS_FPN_IS(CI, CO, KK) if (Cin == CI && Cout == CO && k == KK && stride == 2) return 1;
    MVS_FPN_ENC_DGRADS(MVS_FPN_IS)
#undef MVS_FPN_IS
    return 0;
}

extern "C" size_t mvs_fpn_enc_dgrad_weights_bytes(int Cin, int Cout, int k) {
#define MVS_FPN_WB(CI, CO, KK) if (Cin == CI && Cout == CO && k == KK) return 4 * dgrad_class_bytes<CO, CI>();
    MVS_FPN_ENC_DGRADS(MVS_FPN_WB)
#undef MVS_FPN_WB
    return 0;
}

extern "C" int mvs_fpn_enc_dgrad(const float* dz, const void* w_packed, float* dx, int N, int Cin, int Cout, int k, int H, int W, void* stream) {
    if (!dz || !w_packed || !dx || !enc_dims(N, H, W) || H < 2 || W < 2 || (H & 1) || (W & 1)) {
        set_error("mvs_fpn_enc_dgrad: bad arguments (H, W of dx even and >= 2)");
        return MVS_ERR_ARG;
    }
#define MVS_FPN_DG(CI, CO, KK) \
    if (Cin == CI && Cout == CO && k == KK) return launch_enc_dgrad<CI, CO>(dz, w_packed, dx, N, H / 2, W / 2, (hipStream_t)stream);
    MVS_FPN_ENC_DGRADS(MVS_FPN_DG)
#undef MVS_FPN_DG
    set_error("mvs_fpn_enc_dgrad: built for the FPNEncoder's stride-2 blocks (mvs_fpn_enc_dgrad_is_built); got (Cin %d, Cout %d, k %d)", Cin, Cout, k);
    return MVS_ERR_UNSUPPORTED;
}
