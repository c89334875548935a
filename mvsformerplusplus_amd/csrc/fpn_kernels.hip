// FPN feature encoder and decoder: every layer of the reference's FPNEncoder / FPNDecoder at full image
// resolution, fp32-equivalent.
//
// Reference (restated, never copied): models/module.py:47-86 (Conv2d = conv without bias + BatchNorm2d + leaky_relu(0.1)) and
// models/module.py:200-270 (FPNEncoder: conv00 7x7 3->8, conv01 5x5, downsample1/2 5x5 s2, downsample3 3x3 s2, conv10 .. conv31 3x3;
// FPNDecoder: out0 = Swish(BN(1x1 64->64)); intra_k = up2(intra_{k-1}) + inner_k(lateral_k), inner_k = 1x1 conv with bias, up2 =
// F.interpolate(scale_factor=2, bilinear, align_corners=True) in fp32; out_k = Swish(BN(3x3 64->Ck))).
//
// Three kernels, all instances of the templates in conv2d_split.h (this file holds the list of built layers and the entry points;
// MergeSrc is in fpn_merge.h, which the training kernels of fpn_train_kernels.hip share):
//   1. the convolution (reported as fpn_conv_kernel): conv2d_split_kernel<Cin, Cout, k, stride, PlanarSrc, PlanarSink<true>> - Conv2d(k = 1 |
//      3 | 5 | 7, stride 1 | 2, padding k/2) with the BatchNorm folded on the host into weights + bias, then none | Swish |
//      LeakyReLU(0.1); planar fp32 in and out, split-bf16 three-term MFMA (fp32-equivalent).  Cin = 3 is staged as one octet with
//      channels 3..7 zero (their packed weights are zero too).
//   2. the merge (reported as fpn_merge_kernel): conv2d_source_kernel on MergeSrc - intra_k = up2(intra_{k-1}) + inner_k(lateral), one
//      thread per pixel, all 64 channels, fp32 VALU (the 1x1 weights are uniform across the wave); writes the 64-channel fp32 intra_k
//      that out_k and the next level read.
//   3. the last level fused: the convolution with MergeSrc as its source - the staging computes up2(intra2) + inner3(conv01) for the
//      tile and its halo on the fly, so the full-resolution 64-channel intra3 is never written (453 MB write + read per view at
//      1152 x 1536 in fp32).
// Staged positions are clamped to the image explicitly (zero padding from a branch, never from an out-of-range load).
#include "fpn_merge.h"

using namespace mvs;

// (Cin, Cout, k, stride) of every FPNEncoder / FPNDecoder convolution with feat_chs = [8, 16, 32, 64] (module.py:203-216, 246-256)
#define MVS_FPN_CONVS(X) X(3, 8, 7, 1) X(8, 8, 5, 1) X(8, 16, 5, 2) X(16, 16, 3, 1) X(16, 32, 5, 2) X(32, 32, 3, 1) X(32, 64, 3, 2) \
    X(64, 64, 3, 1) X(64, 64, 1, 1) X(64, 32, 3, 1) X(64, 16, 3, 1) X(64, 8, 3, 1)

extern "C" int mvs_fpn_conv_is_built(int Cin, int Cout, int k, int stride) {
#define MVS_FPN_IS(CI, CO, KK, SS) if (Cin == CI && Cout == CO && k == KK && stride == SS) return 1;
    MVS_FPN_CONVS(MVS_FPN_IS)
#undef MVS_FPN_IS
    return 0;
}

extern "C" int mvs_fpn_merge_is_built(int Clat, int Cout) {
    if (Cout == 0) return Clat == 8 || Clat == 16 || Clat == 32 ? 1 : 0;
    return Clat == 8 && Cout == 8 ? 1 : 0;
}

extern "C" int mvs_fpn_conv_fwd(const float* x, const void* w_packed, const float* bias, int act, float* y, int N, int Cin, int Cout, int k,
                                int stride, int H, int W, void* stream) {
    if (!x || !w_packed || !y || N < 1 || N > 65535 || H < 1 || W < 1) { set_error("mvs_fpn_conv_fwd: bad arguments"); return MVS_ERR_ARG; }
    if (act < 0 || act > 2) { set_error("mvs_fpn_conv_fwd: activation must be 0 (none), 1 (Swish) or 2 (LeakyReLU 0.1)"); return MVS_ERR_ARG; }
    if ((long long)N * Cin * H * W >= (1LL << 40)) { set_error("mvs_fpn_conv_fwd: tensor too large"); return MVS_ERR_ARG; }
    if (!mvs_fpn_conv_is_built(Cin, Cout, k, stride)) {
        set_error("mvs_fpn_conv_fwd: built for the FPN layers of feat_chs = [8, 16, 32, 64] [module.py:203-216, 246-256]; got (Cin %d, Cout %d, "
                  "k %d, stride %d)", Cin, Cout, k, stride);
        return MVS_ERR_UNSUPPORTED;
    }
    const PlanarSrc src{x, Cin, H, W, nullptr};
    const PlanarSink<true> sink{bias, act, y, nullptr, 0};
#define MVS_FPN_GO(CI, CO, KK, SS) \
    if (Cin == CI && Cout == CO && k == KK && stride == SS) return launch_conv2d_split<CI, CO, KK, SS>(src, w_packed, sink, N, H, W, (hipStream_t)stream, "fpn_conv_kernel");
    MVS_FPN_CONVS(MVS_FPN_GO)
#undef MVS_FPN_GO
    return MVS_ERR_UNSUPPORTED;
}

extern "C" int mvs_fpn_merge_fwd(const float* prev, const float* lateral, const float* w_inner, const float* b_inner, float* intra, int N, int Clat,
                                 int H, int W, void* stream) {
    if (!prev || !lateral || !w_inner || !b_inner || !intra || N < 1 || N > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1)) {
        set_error("mvs_fpn_merge_fwd: bad arguments (H, W even and >= 2)");
        return MVS_ERR_ARG;
    }
    if (!mvs_fpn_merge_is_built(Clat, 0)) { set_error("mvs_fpn_merge_fwd: lateral width %d (built: 8, 16, 32) [module.py:248-254]", Clat); return MVS_ERR_UNSUPPORTED; }
#define MVS_FPN_MG(CL) \
    if (Clat == CL) return launch_conv2d_source<64, 1>(merge_src<CL>(prev, lateral, w_inner, b_inner, H, W), intra, N, (hipStream_t)stream, "fpn_merge_kernel");
    MVS_FPN_MG(8) MVS_FPN_MG(16) MVS_FPN_MG(32)
#undef MVS_FPN_MG
    return MVS_ERR_UNSUPPORTED;
}

extern "C" int mvs_fpn_merge_conv_fwd(const float* prev, const float* lateral, const float* w_inner, const float* b_inner, const void* w_packed,
                                      const float* bias, int act, float* y, int N, int Clat, int Cout, int H, int W, void* stream) {
    if (!prev || !lateral || !w_inner || !b_inner || !w_packed || !y || N < 1 || N > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1)) {
        set_error("mvs_fpn_merge_conv_fwd: bad arguments (H, W even and >= 2)");
        return MVS_ERR_ARG;
    }
    if (act < 0 || act > 2) { set_error("mvs_fpn_merge_conv_fwd: activation must be 0, 1 or 2"); return MVS_ERR_ARG; }
    if (!mvs_fpn_merge_is_built(Clat, Cout)) {
        set_error("mvs_fpn_merge_conv_fwd: built for the decoder's last level (Clat 8 -> 64 -> Cout 8) [module.py:267-268]; got (%d, %d)", Clat, Cout);
        return MVS_ERR_UNSUPPORTED;
    }
    return launch_conv2d_split<64, 8, 3, 1>(merge_src<8>(prev, lateral, w_inner, b_inner, H, W), w_packed, PlanarSink<true>{bias, act, y, nullptr, 0}, N, H, W,
                                            (hipStream_t)stream, "fpn_conv_kernel");
}
