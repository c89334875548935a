// Producer-side feature emitter: the LAST convolution of the reference's feature side written
// straight into the layout the gather passes read.
//
// Reference (restated, never copied): the per-stage feature maps that reach StageNet come out of 3x3 Conv2d layers -
//   * FMT_with_pathway.smooth_1 / _2 / _3 (models/FMT.py:195-197: Conv2d(C, C, 3, padding=1, bias=False), C = 32 / 16 / 8) for
//     stages 2-4 of the shipped model (models/FMT.py:231-233, torch.stack over views into [B,V,C,H,W]);
//   * FPNDecoder.out1 / out2 / out3 (models/module.py:257-270: Conv2d(64, C, 3, padding=1) + BatchNorm2d + Swish) where a model feeds
//     the FPN heads to the cost volume directly (casmvs-style networks).
// Both emit planar NCHW; StageNet upcasts per view (cost_volume.py:67) and the gather kernels then read it with one strided plane per
// channel - or, in the hand-off layout [B,V,C/8,H,W,8] (gather_lds.h TILED), one 16- / 32-byte run per pixel and channel octet.  Round 2
// built the consumer side plus a converter pass (mvs_pack_features: one extra read + write of every feature map).  This kernel is the
// producer side: the convolution's epilogue adds the bias, applies the activation (none | Swish, BatchNorm folded on the host), rounds
// to the hand-off dtype (bf16 like the reference's autocast, test.py:250; or fp16 / fp32) and stores octet tiles directly - the
// planar [B,V,C,H,W] tensor is never materialised and no transpose pass runs.
//
// Form: the feature side's shared 3x3 implicit GEMM, conv2d_split_kernel<Cin, Cout, 3, 1, Src, Sink> (conv2d_split.h: split-bf16
// three-term MFMA, fp32-equivalent like the regularisers' "bf16x3" mode; tile, LDS image, weight packing and contraction are defined
// there).  This file adds the emitter's two ends: TypedPlanarSrc reads the planar input in its run-time dtype with any batch stride
// (lane-consecutive loads along x, one plane per channel: coalesced; one channel octet per staging work-item), TileSink is the epilogue
// described above.
// Roofline: HBM (Cin x 4 B in, Cout x 2 B out per pixel; 64 -> 8 at 1152 x 1536: 453 MB + 28 MB per view) for Cin <= 16, MFMA-issue
// for the 64-channel FPN heads (9.2 KFLOP x 3 terms per pixel).  Not part of the timed path (features are its inputs).
#include "conv2d_split.h"

namespace mvs {

__device__ __forceinline__ float fc_load(const void* p, int dtype, size_t i) {
    if (dtype == MVS_DTYPE_F32) return static_cast<const float*>(p)[i];
    if (dtype == MVS_DTYPE_BF16) return to_f32(static_cast<const uint16_t*>(p)[i]);
    return (float)static_cast<const _Float16*>(p)[i];
}

// planar [N, C, H, W] in a run-time dtype, any batch stride (in elements)
struct TypedPlanarSrc {
    static constexpr int STAGE_OCTETS = 1;            // eight loads in three dtypes in flight per work-item, not 8 x OPT
    const void* x;
    int dtype, H, W;
    long long batch_stride;
    size_t base;
    __device__ __forceinline__ void at(int n, int gy, int gx) { base = (size_t)n * (size_t)batch_stride + (size_t)gy * W + gx; }
    __device__ __forceinline__ void load8(int c0, float* v) const {
        const size_t HW = (size_t)H * (size_t)W;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fc_load(x, dtype, base + (size_t)(c0 + k) * HW);
    }
};

// bias (nullable), none | Swish, the hand-off dtype, octet tiles [N][C/8][H][W][8] with any batch stride (in elements): a lane's four
// channels are half an octet = one 8-byte (16-bit dtypes) / 16-byte (fp32) store
struct TileSink {
    const float* bias;
    int act;
    void* out;
    int dtype;
    long long batch_stride;
    size_t obase;
    int y, H, W;
    __device__ __forceinline__ void at(int n, int y_, int, int OH, int OW) {
        obase = (size_t)n * (size_t)batch_stride;
        y = y_; H = OH; W = OW;
    }
    __device__ __forceinline__ void store4(int xx, int co, const f32x4& a) const {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = conv2d_act(conv2d_bias(a[k], bias, co + k), act);
        const size_t o = obase + (((size_t)(co >> 3) * H + y) * W + xx) * 8 + (co & 7);
        if (dtype == MVS_DTYPE_F32) {
            *reinterpret_cast<float4*>(static_cast<float*>(out) + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else if (dtype == MVS_DTYPE_BF16) {
            typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<u16x4*>(static_cast<uint16_t*>(out) + o) =
                u16x4{from_f32<uint16_t>(v[0]), from_f32<uint16_t>(v[1]), from_f32<uint16_t>(v[2]), from_f32<uint16_t>(v[3])};
        } else {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            const float m = 65504.0f;
            *reinterpret_cast<h4*>(static_cast<_Float16*>(out) + o) =
                h4{(_Float16)fminf(fmaxf(v[0], -m), m), (_Float16)fminf(fmaxf(v[1], -m), m), (_Float16)fminf(fmaxf(v[2], -m), m),
                   (_Float16)fminf(fmaxf(v[3], -m), m)};
        }
    }
};

}  // namespace mvs

using namespace mvs;

// (Cin, Cout) of the reference's feature heads: FMT_with_pathway.smooth_k and FPNDecoder.out_k
#define MVS_FEAT_CONVS(X) X(8, 8) X(16, 16) X(32, 32) X(64, 8) X(64, 16) X(64, 32)

extern "C" int mvs_feature_conv_is_built(int Cin, int Cout) {
#define MVS_FC_IS(CI, CO) if (Cin == CI && Cout == CO) return 1;
    MVS_FEAT_CONVS(MVS_FC_IS)
#undef MVS_FC_IS
    return 0;
}

extern "C" int mvs_conv2d3x3_tiles_fwd(const void* x, int in_dtype, const void* w_packed, const float* bias, int act, void* tiled, int out_dtype, int N,
                                       int Cin, int Cout, int H, int W, long long in_batch_stride, long long out_batch_stride, void* stream) {
    if (!x || !w_packed || !tiled || N < 1 || H < 1 || W < 1) { set_error("mvs_conv2d3x3_tiles_fwd: bad arguments"); return MVS_ERR_ARG; }
    if (in_dtype < MVS_DTYPE_F32 || in_dtype > MVS_DTYPE_F16 || out_dtype < MVS_DTYPE_F32 || out_dtype > MVS_DTYPE_F16) { set_error("mvs_conv2d3x3_tiles_fwd: unknown dtype"); return MVS_ERR_ARG; }
    if (act != 0 && act != 1) { set_error("mvs_conv2d3x3_tiles_fwd: activation must be 0 (none) or 1 (Swish)"); return MVS_ERR_ARG; }
    if (in_batch_stride < (long long)Cin * H * W || out_batch_stride < (long long)Cout * H * W) { set_error("mvs_conv2d3x3_tiles_fwd: batch strides shorter than one image"); return MVS_ERR_ARG; }
    if (!mvs_feature_conv_is_built(Cin, Cout)) {
        set_error("mvs_conv2d3x3_tiles_fwd: built for the reference's feature heads - (Cin, Cout) = (8,8), (16,16), (32,32) [FMT.py:195-197] and "
                  "(64,8), (64,16), (64,32) [module.py:257-270]; got (%d, %d)", Cin, Cout);
        return MVS_ERR_UNSUPPORTED;
    }
    const TypedPlanarSrc src{x, in_dtype, H, W, in_batch_stride, 0};
    const TileSink sink{bias, act, tiled, out_dtype, out_batch_stride, 0, 0, 0, 0};
#define MVS_FC(CI, CO) \
    if (Cin == CI && Cout == CO) return launch_conv2d_split<CI, CO, 3, 1>(src, w_packed, sink, N, H, W, (hipStream_t)stream, "conv2d3x3_tiles_kernel");
    MVS_FEAT_CONVS(MVS_FC)
#undef MVS_FC
    return MVS_ERR_UNSUPPORTED;
}
