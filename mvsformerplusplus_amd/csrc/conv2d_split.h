// The 2-D split-bf16 convolution: ONE implicit-GEMM kernel template for the feature side - the FPN layers (fpn_kernels.hip), the
// FMT pathway (fmt_kernels.hip), the producer-side feature emitter (feat_conv_kernels.hip) and the data gradients of FPN training
// (fpn_train_kernels.hip, fpn_encoder_train_kernels.hip) are instances of it.
//
// Conv2d(CIN, COUT, K = 1 | 3 | 5 | 7, stride S = 1 | 2, padding K/2), fp32-equivalent: v_mfma_f32_16x16x32_bf16 with the three-term
// split-bf16 product (hi*hi + hi*lo + lo*hi, fp32 accumulate; the result must not depend on the input being rounded),
// D[cout, pixel] += W[cout, k] X[k, pixel], k = (tap, cin).  A workgroup owns 4 output rows x 64 columns (one row per wave, four
// 16-pixel column blocks per wave); the input tile + halo is staged once per channel pass, split once into hi | lo bf16 and kept in LDS
// channel-last ([octet plane][pixel][hi x8 | lo x8]) so that a B operand (8 consecutive input channels of one pixel) is one
// ds_read_b128 per half; packed weights (packing.pack_fpn_conv_weights) come per step from global / L2 in lane order.
//
// An instance differs from another in three things only:
//   Src   where a staged pixel's eight channels come from: s.at(n, gy, gx) once per staged pixel inside the image, then
//         s.load8(c0, v) per channel octet (planar tensors here; the merge sources of fpn_kernels.hip / fmt_kernels.hip compute the
//         pixel on the fly).  Src::STAGE_OCTETS = octets a staging work-item loads after one at(): 0 = all of the pass (at() is the
//         expensive call of a merge source), 1 where load8 itself holds many registers (the emitter's run-time dtype);
//   shape CIN, COUT, K, S (Conv2dShape);
//   Sink  everything after the accumulators: s.at(n, y, COUT, OH, OW) per output row, then s.store4(x, co, acc) with the lane's four
//         consecutive output channels co .. co + 3 of pixel (y, x).
// Staged positions are clamped to the image explicitly (zero padding from a branch, never from an out-of-range load).
#pragma once
#include "mvs_common.h"
#include "split_format.h"

namespace mvs {

constexpr int C2_TH = 4, C2_TW = 64;                   // output rows x columns of a workgroup

template <int CIN, int K, int S>
struct Conv2dShape {
    static constexpr int CINP = (CIN + 7) / 8 * 8;                             // Cin = 3 is staged as one octet (channels 3..7 zero)
    static constexpr int CH = S == 1 ? (CINP < 32 ? CINP : 32) : 8;           // channels staged per pass (packing.fpn_chunk)
    static constexpr int OPT = CH / 8, NPASS = CINP / CH, NOCT = K * K * OPT, NSTEP = (NOCT + 3) / 4;
    static constexpr int IH = (C2_TH - 1) * S + K, IW = (C2_TW - 1) * S + K, NPIX = IH * IW;
    static constexpr int PLANE = NPIX * 32 + 32;                               // bytes of one octet plane (+ one slot: bank rows differ)
    static constexpr size_t LDS = (size_t)OPT * PLANE;
};

// ---- sources ----

// planar fp32 [N, C, H, W]: channels >= C read as zero (Cin = 3 padded to one octet)
struct PlanarSrc {
    static constexpr int STAGE_OCTETS = 0;
    const float* x;
    int C, H, W;
    const float* p;
    __device__ __forceinline__ void at(int n, int gy, int gx) { p = x + ((size_t)n * C * H + gy) * W + gx; }
    __device__ __forceinline__ void load8(int c0, float* v) const {
        const size_t hw = (size_t)H * W;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = c0 + k < C ? p[(size_t)(c0 + k) * hw] : 0.0f;
    }
};

// ---- sinks ----

__device__ __forceinline__ float conv2d_act(float t, int act) {
    if (act == 1) return t / (1.0f + expf(-t));               // Swish (module.py Swish: x * sigmoid(x))
    if (act == 2) return t > 0.0f ? t : 0.1f * t;             // F.leaky_relu(y, 0.1) (module.py Conv2d)
    return t;
}

// A null bias adds -0.0f, the additive identity (t + -0.0f == t for every t, -0.0f included): the accumulator reaches the activation as it is.
__device__ __forceinline__ float conv2d_bias(float t, const float* bias, int co) { return t + (bias ? bias[co] : -0.0f); }

// bias (nullable: a folded BatchNorm shift), activation, planar fp32 [N, COUT, OH, OW]: 16 consecutive pixels of one channel per lane
// group = 64 contiguous bytes.  EPILOGUE = false stores the accumulators as they are: the FMT pathway has neither bias nor activation,
// and with the run-time checks between its stores its full-resolution level fell outside the A/B margin.  The stores go through
// store4_to's __restrict__ parameters: as plain members of a by-value struct `out` and `bias` may alias, every bias load then waits
// behind the store before it, and the fused last FPN level measured 4 % slower (both figures: profiles/conv2d_unify_ab.json,
// earlier_forms).
template <bool EPILOGUE>
struct PlanarSink {
    const float* bias;
    int act;
    float* out;
    float* ob;
    size_t ohw;
    __device__ __forceinline__ void at(int n, int y, int cout, int OH, int OW) {
        ohw = (size_t)OH * OW;
        ob = out + (size_t)n * cout * ohw + (size_t)y * OW;
    }
    static __device__ __forceinline__ void store4_to(float* __restrict__ o, size_t ohw, const float* __restrict__ bias, int act, const f32x4& a) {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[(size_t)k * ohw] = EPILOGUE ? conv2d_act(conv2d_bias(a[k], bias, k), act) : a[k];
    }
    __device__ __forceinline__ void store4(int xx, int co, const f32x4& a) const { store4_to(ob + (size_t)co * ohw + xx, ohw, bias ? bias + co : nullptr, act, a); }
};

// ---- the kernel ----

template <int CIN, int COUT, int K, int S, class Src, class Sink>
__global__ __launch_bounds__(256) void conv2d_split_kernel(Src src, const void* __restrict__ wp, Sink sink, int H, int W, int OH, int OW,
                                                           int tiles_x, int ntiles) {
    typedef Conv2dShape<CIN, K, S> F;
    constexpr int OPT = F::OPT, NOCT = F::NOCT, NSTEP = F::NSTEP, IW = F::IW, NPIX = F::NPIX, P = K / 2;
    constexpr int MREP = (COUT + 15) / 16, NREP = C2_TW / 16;
    constexpr int UNROLL = MREP >= 4 ? 3 : NSTEP;                 // 64 output channels: a full unroll hoists weight loads into spills
    HIP_DYNAMIC_SHARED(float4, lds4)
    char* ldsb = reinterpret_cast<char*>(lds4);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int tile = (int)xcd_remap(blockIdx.x, (unsigned)ntiles), n = (int)blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * C2_TH, x0 = tx * C2_TW;

    f32x4 acc[MREP][NREP];
#pragma unroll
    for (int mb = 0; mb < MREP; ++mb)
#pragma unroll
        for (int nb = 0; nb < NREP; ++nb) acc[mb][nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    for (int pass = 0; pass < F::NPASS; ++pass) {
        if (pass > 0) __syncthreads();                            // every wave has read the previous pass's image
        // ---- stage: one work-item = one staged pixel x Src::STAGE_OCTETS of the pass's OPT octets (0 = all of them); consecutive
        //      work-items = consecutive pixels ----
        constexpr int SO = Src::STAGE_OCTETS == 0 ? OPT : Src::STAGE_OCTETS, NGRP = OPT / SO;
        static_assert(OPT % SO == 0, "Src::STAGE_OCTETS must divide the octets of a pass");
        for (int e = tid; e < NPIX * NGRP; e += 256) {
            const int grp = NGRP == 1 ? 0 : e / NPIX, pix = e - grp * NPIX;
            const int iy = pix / IW, ix = pix - iy * IW;
            const int gy = y0 * S - P + iy, gx = x0 * S - P + ix;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;          // zero padding (padding = k/2) outside the image
            Src s = src;
            if (inside) s.at(n, gy, gx);
#pragma unroll
            for (int oc = grp * SO; oc < grp * SO + SO; ++oc) {
                float v[8];
                if (inside) {
                    s.load8(pass * F::CH + oc * 8, v);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = 0.0f;
                }
                bf16x8 hi, lo;
                split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hi, lo);
                char* dst = ldsb + oc * F::PLANE + pix * 32;
                *reinterpret_cast<bf16x8*>(dst) = hi;
                *reinterpret_cast<bf16x8*>(dst + 16) = lo;
            }
        }
        __syncthreads();
        // ---- contract: step = four channel octets (one per lane group), octet q = 4 step + g -> (tap, oc) = divmod(q, OPT) ----
        const bf16x8* wq = reinterpret_cast<const bf16x8*>(wp) + (size_t)pass * NSTEP * MREP * 2 * 64 + lane;
#pragma unroll UNROLL
        for (int step = 0; step < NSTEP; ++step) {
            const int q = 4 * step + g;
            const bool live = q < NOCT;                           // the last step may run past the K x K x OPT octets: zero operand (the packed weights are zero there too)
            const int tap = live ? q / OPT : 0, oc = live ? q - tap * OPT : 0;
            const int ky = tap / K, kx = tap - ky * K;
            const char* srcp = ldsb + oc * F::PLANE + ((wave * S + ky) * IW + li * S + kx) * 32;
            bf16x8 ah[MREP], al[MREP], bh[NREP], bl[NREP];
#pragma unroll
            for (int mb = 0; mb < MREP; ++mb) {
                ah[mb] = wq[(size_t)((step * MREP + mb) * 2 + 0) * 64];
                al[mb] = wq[(size_t)((step * MREP + mb) * 2 + 1) * 64];
            }
#pragma unroll
            for (int nb = 0; nb < NREP; ++nb) {
                bf16x8 h = *reinterpret_cast<const bf16x8*>(srcp + nb * 16 * S * 32);
                bf16x8 l = *reinterpret_cast<const bf16x8*>(srcp + nb * 16 * S * 32 + 16);
                if (!live) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) { h[k] = (__bf16)0.0f; l[k] = (__bf16)0.0f; }
                }
                bh[nb] = h;
                bl[nb] = l;
            }
#pragma unroll
            for (int mb = 0; mb < MREP; ++mb)
#pragma unroll
                for (int nb = 0; nb < NREP; ++nb) acc[mb][nb] = mfma3_bf16(ah[mb], al[mb], bh[nb], bl[nb], acc[mb][nb]);
        }
    }

    // ---- epilogue: lane (pixel li, group g) holds output channels 16 mb + 4 g .. + 3 of its pixel ----
    const int y = y0 + wave;
    if (y >= OH) return;
    sink.at(n, y, COUT, OH, OW);
#pragma unroll
    for (int nb = 0; nb < NREP; ++nb) {
        const int xx = x0 + nb * 16 + li;
        if (xx >= OW) continue;
#pragma unroll
        for (int mb = 0; mb < MREP; ++mb) {
            const int co = 16 * mb + 4 * g;
            if (co >= COUT) continue;
            sink.store4(xx, co, acc[mb][nb]);
        }
    }
}

// `what` names the launch in the error text of a failed one
template <int CIN, int COUT, int K, int S, class Src, class Sink>
static int launch_conv2d_split(const Src& src, const void* wp, const Sink& sink, int N, int H, int W, hipStream_t st, const char* what) {
    typedef Conv2dShape<CIN, K, S> F;
    const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;                      // padding k/2, odd k
    const int tiles_x = (int)ceil_div(OW, C2_TW), tiles_y = (int)ceil_div(OH, C2_TH);
    if (F::LDS > 48 * 1024)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_split_kernel<CIN, COUT, K, S, Src, Sink>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)F::LDS);
    hipLaunchKernelGGL((conv2d_split_kernel<CIN, COUT, K, S, Src, Sink>), dim3(tiles_x * tiles_y, N), dim3(256), F::LDS, st, src, wp, sink, H, W, OH, OW,
                       tiles_x, tiles_x * tiles_y);
    return check_launch(what);
}

// The unfused form of a merge source: its map written out as planar fp32 [N, C, H, W], one thread per pixel.  UNROLL: octets of the
// channel loop in flight (1 where load8 carries a long dot product per channel and more would spill).
template <int C, int UNROLL, class Src>
__global__ __launch_bounds__(256) void conv2d_source_kernel(Src src, float* __restrict__ out) {
    const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), n = (int)blockIdx.z;
    if (x >= src.W || y >= src.H) return;
    Src s = src;
    s.at(n, y, x);
    const size_t HW = (size_t)src.H * src.W;
    float* o = out + (size_t)n * C * HW + (size_t)y * src.W + x;
#pragma unroll UNROLL
    for (int c0 = 0; c0 < C; c0 += 8) {
        float v[8];
        s.load8(c0, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[(size_t)(c0 + k) * HW] = v[k];
    }
}

template <int C, int UNROLL, class Src>
static int launch_conv2d_source(const Src& src, float* out, int N, hipStream_t st, const char* what) {
    hipLaunchKernelGGL((conv2d_source_kernel<C, UNROLL, Src>), dim3(ceil_div(src.W, 64), ceil_div(src.H, 4), N), dim3(256), 0, st, src, out);
    return check_launch(what);
}

}  // namespace mvs
