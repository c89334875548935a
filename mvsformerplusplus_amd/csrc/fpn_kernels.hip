// FPN feature encoder and decoder: every layer of the reference's FPNEncoder / FPNDecoder at full image
// resolution, fp32-equivalent.
//
// Reference (restated, never copied): models/module.py:47-86 (Conv2d = conv without bias + BatchNorm2d + leaky_relu(0.1)) and
// models/module.py:200-270 (FPNEncoder: conv00 7x7 3->8, conv01 5x5, downsample1/2 5x5 s2, downsample3 3x3 s2, conv10 .. conv31 3x3;
// FPNDecoder: out0 = Swish(BN(1x1 64->64)); intra_k = up2(intra_{k-1}) + inner_k(lateral_k), inner_k = 1x1 conv with bias, up2 =
// F.interpolate(scale_factor=2, bilinear, align_corners=True) in fp32; out_k = Swish(BN(3x3 64->Ck))).
//
// Three kernels:
//   1. fpn_conv_kernel: Conv2d(k = 1 | 3 | 5 | 7, stride 1 | 2, padding k/2) with the BatchNorm folded on the host into weights + bias,
//      then none | Swish | LeakyReLU(0.1); planar fp32 in and out.  Implicit GEMM on v_mfma_f32_16x16x32_bf16 with the three-term
//      split-bf16 product (fp32-equivalent), in the form of feat_conv_kernels.hip: a workgroup owns 4 output rows x 64 columns (one
//      row per wave, four 16-pixel column blocks), the input tile + halo is staged once per channel pass, split into hi | lo bf16 and
//      kept channel-last in LDS ([octet plane][pixel][hi x8 | lo x8]); packed weights (packing.pack_conv_weights_bf16x3) come per step
//      from L2 in lane order.  Cin = 3 is staged as one octet with channels 3..7 zero (their packed weights are zero too).
//   2. fpn_merge_kernel: intra_k = up2(intra_{k-1}) + inner_k(lateral), one thread per pixel, all 64 channels, fp32 VALU (the 1x1
//      weights are uniform across the wave); writes the 64-channel fp32 intra_k that out_k and the next level read.
//   3. the last level fused: fpn_conv_kernel with MergeSrc as its source - the staging computes up2(intra2) + inner3(conv01) for the
//      tile and its halo on the fly, so the full-resolution 64-channel intra3 is never written (453 MB write + read per view at
//      1152 x 1536 in fp32).
// Staged positions are clamped to the image explicitly (zero padding from a branch, never from an out-of-range load).
#include "mvs_common.h"
#include "split_format.h"

namespace mvs {

constexpr int FP_TH = 4, FP_TW = 64;

// planar fp32 source [N, C, H, W]: channels >= C read as zero (Cin = 3 padded to one octet)
struct PlanarSrc {
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

// intra[c] at a full-resolution pixel = up2(prev)[c] + b[c] + sum_ci w[c][ci] * lat[ci]; prev [N, 64, H/2, W/2], lat [N, CLAT, H, W]
template <int CLAT>
struct MergeSrc {
    const float* prev;
    const float* lat;
    const float* w;          // [64][CLAT]
    const float* b;          // [64]
    int H, W, h, w2;         // full resolution; prev is h x w2 (H = 2h, W = 2 w2)
    float sy, sx;            // align_corners=True source scale (h - 1) / (H - 1), in fp32 like F.interpolate on fp32 input
    float l[CLAT];
    const float* pp;
    int dy, dx;
    float ly, lx;
    __device__ __forceinline__ void at(int n, int gy, int gx) {
        const size_t HW = (size_t)H * W;
        const float* lp = lat + (size_t)n * CLAT * HW + (size_t)gy * W + gx;
#pragma unroll
        for (int ci = 0; ci < CLAT; ++ci) l[ci] = lp[(size_t)ci * HW];
        const float fy = sy * (float)gy, fx = sx * (float)gx;
        const int y0 = (int)fy, x0 = (int)fx;
        ly = fy - (float)y0;
        lx = fx - (float)x0;
        dy = y0 < h - 1 ? w2 : 0;
        dx = x0 < w2 - 1 ? 1 : 0;
        pp = prev + (size_t)n * 64 * h * w2 + (size_t)y0 * w2 + x0;
    }
    __device__ __forceinline__ void load8(int c0, float* v) const {
        const size_t hw = (size_t)h * w2;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + k;
            const float* q = pp + (size_t)c * hw;
            const float up = (1.0f - ly) * ((1.0f - lx) * q[0] + lx * q[dx]) + ly * ((1.0f - lx) * q[dy] + lx * q[dy + dx]);
            float s = b[c];
#pragma unroll
            for (int ci = 0; ci < CLAT; ++ci) s = fmaf(w[c * CLAT + ci], l[ci], s);
            v[k] = up + s;
        }
    }
};

__device__ __forceinline__ float fp_act(float t, int act) {
    if (act == 1) return t / (1.0f + expf(-t));               // Swish (module.py Swish: x * sigmoid(x))
    if (act == 2) return t > 0.0f ? t : 0.1f * t;             // F.leaky_relu(y, 0.1) (module.py Conv2d)
    return t;
}

template <int CIN, int K, int S>
struct FpnShape {
    static constexpr int CINP = (CIN + 7) / 8 * 8;
    static constexpr int CH = S == 1 ? (CINP < 32 ? CINP : 32) : 8;           // channels staged per pass (packing.fpn_chunk)
    static constexpr int OPT = CH / 8, NPASS = CINP / CH, NOCT = K * K * OPT, NSTEP = (NOCT + 3) / 4;
    static constexpr int IH = (FP_TH - 1) * S + K, IW = (FP_TW - 1) * S + K, NPIX = IH * IW;
    static constexpr int PLANE = NPIX * 32 + 32;                               // bytes of one octet plane (+ one slot: bank rows differ)
    static constexpr size_t LDS = (size_t)OPT * PLANE;
};

template <int CIN, int COUT, int K, int S, class Src>
__global__ __launch_bounds__(256) void fpn_conv_kernel(Src src, const void* __restrict__ wp, const float* __restrict__ bias, int act,
                                                       float* __restrict__ out, int H, int W, int OH, int OW, int tiles_x, int ntiles) {
    typedef FpnShape<CIN, K, S> F;
    constexpr int OPT = F::OPT, NOCT = F::NOCT, NSTEP = F::NSTEP, IW = F::IW, NPIX = F::NPIX, P = K / 2;
    constexpr int MREP = (COUT + 15) / 16, NREP = FP_TW / 16;
    constexpr int UNROLL = MREP >= 4 ? 3 : NSTEP;                 // 64 output channels: a full unroll hoists weight loads into spills
    HIP_DYNAMIC_SHARED(float4, lds4)
    char* ldsb = reinterpret_cast<char*>(lds4);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int tile = (int)xcd_remap(blockIdx.x, (unsigned)ntiles), n = (int)blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * FP_TH, x0 = tx * FP_TW;

    f32x4 acc[MREP][NREP];
#pragma unroll
    for (int mb = 0; mb < MREP; ++mb)
#pragma unroll
        for (int nb = 0; nb < NREP; ++nb) acc[mb][nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    for (int pass = 0; pass < F::NPASS; ++pass) {
        if (pass > 0) __syncthreads();                            // every wave has read the previous pass's image
        // ---- stage: one work-item = one staged pixel (all OPT octets of the pass); consecutive work-items = consecutive pixels ----
        for (int pix = tid; pix < NPIX; pix += 256) {
            const int iy = pix / IW, ix = pix - iy * IW;
            const int gy = y0 * S - P + iy, gx = x0 * S - P + ix;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;          // zero padding (padding = k/2) outside the image
            Src s = src;
            if (inside) s.at(n, gy, gx);
#pragma unroll
            for (int oc = 0; oc < OPT; ++oc) {
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
            const bool live = q < NOCT;                           // the last step may run past the K x K x OPT octets: zero operand
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
                for (int nb = 0; nb < NREP; ++nb) {
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mb], bh[nb], acc[mb][nb], 0, 0, 0);
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mb], bl[nb], acc[mb][nb], 0, 0, 0);
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mb], bh[nb], acc[mb][nb], 0, 0, 0);
                }
        }
    }

    // ---- epilogue: lane (pixel li, group g) holds output channels 16 mb + 4 g .. + 3 of its pixel: bias (folded BatchNorm shift),
    //      activation, planar fp32 stores (16 consecutive pixels of one channel per lane group: 64 contiguous bytes) ----
    const int y = y0 + wave;
    if (y >= OH) return;
    const size_t ohw = (size_t)OH * OW;
    float* ob = out + (size_t)n * COUT * ohw + (size_t)y * OW;
#pragma unroll
    for (int nb = 0; nb < NREP; ++nb) {
        const int xx = x0 + nb * 16 + li;
        if (xx >= OW) continue;
#pragma unroll
        for (int mb = 0; mb < MREP; ++mb) {
            const int co = 16 * mb + 4 * g;
            if (co >= COUT) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) ob[(size_t)(co + k) * ohw + xx] = fp_act(acc[mb][nb][k] + (bias ? bias[co + k] : 0.0f), act);
        }
    }
}

template <int CLAT>
__global__ __launch_bounds__(256) void fpn_merge_kernel(MergeSrc<CLAT> src, float* __restrict__ out, int N) {
    const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), n = (int)blockIdx.z;
    if (x >= src.W || y >= src.H || n >= N) return;
    MergeSrc<CLAT> s = src;
    s.at(n, y, x);
    const size_t HW = (size_t)src.H * src.W;
    float* o = out + (size_t)n * 64 * HW + (size_t)y * src.W + x;
#pragma unroll 1
    for (int c0 = 0; c0 < 64; c0 += 8) {
        float v[8];
        s.load8(c0, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[(size_t)(c0 + k) * HW] = v[k];
    }
}

template <int CIN, int COUT, int K, int S, class Src>
static int launch_fpn_conv(const Src& src, const void* wp, const float* bias, int act, float* out, int N, int H, int W, hipStream_t st) {
    typedef FpnShape<CIN, K, S> F;
    const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;                      // padding k/2, odd k
    const int tiles_x = (int)ceil_div(OW, FP_TW), tiles_y = (int)ceil_div(OH, FP_TH);
    if (F::LDS > 48 * 1024)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fpn_conv_kernel<CIN, COUT, K, S, Src>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
    hipLaunchKernelGGL((fpn_conv_kernel<CIN, COUT, K, S, Src>), dim3(tiles_x * tiles_y, N), dim3(256), F::LDS, st, src, wp, bias, act, out, H, W, OH, OW,
                       tiles_x, tiles_x * tiles_y);
    return check_launch("fpn_conv_kernel");
}

template <int CLAT>
static MergeSrc<CLAT> merge_src(const float* prev, const float* lat, const float* w, const float* b, int H, int W) {
    MergeSrc<CLAT> s{};
    s.prev = prev; s.lat = lat; s.w = w; s.b = b;
    s.H = H; s.W = W; s.h = H / 2; s.w2 = W / 2;
    s.sy = H > 1 ? (float)(s.h - 1) / (float)(H - 1) : 0.0f;
    s.sx = W > 1 ? (float)(s.w2 - 1) / (float)(W - 1) : 0.0f;
    return s;
}

}  // namespace mvs

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
    hipStream_t st = (hipStream_t)stream;
    PlanarSrc src{x, Cin, H, W, nullptr};
#define MVS_FPN_GO(CI, CO, KK, SS) \
    if (Cin == CI && Cout == CO && k == KK && stride == SS) return launch_fpn_conv<CI, CO, KK, SS>(src, w_packed, bias, act, y, N, H, W, st);
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
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(W, 64), ceil_div(H, 4), N);
#define MVS_FPN_MG(CL) \
    if (Clat == CL) { \
        hipLaunchKernelGGL((fpn_merge_kernel<CL>), grid, dim3(256), 0, st, merge_src<CL>(prev, lateral, w_inner, b_inner, H, W), intra, N); \
        return check_launch("fpn_merge_kernel"); \
    }
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
    return launch_fpn_conv<64, 8, 3, 1>(merge_src<8>(prev, lateral, w_inner, b_inner, H, W), w_packed, bias, act, y, N, H, W, (hipStream_t)stream);
}
