// Training of the CrossVITDecoder's blocks: what the backward of a CrossBlock at d_model 768 needs beside the
// forward's own launches (vitdec_kernels.hip), fp32-equivalent.
//
// Kernels:
//   1. vd_wgrad_kernel: the weight gradient of a linear layer over tokens, dw[N, K] = sum_m dy[m, n] x[m, k] (and dbias[n] = sum_m dy[m, n]),
//      from dy [M, N] and x [M, K], both fp32 and token-major: the token weight gradient of token_wgrad.h with the identity map and
//      the bias partial.
//   2. vd_ln_bwd_kernel: LayerNorm backward over rows of 768, one wave per row (the row layout of vd_rows_kernel): mean and rstd are
//      recomputed, d_x = rstd (g - mean(g) - xhat mean(g xhat)) [+ add], g = w d_y; d_w = sum_rows d_y xhat and d_b = sum_rows d_y are
//      kept per wave over the rows it walks (stride = the grid), the four waves of a workgroup are added in wave order and the
//      per-workgroup partials by fmt_partial_reduce_kernel.
//   3. vd_pack_kernel: fp32 [M, C] -> the packed-split row operand of vd_gemm_kernel (a gradient on its way into a data-gradient GEMM,
//      which is mvs_vitdec_linear_fwd on the transposed weight).
#include "mvs_common.h"
#include "partial_reduce.h"
#include "split_format.h"
#include "token_wgrad.h"
#include "vit_split.h"

namespace mvs {

constexpr int VW_C = 768;
constexpr int VW_LN_MAXWG = 512;

__global__ __launch_bounds__(256) void vd_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part,
                                                       float* __restrict__ bpart, int M, int N, int K, int tok_per_slab) {
    token_wgrad<true>(TwMap<TW_IDENTITY>{dy, x, N, K, 1, 1, 0}, part, bpart, M, N, K, tok_per_slab);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// LayerNorm backward
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vw_wave_sum(float s) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    return s;
}

// part [gridDim.x][2][768]: d_w | d_b of the rows this workgroup walked
__global__ __launch_bounds__(256) void vd_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ add, float* __restrict__ dx, float* __restrict__ part, int M,
                                                        float eps) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* red = reinterpret_cast<float*>(lds4);                  // [3 waves][2][768]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float aw[3][4], ab[3][4], ww[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 t = *reinterpret_cast<const float4*>(w + 4 * (lane + 64 * j));
        ww[j][0] = t.x; ww[j][1] = t.y; ww[j][2] = t.z; ww[j][3] = t.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) aw[j][k] = ab[j][k] = 0.0f;
    }
#pragma unroll 1
    for (int r = (int)blockIdx.x * 4 + wave; r < M; r += (int)gridDim.x * 4) {        // wave-uniform
        float v[3][4], d[3][4];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 a = *reinterpret_cast<const float4*>(x + (size_t)r * VW_C + 4 * (lane + 64 * j));
            const float4 b = *reinterpret_cast<const float4*>(dy + (size_t)r * VW_C + 4 * (lane + 64 * j));
            v[j][0] = a.x; v[j][1] = a.y; v[j][2] = a.z; v[j][3] = a.w;
            d[j][0] = b.x; d[j][1] = b.y; d[j][2] = b.z; d[j][3] = b.w;
        }
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        const float mean = vw_wave_sum(s) * (1.0f / VW_C);
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float t = v[j][k] - mean;
                q = fmaf(t, t, q);
            }
        const float rstd = 1.0f / sqrtf(vw_wave_sum(q) * (1.0f / VW_C) + eps);
        float sg = 0.0f, sgx = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xh = (v[j][k] - mean) * rstd, gg = ww[j][k] * d[j][k];
                v[j][k] = xh;
                aw[j][k] = fmaf(d[j][k], xh, aw[j][k]);
                ab[j][k] += d[j][k];
                d[j][k] = gg;
                sg += gg;
                sgx = fmaf(gg, xh, sgx);
            }
        const float mg = vw_wave_sum(sg) * (1.0f / VW_C), mgx = vw_wave_sum(sgx) * (1.0f / VW_C);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = rstd * (d[j][k] - mg - v[j][k] * mgx);
            if (add) {
                const float4 a = *reinterpret_cast<const float4*>(add + (size_t)r * VW_C + 4 * (lane + 64 * j));
                o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w;
            }
            *reinterpret_cast<float4*>(dx + (size_t)r * VW_C + 4 * (lane + 64 * j)) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    // waves 1 .. 3 leave their sums in LDS, wave 0 adds them in wave order
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                red[((wave - 1) * 2 + 0) * VW_C + 4 * (lane + 64 * j) + k] = aw[j][k];
                red[((wave - 1) * 2 + 1) * VW_C + 4 * (lane + 64 * j) + k] = ab[j][k];
            }
    }
    __syncthreads();
    if (wave == 0) {
        float* dst = part + (size_t)blockIdx.x * 2 * VW_C;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ch = 4 * (lane + 64 * j) + k;
                float sw = aw[j][k], sb = ab[j][k];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    sw += red[(u * 2 + 0) * VW_C + ch];
                    sb += red[(u * 2 + 1) * VW_C + ch];
                }
                dst[ch] = sw;
                dst[VW_C + ch] = sb;
            }
    }
}

// fp32 [M, C] -> packed-split rows (vit_split.h): one thread per four channels
__global__ __launch_bounds__(256) void vd_pack_kernel(const float* __restrict__ x, bf16x8* __restrict__ out, int M, int C) {
    const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
    const int quads = C >> 2;
    if (i >= (long long)M * quads) return;
    const int row = (int)(i / quads), ch = (int)(i - (long long)row * quads) * 4;
    const float4 t = *reinterpret_cast<const float4*>(x + (size_t)row * C + ch);
    const float v[4] = {t.x, t.y, t.z, t.w};
    vd_store_split4(out, C >> 5, row, ch, v);
}

static int vw_ln_groups(long long M) {
    const long long g = (M + 3) / 4;
    return (int)(g < VW_LN_MAXWG ? g : VW_LN_MAXWG);
}

}  // namespace mvs

using namespace mvs;

static bool vw_shape(long long M, int N, int K) {
    return M >= 1 && M < (1LL << 24) && N >= TW_T && K >= TW_T && N % TW_T == 0 && K % TW_T == 0 && N <= 8192 && K <= 8192;
}

extern "C" size_t mvs_vitdec_wgrad_workspace_bytes(long long M, int N, int K) {
    return vw_shape(M, N, K) ? token_wgrad_workspace_bytes(M, N, K, true) : 0;
}

extern "C" int mvs_vitdec_wgrad(const float* dy, const float* x, float* dw, float* dbias, void* workspace, size_t workspace_bytes, long long M,
                                int N, int K, void* stream) {
    if (!vw_shape(M, N, K)) {
        set_error("mvs_vitdec_wgrad: built for token-major fp32 dy [M, N] and x [M, K] with N and K multiples of 128 (the CrossBlock linears: "
                  "N = 768 | 1536 | 3072, K = 768 | 3072) and 1 <= M < 2^24 [block.py:294-329]; got M = %lld, N = %d, K = %d", M, N, K);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!dy || !x || !dw || !workspace) {
        set_error("mvs_vitdec_wgrad: bad arguments");
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_vitdec_wgrad_workspace_bytes(M, N, K)) {
        set_error("mvs_vitdec_wgrad: workspace smaller than mvs_vitdec_wgrad_workspace_bytes");
        return MVS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](dim3 grid, float* part, float* bpart, int tok_per_slab) {
        hipLaunchKernelGGL(vd_wgrad_kernel, grid, dim3(256), TW_LDS, st, dy, x, part, bpart, (int)M, N, K, tok_per_slab);
    };
    return token_wgrad_run("vd_wgrad_kernel", launch, dw, dbias, workspace, M, N, K, st);
}

extern "C" size_t mvs_vitdec_ln_bwd_workspace_bytes(long long M, int channels) {
    if (M < 1 || M >= (1LL << 24) || channels != VW_C) return 0;
    return (size_t)vw_ln_groups(M) * 2 * VW_C * sizeof(float);
}

extern "C" int mvs_vitdec_ln_bwd(const float* d_y, const float* x, const float* w, float eps, const float* add, float* d_x, float* d_wb,
                                 void* workspace, size_t workspace_bytes, long long M, int channels, void* stream) {
    if (channels != VW_C) {
        set_error("mvs_vitdec_ln_bwd: built for rows of 768 channels (decoder_cfg d_model) [module.py:306]; got %d", channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!d_y || !x || !w || !d_x || !d_wb || !workspace || M < 1 || M >= (1LL << 24) || !(eps > 0.0f) ||
        workspace_bytes < mvs_vitdec_ln_bwd_workspace_bytes(M, channels)) {
        set_error("mvs_vitdec_ln_bwd: bad arguments (the workspace is mvs_vitdec_ln_bwd_workspace_bytes)");
        return MVS_ERR_ARG;
    }
    const int groups = vw_ln_groups(M);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vd_ln_bwd_kernel, dim3(groups), dim3(256), 3 * 2 * VW_C * sizeof(float), st, d_y, x, w, add, d_x,
                       reinterpret_cast<float*>(workspace), (int)M, eps);
    int rc = check_launch("vd_ln_bwd_kernel");
    if (rc != MVS_OK) return rc;
    return ft_reduce_partials(reinterpret_cast<const float*>(workspace), d_wb, groups, 2 * VW_C, st);
}

extern "C" int mvs_vitdec_pack_fwd(const float* x, void* x_packed, long long M, int channels, void* stream) {
    if (channels != VW_C && channels != 2 * VW_C && channels != 4 * VW_C) {
        set_error("mvs_vitdec_pack_fwd: built for rows of 768, 1536 or 3072 channels (the row operands of the CrossBlock's data-gradient "
                  "GEMMs) [block.py:294-329]; got %d", channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!x || !x_packed || M < 1 || M >= (1LL << 24)) {
        set_error("mvs_vitdec_pack_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    hipLaunchKernelGGL(vd_pack_kernel, dim3(ceil_div(M * (channels / 4), 256)), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<bf16x8*>(x_packed), (int)M, channels);
    return check_launch("vd_pack_kernel");
}
