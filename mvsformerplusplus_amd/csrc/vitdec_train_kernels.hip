// Training of the CrossVITDecoder's blocks: what the backward of a CrossBlock at d_model 768 needs beside the
// forward's own launches (vitdec_kernels.hip), fp32-equivalent.
//
// Kernels:
//   1. vd_wgrad_kernel: the weight gradient of a linear layer over tokens, dw[N, K] = sum_m dy[m, n] x[m, k] (and dbias[n] = sum_m dy[m, n]),
//      from dy [M, N] and x [M, K], both fp32 and token-major.  The contraction index is the TOKEN, so an MFMA lane wants 8 consecutive
//      tokens of one channel: the transpose of the forward's packed-split rows.  A workgroup (2 x 2 waves, wave = 64 x 64 of a 128 x 128
//      tile of dw) stages 32 tokens at a time: thread t reads channel t & 127 of tokens 8 o .. 8 o + 7 for the two octets o = 2 (t >> 7),
//      2 (t >> 7) + 1 (4-byte loads, a wave's lanes on 64 consecutive channels of one token row), splits the eight values into hi + lo
//      bf16 (split_format.h) and writes them as ONE 16-byte piece in the order the lanes read them,
//          lds[channel >> 4][hi|lo][lane = octet * 16 + (channel & 15)]           (conflict-free ds_write_b128 / ds_read_b128)
//      Products are the three-term ones of the forward (mfma3_bf16), fp32 accumulate, tokens ascending.  The next 32 tokens' global
//      loads are in flight during the MFMAs.  Tokens past M contribute zero from a branch, never from an out-of-range load.
//      grid = (token slabs, K / 128, N / 128): every workgroup writes its partial tile to the workspace and fmt_partial_reduce_kernel
//      (partial_reduce.h) adds the slabs in slab order: no atomics, no arrival counters, bit-identical run to run.  A launch of one slab
//      writes dw and dbias directly.
//   2. vd_ln_bwd_kernel: LayerNorm backward over rows of 768, one wave per row (the row layout of vd_rows_kernel): mean and rstd are
//      recomputed, d_x = rstd (g - mean(g) - xhat mean(g xhat)) [+ add], g = w d_y; d_w = sum_rows d_y xhat and d_b = sum_rows d_y are
//      kept per wave over the rows it walks (stride = the grid), the four waves of a workgroup are added in wave order and the
//      per-workgroup partials by fmt_partial_reduce_kernel.
//   3. vd_pack_kernel: fp32 [M, C] -> the packed-split row operand of vd_gemm_kernel (a gradient on its way into a data-gradient GEMM,
//      which is mvs_vitdec_linear_fwd on the transposed weight).
#include "mvs_common.h"
#include "partial_reduce.h"
#include "split_format.h"
#include "vit_split.h"

namespace mvs {

constexpr int VW_C = 768;
constexpr int VW_T = 128;                     // dw tile: 128 output channels (n) x 128 input channels (k)
constexpr int VW_TOK = 32;                    // tokens per staged chunk = one MFMA k-step
constexpr int VW_TARGET = 512;                // workgroups wanted in a launch: two per compute unit
constexpr int VW_LN_MAXWG = 512;

// slabs of whole 32-token chunks: enough for VW_TARGET workgroups over the launch's tiles, never more than there are chunks
static void vw_slabs(long long M, int N, int K, int& slabs, int& chunks_per_slab) {
    const int chunks = (int)ceil_div(M, VW_TOK), tiles = (N / VW_T) * (K / VW_T);
    int want = (int)ceil_div(VW_TARGET, tiles);
    if (want > chunks) want = chunks;
    chunks_per_slab = (int)ceil_div(chunks, want);
    slabs = (int)ceil_div(chunks, chunks_per_slab);
}

__global__ __launch_bounds__(256) void vd_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part,
                                                       float* __restrict__ bpart, int M, int N, int K, int tok_per_slab) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    bf16x8* ly = reinterpret_cast<bf16x8*>(lds4);                 // [8 channel blocks][hi|lo][64 lanes]: dy
    bf16x8* lx = ly + 8 * 128;                                    // the same for x
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int wn = wave >> 1, wk = wave & 1;
    const int slab = (int)blockIdx.x, k0 = (int)blockIdx.y * VW_T, n0 = (int)blockIdx.z * VW_T;
    const int t0 = slab * tok_per_slab, t1 = t0 + tok_per_slab < M ? t0 + tok_per_slab : M;
    const int c = tid & 127, o0 = (tid >> 7) * 2;                 // staged channel of the tile, first of this thread's two token octets
    const float* ysrc = dy + n0 + c;
    const float* xsrc = x + k0 + c;
    float ry[16], rx[16];
    float bsum = 0.0f;

    auto fetch = [&](int t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tok = t + 8 * o0 + e;
            const bool ok = tok < t1;
            ry[e] = ok ? ysrc[(size_t)tok * N] : 0.0f;
            rx[e] = ok ? xsrc[(size_t)tok * K] : 0.0f;
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    fetch(t0);
#pragma unroll 1
    for (int t = t0; t < t1; t += VW_TOK) {
        __syncthreads();                                           // the previous chunk has been read
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            float vy[8], vx[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                vy[e] = ry[8 * o + e];
                vx[e] = rx[8 * o + e];
                bsum += vy[e];
            }
            bf16x8 hi, lo;
            const int piece = (c >> 4) * 128 + (o0 + o) * 16 + (c & 15);
            split8(vy, hi, lo);
            ly[piece] = hi;
            ly[piece + 64] = lo;
            split8(vx, hi, lo);
            lx[piece] = hi;
            lx[piece + 64] = lo;
        }
        __syncthreads();
        if (t + VW_TOK < t1) fetch(t + VW_TOK);                    // in flight during the MFMAs below
        bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            ah[a] = ly[(wn * 4 + a) * 128 + lane];
            al[a] = ly[(wn * 4 + a) * 128 + 64 + lane];
            bh[a] = lx[(wk * 4 + a) * 128 + lane];
            bl[a] = lx[(wk * 4 + a) * 128 + 64 + lane];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = mfma3_bf16(ah[a], al[a], bh[b], bl[b], acc[a][b]);
    }

    // ---- partial tile: lane (li, g) holds dw[n = 16 a + 4 g + r][k = 16 b + li] ----
    float* dst = part + (size_t)slab * N * K;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* row = dst + (size_t)(n0 + wn * 64 + 16 * a + 4 * g + r) * K + k0 + wk * 64 + li;
#pragma unroll
            for (int b = 0; b < 4; ++b) row[16 * b] = acc[a][b][r];
        }
    // ---- bias partial: the workgroups of the first K tile; the two thread halves hold the two octet pairs of a chunk ----
    if (bpart && blockIdx.y == 0) {
        float* red = reinterpret_cast<float*>(lds4);
        __syncthreads();
        if (tid >= 128) red[c] = bsum;
        __syncthreads();
        if (tid < 128) bpart[(size_t)slab * N + n0 + c] = bsum + red[c];
    }
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
    return M >= 1 && M < (1LL << 24) && N >= VW_T && K >= VW_T && N % VW_T == 0 && K % VW_T == 0 && N <= 8192 && K <= 8192;
}

extern "C" size_t mvs_vitdec_wgrad_workspace_bytes(long long M, int N, int K) {
    if (!vw_shape(M, N, K)) return 0;
    int slabs, per;
    vw_slabs(M, N, K, slabs, per);
    return (size_t)slabs * ((size_t)N * K + N) * sizeof(float);
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
    int slabs, per;
    vw_slabs(M, N, K, slabs, per);
    hipStream_t st = (hipStream_t)stream;
    // one slab: its "partial" is the result, written in place with no second launch
    float* part = slabs == 1 ? dw : reinterpret_cast<float*>(workspace);
    float* bpart = !dbias ? nullptr : (slabs == 1 ? dbias : reinterpret_cast<float*>(workspace) + (size_t)slabs * N * K);
    hipLaunchKernelGGL(vd_wgrad_kernel, dim3(slabs, K / VW_T, N / VW_T), dim3(256), 2 * 8 * 128 * sizeof(bf16x8), st, dy, x, part, bpart, (int)M, N,
                       K, per * VW_TOK);
    int rc = check_launch("vd_wgrad_kernel");
    if (rc != MVS_OK || slabs == 1) return rc;
    rc = ft_reduce_partials(part, dw, slabs, N * K, st);
    if (rc != MVS_OK || !dbias) return rc;
    return ft_reduce_partials(bpart, dbias, slabs, N, st);
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
