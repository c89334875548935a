// FMT_with_pathway: the stage-1 linear-attention transformer and the three-level pathway of the shipped
// network, fp32-equivalent.
//
// Reference (restated, never copied): models/FMT.py:35-206 (FMT, FMT_with_pathway), models/dino/layers/block.py (CrossBlock, pre-norm,
// LayerScale), models/dino/layers/attention.py (CrossLinearAttention: q = elu(Wq x) + 1, k = elu(Wk kv) + 1, v = Wv kv,
// KV_h = sum_s k_s (x) v_s, a = (q . KV_h) / (q . sum_s k_s + 1e-6)), models/dino/layers/mlp.py (fc1, GELU (erf), fc2).
//
// Layout.  Tokens stay PLANAR: a token tensor is [N, 64, n] fp32 (n = h w), i.e. the feature map itself, so there is no transpose on
// the way in or out.  Every GEMM puts the tokens on the MFMA's column (or row) index = the lane: lane (li = lane & 15, g = lane >> 4)
// of a wave owns token t0 + 16 nb + li (nb < FT_NREP) and, in the ACCUMULATOR LAYOUT, its channels 16 mb + 4 g + k (mb = 16-channel
// block, k < 4).  A v_mfma_f32_16x16x32_bf16 result (rows = output channels, columns = tokens) is already in that layout, and it is the
// next GEMM's B operand with no data movement: the 8 elements of k-step s are the registers of blocks 2s and 2s+1, i.e. k-slot
// (s, g, e) holds channel 32 s + 16 (e >> 2) + 4 g + (e & 3).  The weights are packed with the same permutation of their input
// channels (packing.pack_fmt_linear), so a whole block - LayerNorm, q, the per-head apply, proj, LayerNorm, fc1, GELU, fc2, both
// residuals - runs in registers; neither q, a nor the 256-wide hidden activation touches LDS or HBM.  Every product is the three-term
// split-bf16 one (hi*hi + hi*lo + lo*hi, fp32 accumulate); LayerNorm statistics, elu, the normaliser, GELU and the residuals are fp32.
//
// Kernels:
//   1. fmt_kv_partial_kernel + fmt_kv_reduce_kernel: LN1 -> k, v (tokens on the MFMA ROW index, so that a lane group holds four
//      tokens of one channel) -> KV_h += k^T v over the tokens on the exact-fp32 v_mfma_f32_16x16x4_f32; per-workgroup partials, added in a
//      fixed order by the second launch (no atomics: bit-identical run to run), which also writes the result as a packed split-bf16
//      operand: a [80 x 64] matrix = block-diagonal KV_h^T plus four rows of sum_s k_s per lane group, so that the apply and the
//      normaliser are one more GEMM of the block kernel.
//   2. fmt_block_kernel: one CrossBlock for 32 tokens per wave; packed weights stream from L2 in lane order (164 KB for the four
//      matrices + the 20 KB key/value operand exceed the LDS; each wave reads them once per 32 tokens).
//   3. the pathway (reported as fmt_path_kernel): smooth_k(bilinear(dim_reduction_k(prev)) + lateral) = the shared implicit-GEMM 3x3
//      conv2d_split_kernel<C, C, 3, 1, FtMergeSrc<C>, PlanarSink<false>> (conv2d_split.h) whose staging evaluates the merged map for the tile
//      and its halo (align_corners=False, any size ratio, no biases); the merged map is never written.  fmt_merge_kernel
//      (conv2d_source_kernel on FtMergeSrc) + the same convolution on PlanarSrc are the unfused form.
//   4. the pathway's backward (further down): fmt_path_bwd_kernel (the interpolation's adjoint as a gather, d prev,
//      the partials of d W_r), fmt_smooth_wgrad_kernel (d S on v_mfma_f32_16x16x4_f32 with the merged map re-evaluated in LDS) and
//      fmt_partial_reduce_kernel (fixed-order sum of the partials, partial_reduce.h).  The blocks' backward is not in this file (training.py).
// Staged positions are clamped to the image explicitly (zero padding from a branch, never from an out-of-range load).
#include "conv2d_split.h"
#include "partial_reduce.h"

namespace mvs {

constexpr int FT_NREP = 2;                    // 16-token column blocks per wave
constexpr int FT_TOK = 16 * FT_NREP;          // tokens per wave
// packed weights, in bf16x8 (16-byte) units: linear [step][mb][hi|lo][64 lanes] (packing.pack_fmt_block)
constexpr int FT_W_Q = 0, FT_W_P = 1024, FT_W_1 = 2048, FT_W_2 = 6144, FT_W_KV = 10240, FT_W_END = 12288;
// fp32 vectors (packing.pack_fmt_block)
constexpr int FT_V_LN1W = 0, FT_V_LN1B = 64, FT_V_BP = 128, FT_V_G1 = 192, FT_V_LN2W = 256, FT_V_LN2B = 320, FT_V_B1 = 384, FT_V_B2 = 640,
              FT_V_G2 = 704, FT_V_END = 768;
constexpr int FT_KVOP = 2 * 5 * 2 * 64;       // bf16x8 units of one key/value operand ([2 steps][5 row blocks][hi|lo][64 lanes])
constexpr int FT_PART = 1280;                 // floats of one partial: KV [4][16][16] | per-lane-group sums of k [4][4][16]
constexpr int FT_MAX_SLABS = 64;      // partials per view: the second launch adds them one after the other (a dependent load each)

__device__ __forceinline__ void ft_operand(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& lo) {
    split8(make_float4(a[0], a[1], a[2], a[3]), make_float4(b[0], b[1], b[2], b[3]), hi, lo);
}

// the wave's tokens in the accumulator layout (+ the position encoding table [64, n]); tokens past the end read as zero
__device__ __forceinline__ void ft_load(const float* __restrict__ xn, const float* __restrict__ pe, int ntok, int t0, int li, int g,
                                        f32x4 (&x)[4][FT_NREP]) {
#pragma unroll
    for (int nb = 0; nb < FT_NREP; ++nb) {
        const int tok = t0 + nb * 16 + li;
        const bool ok = tok < ntok;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t o = (size_t)(16 * mb + 4 * g + k) * ntok + tok;
                float v = 0.0f;
                if (ok) {
                    v = xn[o];
                    if (pe) v += pe[o];
                }
                x[mb][nb][k] = v;
            }
    }
}

// LayerNorm(64, eps 1e-5) of every token (its 64 channels sit in the four lanes li, li + 16, li + 32, li + 48) -> split operands
__device__ __forceinline__ void ft_layernorm(const f32x4 (&x)[4][FT_NREP], const float* __restrict__ w, const float* __restrict__ b, int g,
                                             bf16x8 (&oh)[2][FT_NREP], bf16x8 (&ol)[2][FT_NREP]) {
    float4 wv[4], bv[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        wv[mb] = *reinterpret_cast<const float4*>(w + 16 * mb + 4 * g);
        bv[mb] = *reinterpret_cast<const float4*>(b + 16 * mb + 4 * g);
    }
#pragma unroll
    for (int nb = 0; nb < FT_NREP; ++nb) {
        float s = 0.0f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) s += (x[mb][nb][0] + x[mb][nb][1]) + (x[mb][nb][2] + x[mb][nb][3]);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * (1.0f / 64.0f);
        float q = 0.0f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = x[mb][nb][k] - mean;
                q = fmaf(d, d, q);
            }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        const float rstd = 1.0f / sqrtf(q * (1.0f / 64.0f) + 1e-5f);
        f32x4 y[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const float ww[4] = {wv[mb].x, wv[mb].y, wv[mb].z, wv[mb].w}, bb[4] = {bv[mb].x, bv[mb].y, bv[mb].z, bv[mb].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) y[mb][k] = fmaf((x[mb][nb][k] - mean) * rstd, ww[k], bb[k]);
        }
        ft_operand(y[0], y[1], oh[0][nb], ol[0][nb]);
        ft_operand(y[2], y[3], oh[1][nb], ol[1][nb]);
    }
}

// acc[mb][nb] += W[rows 16 (mb0 + mb) ..][k-steps s0 .. s0 + NSTEP) . operand; wl = packed linear + lane, MTOT = its row blocks
template <int MREP, int NSTEP, int MTOT>
__device__ __forceinline__ void ft_gemm(const bf16x8* __restrict__ wl, int s0, int mb0, const bf16x8 (&bh)[NSTEP][FT_NREP],
                                        const bf16x8 (&bl)[NSTEP][FT_NREP], f32x4 (&acc)[MREP][FT_NREP]) {
#pragma unroll
    for (int s = 0; s < NSTEP; ++s)
#pragma unroll
        for (int mb = 0; mb < MREP; ++mb) {
            const bf16x8 ah = wl[(size_t)((((s0 + s) * MTOT + mb0 + mb) * 2 + 0) * 64)];
            const bf16x8 al = wl[(size_t)((((s0 + s) * MTOT + mb0 + mb) * 2 + 1) * 64)];
#pragma unroll
            for (int nb = 0; nb < FT_NREP; ++nb) acc[mb][nb] = mfma3_bf16(ah, al, bh[s][nb], bl[s][nb], acc[mb][nb]);
        }
}

template <int MREP>
__device__ __forceinline__ void ft_zero(f32x4 (&acc)[MREP][FT_NREP]) {
#pragma unroll
    for (int mb = 0; mb < MREP; ++mb)
#pragma unroll
        for (int nb = 0; nb < FT_NREP; ++nb) acc[mb][nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
}

struct FmtBlockArgs {
    const float* x;          // [N, 64, n]
    const float* pe;         // [64, n] added to x first (nullable)
    const bf16x8* kvop;      // [N / kv_div] key/value operands
    const bf16x8* w;         // packed weights
    const float* vec;        // LayerNorm / bias / layer-scale vectors
    float* out;              // [N, 64, n]
    int ntok, kv_div;
};

__global__ __launch_bounds__(256) void fmt_block_kernel(FmtBlockArgs a) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int n = (int)blockIdx.y, ntok = a.ntok;
    const int t0 = ((int)blockIdx.x * 4 + wave) * FT_TOK;
    if (t0 >= ntok) return;                                       // wave-uniform; the kernel has no workgroup barrier
    const bf16x8* wl = a.w + lane;
    const float* vec = a.vec;

    f32x4 x[4][FT_NREP];
    ft_load(a.x + (size_t)n * 64 * ntok, a.pe, ntok, t0, li, g, x);
    bf16x8 bh[2][FT_NREP], bl[2][FT_NREP];
    f32x4 acc[4][FT_NREP];

    // ---- attention: q = elu(Wq LN1(x)) + 1 ----
    ft_layernorm(x, vec + FT_V_LN1W, vec + FT_V_LN1B, g, bh, bl);
    ft_zero<4>(acc);
    ft_gemm<4, 2, 4>(wl + FT_W_Q, 0, 0, bh, bl, acc);
#pragma unroll
    for (int nb = 0; nb < FT_NREP; ++nb) {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[mb][nb][k] = elu1(acc[mb][nb][k]);
        ft_operand(acc[0][nb], acc[1][nb], bh[0][nb], bl[0][nb]);
        ft_operand(acc[2][nb], acc[3][nb], bh[1][nb], bl[1][nb]);
    }
    // ---- a = (q . KV_h) / (q . ksum_h + 1e-6): rows 0..63 of the operand are the heads' KV_h^T, row 64 + 4 g' + h is ksum_h ----
    {
        f32x4 ap[5][FT_NREP];
        ft_zero<5>(ap);
        ft_gemm<5, 2, 5>(a.kvop + (size_t)(n / a.kv_div) * FT_KVOP + lane, 0, 0, bh, bl, ap);
#pragma unroll
        for (int nb = 0; nb < FT_NREP; ++nb) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                const float den = ap[4][nb][mb] + 1e-6f;
#pragma unroll
                for (int k = 0; k < 4; ++k) ap[mb][nb][k] = ap[mb][nb][k] / den;
            }
            ft_operand(ap[0][nb], ap[1][nb], bh[0][nb], bl[0][nb]);
            ft_operand(ap[2][nb], ap[3][nb], bh[1][nb], bl[1][nb]);
        }
    }
    // ---- x += ls1 * (Wp a + bp) ----
    ft_zero<4>(acc);
    ft_gemm<4, 2, 4>(wl + FT_W_P, 0, 0, bh, bl, acc);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const float4 bp = *reinterpret_cast<const float4*>(vec + FT_V_BP + 16 * mb + 4 * g);
        const float4 g1 = *reinterpret_cast<const float4*>(vec + FT_V_G1 + 16 * mb + 4 * g);
        const float bb[4] = {bp.x, bp.y, bp.z, bp.w}, gg[4] = {g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int nb = 0; nb < FT_NREP; ++nb)
#pragma unroll
            for (int k = 0; k < 4; ++k) x[mb][nb][k] = fmaf(gg[k], acc[mb][nb][k] + bb[k], x[mb][nb][k]);
    }
    // ---- x += ls2 * (W2 gelu(W1 LN2(x) + b1) + b2): 64 hidden channels at a time, each chunk is two k-steps of fc2 ----
    ft_layernorm(x, vec + FT_V_LN2W, vec + FT_V_LN2B, g, bh, bl);
    ft_zero<4>(acc);
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        f32x4 hd[4][FT_NREP];
        bf16x8 hh[2][FT_NREP], hl[2][FT_NREP];
        ft_zero<4>(hd);
        ft_gemm<4, 2, 16>(wl + FT_W_1, 0, 4 * c, bh, bl, hd);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const float4 b1 = *reinterpret_cast<const float4*>(vec + FT_V_B1 + 64 * c + 16 * mb + 4 * g);
            const float bb[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int nb = 0; nb < FT_NREP; ++nb)
#pragma unroll
                for (int k = 0; k < 4; ++k) hd[mb][nb][k] = gelu_erf(hd[mb][nb][k] + bb[k]);
        }
#pragma unroll
        for (int nb = 0; nb < FT_NREP; ++nb) {
            ft_operand(hd[0][nb], hd[1][nb], hh[0][nb], hl[0][nb]);
            ft_operand(hd[2][nb], hd[3][nb], hh[1][nb], hl[1][nb]);
        }
        ft_gemm<4, 2, 4>(wl + FT_W_2, 2 * c, 0, hh, hl, acc);
    }
    float* on = a.out + (size_t)n * 64 * ntok;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const float4 b2 = *reinterpret_cast<const float4*>(vec + FT_V_B2 + 16 * mb + 4 * g);
        const float4 g2 = *reinterpret_cast<const float4*>(vec + FT_V_G2 + 16 * mb + 4 * g);
        const float bb[4] = {b2.x, b2.y, b2.z, b2.w}, gg[4] = {g2.x, g2.y, g2.z, g2.w};
#pragma unroll
        for (int nb = 0; nb < FT_NREP; ++nb) {
            const int tok = t0 + nb * 16 + li;
            if (tok >= ntok) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                on[(size_t)(16 * mb + 4 * g + k) * ntok + tok] = fmaf(gg[k], acc[mb][nb][k] + bb[k], x[mb][nb][k]);
        }
    }
}

// Key/value summary, first launch: workgroup `slab` of view n takes the 32-token tiles slab * 4 + wave + i * (4 * slabs) and writes
// part[n][slab] = its four waves' sums, added in wave order.
__global__ __launch_bounds__(256) void fmt_kv_partial_kernel(const float* __restrict__ x, const float* __restrict__ pe, const bf16x8* __restrict__ w,
                                                             const float* __restrict__ vec, float* __restrict__ part, int ntok, int ntile) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* lds = reinterpret_cast<float*>(lds4);                  // [4 waves][FT_PART]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int n = (int)blockIdx.y, nslot = (int)gridDim.x * 4;
    const bf16x8* wl = w + FT_W_KV + lane;
    f32x4 kv[4];
    float ks[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        kv[h] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        ks[h] = 0.0f;
    }
#pragma unroll 1
    for (int tile = (int)blockIdx.x * 4 + wave; tile < ntile; tile += nslot) {
        const int t0 = tile * FT_TOK;
        f32x4 xx[4][FT_NREP];
        ft_load(x + (size_t)n * 64 * ntok, pe, ntok, t0, li, g, xx);
        bf16x8 th[2][FT_NREP], tl[2][FT_NREP];
        ft_layernorm(xx, vec + FT_V_LN1W, vec + FT_V_LN1B, g, th, tl);
        // tokens on the row index: lane (li, g) gets [token 4 g + kk of block nb][output channel 16 cb + li]; cb < 4 = k, else v
        f32x4 kacc[4][FT_NREP], vacc[4][FT_NREP];
        ft_zero<4>(kacc);
        ft_zero<4>(vacc);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                const bf16x8 wh = wl[(size_t)(((s * 8 + cb) * 2 + 0) * 64)];
                const bf16x8 wo = wl[(size_t)(((s * 8 + cb) * 2 + 1) * 64)];
#pragma unroll
                for (int nb = 0; nb < FT_NREP; ++nb) {
                    f32x4& d = cb < 4 ? kacc[cb & 3][nb] : vacc[cb & 3][nb];
                    d = mfma3_bf16(th[s][nb], tl[s][nb], wh, wo, d);
                }
            }
        // KV_h[d][m] += sum over four tokens (one per lane group) of k[token][d] v[token][m], exact fp32 products
#pragma unroll
        for (int nb = 0; nb < FT_NREP; ++nb)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bool ok = t0 + nb * 16 + 4 * g + kk < ntok;
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float kval = ok ? elu1(kacc[h][nb][kk]) : 0.0f;
                    ks[h] += kval;
                    kv[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(kval, vacc[h][nb][kk], kv[h], 0, 0, 0);
                }
            }
    }
    // lane (li = m, g) holds KV_h[d = 4 g + r][m] and the sum of k_h[.][d = li] over its lane group's tokens
    float* mine = lds + wave * FT_PART;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[h * 256 + (4 * g + r) * 16 + li] = kv[h][r];
        mine[1024 + (h * 4 + g) * 16 + li] = ks[h];
    }
    __syncthreads();
    float* dst = part + ((size_t)n * gridDim.x + blockIdx.x) * FT_PART;
    for (int e = tid; e < FT_PART; e += 256) dst[e] = ((lds[e] + lds[FT_PART + e]) + lds[2 * FT_PART + e]) + lds[3 * FT_PART + e];
}

// Second launch: block (mb, n) adds the slabs' partials of row block mb in slab order and writes that row block's 64-lane hi | lo pairs
// of both k-steps of the operand: M[16 mb + j][col] = KV_mb[col & 15][j] where col >> 4 == mb (mb < 4); M[64 + j][col] = ksum_{col >> 4}[col & 15] where
// (j & 3) == col >> 4; k-slot (step, g, e) = column 32 step + 16 (e >> 2) + 4 g + (e & 3).
__global__ __launch_bounds__(256) void fmt_kv_reduce_kernel(const float* __restrict__ part, bf16x8* __restrict__ kvop, int nslab) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* lds = reinterpret_cast<float*>(lds4);                  // [256]
    const int tid = (int)threadIdx.x, mb = (int)blockIdx.x, n = (int)blockIdx.y;
    const float* p = part + (size_t)n * nslab * FT_PART;
    float sum = 0.0f;
    if (mb < 4) {
        for (int sl = 0; sl < nslab; ++sl) sum += p[(size_t)sl * FT_PART + mb * 256 + tid];                      // [d][m]
    } else if (tid < 64) {
        const int hc = tid >> 4, d = tid & 15;
        for (int sl = 0; sl < nslab; ++sl)
            for (int gg = 0; gg < 4; ++gg) sum += p[(size_t)sl * FT_PART + 1024 + (hc * 4 + gg) * 16 + d];      // [head][d]
    }
    lds[tid] = sum;
    __syncthreads();
    if (tid >= 128) return;
    const int s = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int col = 32 * s + 16 * (e >> 2) + 4 * g + (e & 3), hc = col >> 4, d = col & 15;
        if (mb < 4) v[e] = hc == mb ? lds[d * 16 + j] : 0.0f;
        else v[e] = (j & 3) == hc ? lds[hc * 16 + d] : 0.0f;
    }
    bf16x8 hi, lo;
    split8(v, hi, lo);
    bf16x8* o = kvop + (size_t)n * FT_KVOP + (size_t)(s * 5 + mb) * 2 * 64 + lane;
    o[0] = hi;
    o[64] = lo;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// pathway: smooth_k(bilinear(dim_reduction_k(prev), size of lateral, align_corners=False) + lateral)
// ---------------------------------------------------------------------------------------------------------------------------------
// merged[c] at a pixel of the lateral = lateral[c] + sum_ci w[c][ci] * bilinear(prev[ci]); prev [N, 2C, h, w], lateral [N, C, H, W].
// The 1x1 and the interpolation are both linear and bias-free: the 2C coarse channels are interpolated once per pixel, then reduced.
// One axis of the interpolation (align_corners=False, F.interpolate(size=...)): fine index gi of a map whose coarse side has n entries,
// s = (float)n / N -> the first tap i0 and the weight l of the second tap i0 + (i0 < n - 1); the first tap's weight is 1 - l.  The
// backward gathers with this same function, so that it is the exact adjoint of what the forward evaluated.
__device__ __forceinline__ void ft_axis(int gi, float s, int n, int& i0, float& l) {
    const float f = fmaxf(((float)gi + 0.5f) * s - 0.5f, 0.0f);
    const int i = (int)f;
    i0 = i < n - 1 ? i : n - 1;
    l = fminf(f - (float)i0, 1.0f);
}

template <int C>
struct FtMergeSrc {
    static constexpr int STAGE_OCTETS = 0;
    static constexpr int CP = 2 * C;
    const float* prev;
    const float* lat;
    const float* wr;         // dim_reduction weight [C][2C]
    int H, W, h, w;
    float sy, sx;            // (float)h / H, (float)w / W as F.interpolate(size=...) computes them
    float p[CP];
    const float* lp;
    __device__ __forceinline__ void at(int n, int gy, int gx) {
        lp = lat + ((size_t)n * C * H + gy) * W + gx;
        int y0, x0;
        float ly, lx;
        ft_axis(gy, sy, h, y0, ly);
        ft_axis(gx, sx, w, x0, lx);
        const int dy = y0 < h - 1 ? w : 0, dx = x0 < w - 1 ? 1 : 0;
        const float* q = prev + (size_t)n * CP * h * w + (size_t)y0 * w + x0;
        const size_t hw = (size_t)h * w;
#pragma unroll
        for (int ci = 0; ci < CP; ++ci) {
            const float* qc = q + (size_t)ci * hw;
            p[ci] = (1.0f - ly) * ((1.0f - lx) * qc[0] + lx * qc[dx]) + ly * ((1.0f - lx) * qc[dy] + lx * qc[dy + dx]);
        }
    }
    __device__ __forceinline__ void load8(int c0, float* v) const {
        const size_t HW = (size_t)H * W;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float s = 0.0f;
#pragma unroll
            for (int ci = 0; ci < CP; ++ci) s = fmaf(wr[(c0 + k) * CP + ci], p[ci], s);
            v[k] = s + lp[(size_t)(c0 + k) * HW];
        }
    }
};

template <int C>
static FtMergeSrc<C> ft_merge_src(const float* prev, const float* lat, const float* wr, int h, int w, int H, int W) {
    FtMergeSrc<C> s{};
    s.prev = prev; s.lat = lat; s.wr = wr;
    s.H = H; s.W = W; s.h = h; s.w = w;
    s.sy = (float)h / (float)H;
    s.sx = (float)w / (float)W;
    return s;
}

static int ft_slabs(int ntok) {
    const int ntile = (int)ceil_div(ntok, FT_TOK), s = (int)ceil_div(ntile, 4);
    return s < FT_MAX_SLABS ? s : FT_MAX_SLABS;
}

static bool ft_path_args(const char* what, int N, int C, int H, int W) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)N * C * H * W >= (1LL << 40)) { set_error("%s: bad arguments", what); return false; }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// pathway backward.  Y = S * M, M = U(W_r prev) + lat.  d lat = dM is the forward convolution with flipped,
// channel-transposed taps (mvs_fmt_smooth_fwd on repacked weights); the two kernels below give d prev, d W_r and d S.  Weight
// gradients leave each workgroup as one fp32 partial; fmt_partial_reduce_kernel adds the partials in a fixed order (no atomics).
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int FT_BWD_PIX = 256;               // coarse pixels per workgroup pass of fmt_path_bwd_kernel

// partials (= workgroups) of one launch: bounded, so that the reduction's chains stay short (8192 / C: 256 | 512 | 1024)
static int ft_bwd_parts(long long work, int C) {
    const long long cap = 8192 / C;
    return (int)(work < cap ? work : cap);
}

// weight with which coarse index c enters fine index gi's two taps (both, where they collapse onto the last entry)
__device__ __forceinline__ float ft_tap_weight(int gi, float s, int n, int c) {
    int i0;
    float l;
    ft_axis(gi, s, n, i0, l);
    const int i1 = i0 < n - 1 ? i0 + 1 : i0;
    return (i0 == c ? 1.0f - l : 0.0f) + (i1 == c ? l : 0.0f);
}

// fine indices that can name coarse index c: those whose source coordinate lies within (c - 1, c + 1), one more on either side for the
// rounding of this estimate (ft_tap_weight decides); the clamps of ft_axis at both ends fall inside the clamped range
__device__ __forceinline__ void ft_fine_range(int c, float inv, int N, int& lo, int& hi) {
    lo = (int)floorf(((float)c - 0.5f) * inv - 0.5f) - 1;
    hi = (int)ceilf(((float)c + 1.5f) * inv - 0.5f) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > N - 1 ? N - 1 : hi;
}

// One thread per coarse pixel: dr = U^T(dM) gathered over the fine pixels whose taps name it, d prev = W_r^T dr, and the workgroup's
// partial of dW_r[c][j] = sum_p dr[c][p] prev[j][p] from LDS copies of dr and (JT channels at a time) prev.  Thread (jl, cg) owns
// rows cg * CPT .. of column pass * JT + jl.  prev is stored rotated by its channel so that the 32 columns of a wave hit 32 banks.
template <int C>
__global__ __launch_bounds__(256) void fmt_path_bwd_kernel(const float* __restrict__ dm, const float* __restrict__ prev, const float* __restrict__ wr,
                                                           float* __restrict__ dprev, float* __restrict__ part, int H, int W, int h, int w, float sy,
                                                           float sx, int chunks_per_view, int nchunk) {
    constexpr int CP = 2 * C, JT = CP < 32 ? CP : 32, NG = FT_BWD_PIX / JT, CPT = (C + NG - 1) / NG, NPASS = CP / JT;
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* drs = reinterpret_cast<float*>(lds4);                  // [C][256]
    float* ps = drs + C * FT_BWD_PIX;                             // [JT][256]
    const int tid = (int)threadIdx.x, jl = tid % JT, cg = tid / JT;
    const size_t hw = (size_t)h * w, HW = (size_t)H * W;
    const float iy = (float)H / (float)h, ix = (float)W / (float)w;
    float acc[NPASS][CPT];
#pragma unroll
    for (int ps_ = 0; ps_ < NPASS; ++ps_)
#pragma unroll
        for (int k = 0; k < CPT; ++k) acc[ps_][k] = 0.0f;
#pragma unroll 1
    for (int chunk = (int)blockIdx.x; chunk < nchunk; chunk += (int)gridDim.x) {
        const int n = chunk / chunks_per_view;
        const size_t p = (size_t)(chunk % chunks_per_view) * FT_BWD_PIX + tid;
        const bool ok = p < hw;
        float dr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dr[c] = 0.0f;
        if (ok) {
            const int cy = (int)(p / w), cx = (int)(p % w);
            int ylo, yhi, xlo, xhi;
            ft_fine_range(cy, iy, H, ylo, yhi);
            ft_fine_range(cx, ix, W, xlo, xhi);
            const float* dn = dm + (size_t)n * C * HW;
#pragma unroll 1
            for (int gy = ylo; gy <= yhi; ++gy) {
                const float wy = ft_tap_weight(gy, sy, h, cy);
                if (wy == 0.0f) continue;
#pragma unroll 1
                for (int gx = xlo; gx <= xhi; ++gx) {
                    const float wgt = wy * ft_tap_weight(gx, sx, w, cx);
                    if (wgt == 0.0f) continue;
                    const float* q = dn + (size_t)gy * W + gx;
#pragma unroll
                    for (int c = 0; c < C; ++c) dr[c] = fmaf(wgt, q[(size_t)c * HW], dr[c]);
                }
            }
            float* o = dprev + (size_t)n * CP * hw + p;
#pragma unroll 4
            for (int j = 0; j < CP; ++j) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) s = fmaf(wr[c * CP + j], dr[c], s);
                o[(size_t)j * hw] = s;
            }
        }
        __syncthreads();                                          // the previous chunk's readers are done with drs and ps
#pragma unroll
        for (int c = 0; c < C; ++c) drs[c * FT_BWD_PIX + tid] = dr[c];
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            if (pass) __syncthreads();
            const float* pn = prev + ((size_t)n * CP + pass * JT) * hw + p;
#pragma unroll 4
            for (int j = 0; j < JT; ++j) ps[j * FT_BWD_PIX + ((tid + j) & (FT_BWD_PIX - 1))] = ok ? pn[(size_t)j * hw] : 0.0f;
            __syncthreads();
            if (cg * CPT < C) {
#pragma unroll 4
                for (int pp = 0; pp < FT_BWD_PIX; ++pp) {
                    const float pv = ps[jl * FT_BWD_PIX + ((pp + jl) & (FT_BWD_PIX - 1))];
#pragma unroll
                    for (int k = 0; k < CPT; ++k) acc[pass][k] = fmaf(drs[(cg * CPT + k) * FT_BWD_PIX + pp], pv, acc[pass][k]);
                }
            }
        }
    }
    if (cg * CPT < C) {
        float* dst = part + (size_t)blockIdx.x * C * CP;
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass)
#pragma unroll
            for (int k = 0; k < CPT; ++k) dst[(cg * CPT + k) * CP + pass * JT + jl] = acc[pass][k];
    }
}

// dS[co][ci][ky][kx] = sum over pixels of dY[co][y][x] M[ci][y + ky - 1][x + kx - 1] as a GEMM on the exact-fp32 v_mfma_f32_16x16x4_f32:
// rows = co (16 per block; the upper 8 are zero at C = 8), columns = (ci, tap) = the 9 C weights of one row of S in memory order, K = the
// pixels of a TH x 64 tile.  The merged map of the tile and its halo is evaluated into LDS by FtMergeSrc, as the forward's staging
// does (zero outside the image); it is never written to memory.  Wave v owns the column blocks v, v + 4, ..: its accumulators are
// final for the workgroup, which keeps them over all of its tiles and writes one partial.
template <int C>
struct FtWgradShape {
    static constexpr int TH = C == 32 ? 2 : 4, TW = 64, NPIX = TH * TW;
    static constexpr int RS = TW + 4, PL = (TH + 2) * RS + 1;     // staged row / channel-plane strides of M
    static constexpr int DSS = NPIX + 4;                          // channel stride of the staged dY: lane (co, k) reads bank 4 co + k
    static constexpr int NRB = (C + 15) / 16, NCOL = 9 * C, NCB = (NCOL + 15) / 16, NCBW = (NCB + 3) / 4;
    static constexpr int LDS = (C * PL + C * DSS) * (int)sizeof(float);
};

template <int C>
__global__ __launch_bounds__(256) void fmt_smooth_wgrad_kernel(FtMergeSrc<C> src, const float* __restrict__ dy, float* __restrict__ part, int tiles_x,
                                                               int tiles_per_view, int ntile) {
    typedef FtWgradShape<C> F;
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* ms = reinterpret_cast<float*>(lds4);                   // [C][TH + 2][RS]
    float* ds = ms + C * F::PL;                                   // [C][DSS]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int H = src.H, W = src.W;
    int off[F::NCBW];                                             // this lane's column (ci, ky, kx) in the staged tile, -1 past the end
#pragma unroll
    for (int t = 0; t < F::NCBW; ++t) {
        const int col = (wave + 4 * t) * 16 + li, ci = col / 9, tap = col % 9;
        off[t] = col < F::NCOL ? ci * F::PL + (tap / 3) * F::RS + tap % 3 : -1;
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
        for (int pos = tid; pos < (F::TH + 2) * (F::TW + 2); pos += 256) {
            const int py = pos / (F::TW + 2), px = pos % (F::TW + 2), gy = y0 - 1 + py, gx = x0 - 1 + px;
            float* m = ms + py * F::RS + px;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                FtMergeSrc<C> s = src;
                s.at(n, gy, gx);
#pragma unroll 1
                for (int c0 = 0; c0 < C; c0 += 8) {
                    float v[8];
                    s.load8(c0, v);
#pragma unroll
                    for (int k = 0; k < 8; ++k) m[(c0 + k) * F::PL] = v[k];
                }
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) m[c * F::PL] = 0.0f;
            }
        }
#pragma unroll 1
        for (int e = tid; e < C * F::NPIX; e += 256) {
            const int c = e / F::NPIX, pix = e % F::NPIX, gy = y0 + pix / F::TW, gx = x0 + pix % F::TW;
            ds[c * F::DSS + pix] = gy < H && gx < W ? dy[(((size_t)n * C + c) * H + gy) * W + gx] : 0.0f;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < F::NPIX / 4; ++q) {
            const int pix = 4 * q + g, at = (pix / F::TW) * F::RS + pix % F::TW;
            float a[F::NRB];
#pragma unroll
            for (int rb = 0; rb < F::NRB; ++rb) a[rb] = rb * 16 + li < C ? ds[(rb * 16 + li) * F::DSS + pix] : 0.0f;
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
    float* dst = part + (size_t)blockIdx.x * C * F::NCOL;
#pragma unroll
    for (int t = 0; t < F::NCBW; ++t) {
        const int col = (wave + 4 * t) * 16 + li;
        if (col >= F::NCOL) continue;
#pragma unroll
        for (int rb = 0; rb < F::NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = rb * 16 + 4 * g + r;
                if (co < C) dst[co * F::NCOL + col] = acc[rb][t][r];
            }
    }
}

static bool ft_level_built(int C) { return C == 32 || C == 16 || C == 8; }

static long long ft_path_bwd_chunks(int N, int h, int w) { return (long long)N * (((long long)h * w + FT_BWD_PIX - 1) / FT_BWD_PIX); }

template <int C>
static long long ft_wgrad_tiles(int N, int H, int W) {
    return (long long)N * ceil_div(H, FtWgradShape<C>::TH) * ceil_div(W, FtWgradShape<C>::TW);
}

template <int C>
static int launch_fmt_path_bwd(const float* dm, const float* prev, const float* wr, float* dprev, float* dwr, float* part, int N, int h, int w, int H,
                               int W, hipStream_t st) {
    constexpr int JT = 2 * C < 32 ? 2 * C : 32, LDS = (C + JT) * FT_BWD_PIX * (int)sizeof(float);
    const int cpv = (int)ceil_div((long long)h * w, FT_BWD_PIX), nchunk = N * cpv, parts = ft_bwd_parts(nchunk, C);
    if (LDS > 48 * 1024)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fmt_path_bwd_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    hipLaunchKernelGGL((fmt_path_bwd_kernel<C>), dim3(parts), dim3(256), LDS, st, dm, prev, wr, dprev, part, H, W, h, w, (float)h / (float)H,
                       (float)w / (float)W, cpv, nchunk);
    const int rc = check_launch("fmt_path_bwd_kernel");
    return rc != MVS_OK ? rc : ft_reduce_partials(part, dwr, parts, C * 2 * C, st);
}

template <int C>
static int launch_fmt_smooth_wgrad(const FtMergeSrc<C>& src, const float* dy, float* ds, float* part, int N, hipStream_t st) {
    typedef FtWgradShape<C> F;
    const int tiles_x = (int)ceil_div(src.W, F::TW), tpv = tiles_x * (int)ceil_div(src.H, F::TH), ntile = N * tpv, parts = ft_bwd_parts(ntile, C);
    if (F::LDS > 48 * 1024)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fmt_smooth_wgrad_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
    hipLaunchKernelGGL((fmt_smooth_wgrad_kernel<C>), dim3(parts), dim3(256), F::LDS, st, src, dy, part, tiles_x, tpv, ntile);
    const int rc = check_launch("fmt_smooth_wgrad_kernel");
    return rc != MVS_OK ? rc : ft_reduce_partials(part, ds, parts, C * F::NCOL, st);
}

}  // namespace mvs

using namespace mvs;

extern "C" size_t mvs_fmt_weights_bytes(void) { return (size_t)FT_W_END * 16; }
extern "C" size_t mvs_fmt_vectors_bytes(void) { return (size_t)FT_V_END * 4; }
extern "C" size_t mvs_fmt_kv_operand_bytes(void) { return (size_t)FT_KVOP * 16; }

extern "C" size_t mvs_fmt_kv_workspace_bytes(int N, int n) {
    if (N < 1 || n < 1) return 0;
    return (size_t)N * ft_slabs(n) * FT_PART * sizeof(float);
}

extern "C" int mvs_fmt_kv_fwd(const float* x, const float* pe, const void* w_packed, const float* vectors, void* workspace, size_t workspace_bytes,
                              void* kv_operand, int N, int n, void* stream) {
    if (!x || !w_packed || !vectors || !workspace || !kv_operand || N < 1 || N > 65535 || n < 1 || (long long)N * 64 * n >= (1LL << 40)) {
        set_error("mvs_fmt_kv_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_fmt_kv_workspace_bytes(N, n)) { set_error("mvs_fmt_kv_fwd: workspace smaller than mvs_fmt_kv_workspace_bytes"); return MVS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int slabs = ft_slabs(n);
    hipLaunchKernelGGL(fmt_kv_partial_kernel, dim3(slabs, N), dim3(256), 4 * FT_PART * sizeof(float), st, x, pe,
                       reinterpret_cast<const bf16x8*>(w_packed), vectors, reinterpret_cast<float*>(workspace), n, (int)ceil_div(n, FT_TOK));
    int rc = check_launch("fmt_kv_partial_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(fmt_kv_reduce_kernel, dim3(5, N), dim3(256), 256 * sizeof(float), st, reinterpret_cast<const float*>(workspace),
                       reinterpret_cast<bf16x8*>(kv_operand), slabs);
    return check_launch("fmt_kv_reduce_kernel");
}

extern "C" int mvs_fmt_block_fwd(const float* x, const float* pe, const void* kv_operand, const void* w_packed, const float* vectors, float* y,
                                 int N, int n, int kv_div, void* stream) {
    if (!x || !kv_operand || !w_packed || !vectors || !y || N < 1 || N > 65535 || n < 1 || kv_div < 1 || (long long)N * 64 * n >= (1LL << 40)) {
        set_error("mvs_fmt_block_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    FmtBlockArgs a{x, pe, reinterpret_cast<const bf16x8*>(kv_operand), reinterpret_cast<const bf16x8*>(w_packed), vectors, y, n, kv_div};
    hipLaunchKernelGGL(fmt_block_kernel, dim3(ceil_div(n, 4 * FT_TOK), N), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("fmt_block_kernel");
}

#define MVS_FMT_LEVELS(X) X(32) X(16) X(8)

extern "C" int mvs_fmt_path_fwd(const float* prev, const float* lateral, const float* w_reduce, const void* w_packed, float* y, int N, int C, int h,
                                int w, int H, int W, void* stream) {
    if (!prev || !lateral || !w_reduce || !w_packed || !y || h < 1 || w < 1 || !ft_path_args("mvs_fmt_path_fwd", N, C, H, W)) {
        set_error("mvs_fmt_path_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
#define MVS_FMT_GO(CC) \
    if (C == CC) \
        return launch_conv2d_split<CC, CC, 3, 1>(ft_merge_src<CC>(prev, lateral, w_reduce, h, w, H, W), w_packed, PlanarSink<false>{nullptr, 0, y, nullptr, 0}, N, H, W, \
                                                 (hipStream_t)stream, "fmt_path_kernel");
    MVS_FMT_LEVELS(MVS_FMT_GO)
#undef MVS_FMT_GO
    set_error("mvs_fmt_path_fwd: built for the pathway levels 64 -> 32, 32 -> 16, 16 -> 8 (C = 32, 16, 8) [FMT.py:146-152]; got C = %d", C);
    return MVS_ERR_UNSUPPORTED;
}

extern "C" int mvs_fmt_merge_fwd(const float* prev, const float* lateral, const float* w_reduce, float* merged, int N, int C, int h, int w, int H,
                                 int W, void* stream) {
    if (!prev || !lateral || !w_reduce || !merged || h < 1 || w < 1 || !ft_path_args("mvs_fmt_merge_fwd", N, C, H, W)) {
        set_error("mvs_fmt_merge_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
#define MVS_FMT_MG(CC) \
    if (C == CC) return launch_conv2d_source<CC, CC / 8>(ft_merge_src<CC>(prev, lateral, w_reduce, h, w, H, W), merged, N, (hipStream_t)stream, "fmt_merge_kernel");
    MVS_FMT_LEVELS(MVS_FMT_MG)
#undef MVS_FMT_MG
    set_error("mvs_fmt_merge_fwd: built for C = 32, 16, 8 [FMT.py:146-152]; got C = %d", C);
    return MVS_ERR_UNSUPPORTED;
}

extern "C" int mvs_fmt_smooth_fwd(const float* x, const void* w_packed, float* y, int N, int C, int H, int W, void* stream) {
    if (!x || !w_packed || !y || !ft_path_args("mvs_fmt_smooth_fwd", N, C, H, W)) { set_error("mvs_fmt_smooth_fwd: bad arguments"); return MVS_ERR_ARG; }
#define MVS_FMT_SM(CC) \
    if (C == CC) \
        return launch_conv2d_split<CC, CC, 3, 1>(PlanarSrc{x, CC, H, W, nullptr}, w_packed, PlanarSink<false>{nullptr, 0, y, nullptr, 0}, N, H, W, (hipStream_t)stream, \
                                                 "fmt_path_kernel");
    MVS_FMT_LEVELS(MVS_FMT_SM)
#undef MVS_FMT_SM
    set_error("mvs_fmt_smooth_fwd: built for C = 32, 16, 8 [FMT.py:150-152]; got C = %d", C);
    return MVS_ERR_UNSUPPORTED;
}

// ---- pathway backward ----
static bool ft_bwd_args(const char* what, int N, int C, int h, int w, int H, int W) {
    if (h < 1 || w < 1 || !ft_path_args(what, N, C, H, W) || (long long)N * 2 * C * h * w >= (1LL << 40)) { set_error("%s: bad arguments", what); return false; }
    return true;
}

extern "C" size_t mvs_fmt_path_bwd_workspace_bytes(int N, int C, int h, int w) {
    if (N < 1 || N > 65535 || h < 1 || w < 1 || !ft_level_built(C) || ft_path_bwd_chunks(N, h, w) > 0x7fffffffLL) return 0;
    return (size_t)ft_bwd_parts(ft_path_bwd_chunks(N, h, w), C) * C * 2 * C * sizeof(float);
}

extern "C" int mvs_fmt_path_bwd(const float* d_merged, const float* prev, const float* w_reduce, float* d_prev, float* d_w_reduce, void* workspace,
                                size_t workspace_bytes, int N, int C, int h, int w, int H, int W, void* stream) {
    if (!ft_level_built(C)) {
        set_error("mvs_fmt_path_bwd: built for the pathway levels 64 -> 32, 32 -> 16, 16 -> 8 (C = 32, 16, 8) [FMT.py:146-152]; got C = %d", C);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!d_merged || !prev || !w_reduce || !d_prev || !d_w_reduce || !workspace || !ft_bwd_args("mvs_fmt_path_bwd", N, C, h, w, H, W)) {
        set_error("mvs_fmt_path_bwd: bad arguments");
        return MVS_ERR_ARG;
    }
    const size_t need = mvs_fmt_path_bwd_workspace_bytes(N, C, h, w);
    if (!need || workspace_bytes < need) { set_error("mvs_fmt_path_bwd: workspace smaller than mvs_fmt_path_bwd_workspace_bytes"); return MVS_ERR_ARG; }
#define MVS_FMT_PB(CC) \
    if (C == CC) return launch_fmt_path_bwd<CC>(d_merged, prev, w_reduce, d_prev, d_w_reduce, reinterpret_cast<float*>(workspace), N, h, w, H, W, (hipStream_t)stream);
    MVS_FMT_LEVELS(MVS_FMT_PB)
#undef MVS_FMT_PB
    return MVS_ERR_UNSUPPORTED;
}

extern "C" size_t mvs_fmt_smooth_wgrad_workspace_bytes(int N, int C, int H, int W) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || !ft_level_built(C)) return 0;
    const long long tiles = C == 32 ? ft_wgrad_tiles<32>(N, H, W) : C == 16 ? ft_wgrad_tiles<16>(N, H, W) : ft_wgrad_tiles<8>(N, H, W);
    if (tiles > 0x7fffffffLL) return 0;
    return (size_t)ft_bwd_parts(tiles, C) * C * 9 * C * sizeof(float);
}

extern "C" int mvs_fmt_smooth_wgrad(const float* dy, const float* prev, const float* lateral, const float* w_reduce, float* d_w_smooth, void* workspace,
                                    size_t workspace_bytes, int N, int C, int h, int w, int H, int W, void* stream) {
    if (!ft_level_built(C)) {
        set_error("mvs_fmt_smooth_wgrad: built for C = 32, 16, 8 [FMT.py:150-152]; got C = %d", C);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!dy || !prev || !lateral || !w_reduce || !d_w_smooth || !workspace || !ft_bwd_args("mvs_fmt_smooth_wgrad", N, C, h, w, H, W)) {
        set_error("mvs_fmt_smooth_wgrad: bad arguments");
        return MVS_ERR_ARG;
    }
    const size_t need = mvs_fmt_smooth_wgrad_workspace_bytes(N, C, H, W);
    if (!need || workspace_bytes < need) { set_error("mvs_fmt_smooth_wgrad: workspace smaller than mvs_fmt_smooth_wgrad_workspace_bytes"); return MVS_ERR_ARG; }
#define MVS_FMT_WG(CC) \
    if (C == CC) \
        return launch_fmt_smooth_wgrad<CC>(ft_merge_src<CC>(prev, lateral, w_reduce, h, w, H, W), dy, d_w_smooth, reinterpret_cast<float*>(workspace), N, \
                                           (hipStream_t)stream);
    MVS_FMT_LEVELS(MVS_FMT_WG)
#undef MVS_FMT_WG
    return MVS_ERR_UNSUPPORTED;
}
