// CrossVITDecoder: the ViT feature decoder of the shipped network at d_model 768, fp32-equivalent.
//
// Reference (restated, never copied): models/module.py:273-364 (CrossVITDecoder), models/dino/layers/block.py (CrossBlock, pre-norm,
// LayerScale), models/dino/layers/attention.py (CrossLinearAttention), models/dino/layers/mlp.py (fc1, GELU (erf), fc2).
//
// Layout.  Tokens are token-major.  The residual stream is fp32 [M, 768] (M = views x tokens, the views one after the other).
// Everything that is only ever a GEMM's row operand is kept as a PACKED-SPLIT tensor: per 16-row block and per 32-wide k-step the
// 64-lane hi fragment, then the 64-lane lo fragment of v_mfma_f32_16x16x32_bf16,
//     packed[row >> 4][k >> 5][hi|lo][lane = ((k >> 3) & 3) * 16 + (row & 15)][k & 7],       x ~= hi + lo (both bf16, RNE)
// i.e. 4 bytes per element like fp32, split ONCE by its producer (LayerNorm, the attention apply, the GELU / SiLU epilogues), so that a
// GEMM stages both operands with plain 16-byte copies in the order its lanes read them (conflict-free ds_read_b128).  Weights are
// packing.pack_linear_bf16x3: [k >> 5][out >> 4][hi|lo][lane][k & 7].  Every product is the three-term one (lo*hi + hi*lo + hi*hi,
// fp32 accumulate, k ascending: the result of an element does not depend on the tile that computes it).
//
// Kernels:
//   1. vd_rows_kernel: one wave per token row.  [prev_value * prev +] input row (fp32 / bf16 / fp16, any batch / view / row stride)
//      [-> LayerNorm eps 1e-6 (norm_layers)] -> x fp32 and / or packed-split(x) and / or packed-split(LayerNorm eps ln_eps (x)).
//      prev_value is read from device memory.
//   2. vd_gemm_kernel<NREP>: Y = epilogue(A W^T), the token GEMM of token_gemm.h (tile, staging, prefetch, MFMA loop, launcher) with one
//      running sum.  Rows: the row operand is read in place (linear layers), through a 3x3 window (proj: implicit GEMM, K = 9 x 768) or
//      through the 2x2 window of one parity class of ConvTranspose2d(4, stride 2, padding 1) (upsampler0 / 1: K = 4 x Cin, blockIdx.z =
//      class).  Sink, chosen at run time: fp32 (elu + 1 on the leading columns), residual + gamma * (. + bias), packed-split
//      act(. + bias), planar fp32 silu(. + bias), and for the ViT backbone QKV (the attention operands of
//      vit_split.h) and EMBED (+ bias + position row).
//   3. vd_kv_partial_kernel + vd_kv_reduce_kernel: KV_h = sum_s k_s (x) v_s and ksum_h = sum_s k_s from exact fp32 products
//      (v_mfma_f32_16x16x4_f32); per-slab partials added in slab order by the second launch: no atomics, bit-identical run to run.
//   4. vd_apply_kernel: a = (q . KV_h) / (q . ksum_h + 1e-6) on the exact fp32 MFMA, KV_h held in registers -> packed-split.
//   5. ViT backbone: vt_patches_kernel (14 x 14 x 3 patches of an image -> packed-split [M, 640]) and vt_cls_kernel (class rows, zeroed
//      padding rows); its GEMMs and LayerNorm rows are kernels 1 and 2, its attention core is vit_attention_kernels.hip.
// Rows past the end and window positions outside the map read as zero from a branch, never from an out-of-range load.
#include "mvs_common.h"
#include "split_format.h"
#include "token_gemm.h"
#include "vit_split.h"

namespace mvs {

constexpr int VD_C = 768, VD_HEADS = 12, VD_HD = 64, VD_HID = 3072;
constexpr int VD_KVPART = VD_HD * VD_HD + VD_HD;      // floats of one (view, head) summary: KV_h [d][m] | ksum_h [d]
constexpr int VD_MAX_SLABS = 16;

enum { VD_EPI_F32 = 0, VD_EPI_RESID = 1, VD_EPI_SPLIT = 2, VD_EPI_PLANAR = 3, VD_EPI_QKV = 4, VD_EPI_EMBED = 5 };
enum { VD_ACT_NONE = 0, VD_ACT_GELU = 1, VD_ACT_SILU = 2 };

__device__ __forceinline__ float vd_act(float t, int act) {
    if (act == VD_ACT_GELU) return gelu_erf(t);
    if (act == VD_ACT_SILU) return t / (1.0f + expf(-t));
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rows: mix, norm, split
// ---------------------------------------------------------------------------------------------------------------------------------
struct VdRowsArgs {
    const void* in;              // row r = (b * in_views + j) * n + t  at  in + b * in_bs + (in_v0 + j) * in_vs + t * in_rs  (elements)
    int in_dtype;
    long long in_bs, in_vs, in_rs;
    int in_v0, in_views;
    const float* prev;           // [M, 768] fp32 (nullable): value = prev_value[0] * prev + in
    const float* prev_value;
    const float* mix_w;          // norm_layers (eps 1e-6) applied to the mix (nullable)
    const float* mix_b;
    float* x;                    // [M, 768] fp32 (nullable)
    bf16x8* xp;                  // packed-split(x) at row ((b * out_V + out_v0 + j) * n + t) (nullable)
    const float* ln_w;           // LayerNorm (eps ln_eps) -> xn packed-split at row r (nullable)
    const float* ln_b;
    bf16x8* xn;
    int M, n, out_V, out_v0;
    float ln_eps;                // of the ln_w / ln_b LayerNorm: 1e-5 in the decoder, 1e-6 in the ViT backbone
};

__device__ __forceinline__ float vd_wave_sum(float s) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    return s;
}

// LayerNorm over the 768 channels of a row held as 3 x 4 values per lane (channels 4 (lane + 64 j) ..)
__device__ __forceinline__ void vd_row_norm(const float (&v)[3][4], const float* __restrict__ w, const float* __restrict__ b, float eps, int lane,
                                            float (&y)[3][4]) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    const float mean = vd_wave_sum(s) * (1.0f / VD_C);
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = v[j][k] - mean;
            q = fmaf(d, d, q);
        }
    const float rstd = 1.0f / sqrtf(vd_wave_sum(q) * (1.0f / VD_C) + eps);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 ww = *reinterpret_cast<const float4*>(w + 4 * (lane + 64 * j));
        const float4 bb = *reinterpret_cast<const float4*>(b + 4 * (lane + 64 * j));
        y[j][0] = fmaf((v[j][0] - mean) * rstd, ww.x, bb.x);
        y[j][1] = fmaf((v[j][1] - mean) * rstd, ww.y, bb.y);
        y[j][2] = fmaf((v[j][2] - mean) * rstd, ww.z, bb.z);
        y[j][3] = fmaf((v[j][3] - mean) * rstd, ww.w, bb.w);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void vd_rows_kernel(VdRowsArgs a) {
    typedef typename FeatT<DT>::type T;
    const int lane = (int)threadIdx.x & 63, r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (r >= a.M) return;                                          // wave-uniform; no workgroup barrier
    const int vv = r / a.n, t = r - vv * a.n, b = vv / a.in_views, j0 = vv - b * a.in_views;
    const T* src = reinterpret_cast<const T*>(a.in) + (size_t)b * a.in_bs + (size_t)(a.in_v0 + j0) * a.in_vs + (size_t)t * a.in_rs;
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][k] = to_f32(src[4 * (lane + 64 * j) + k]);
    if (a.prev) {
        const float pv = a.prev_value[0];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 p = *reinterpret_cast<const float4*>(a.prev + (size_t)r * VD_C + 4 * (lane + 64 * j));
            v[j][0] = fmaf(pv, p.x, v[j][0]);
            v[j][1] = fmaf(pv, p.y, v[j][1]);
            v[j][2] = fmaf(pv, p.z, v[j][2]);
            v[j][3] = fmaf(pv, p.w, v[j][3]);
        }
    }
    if (a.mix_w) {
        float y[3][4];
        vd_row_norm(v, a.mix_w, a.mix_b, 1e-6f, lane, y);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[j][k] = y[j][k];
    }
    if (a.x) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            *reinterpret_cast<float4*>(a.x + (size_t)r * VD_C + 4 * (lane + 64 * j)) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
    }
    if (a.xp) {
        const int orow = (b * a.out_V + a.out_v0 + j0) * a.n + t;
#pragma unroll
        for (int j = 0; j < 3; ++j) vd_store_split4(a.xp, VD_C / 32, orow, 4 * (lane + 64 * j), v[j]);
    }
    if (a.xn) {
        float y[3][4];
        vd_row_norm(v, a.ln_w, a.ln_b, a.ln_eps, lane, y);
#pragma unroll
        for (int j = 0; j < 3; ++j) vd_store_split4(a.xn, VD_C / 32, r, 4 * (lane + 64 * j), y[j]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------------------------
struct VdGemmArgs {
    const bf16x8* a;             // packed-split row operand, K (ROWS) or C (windows) channels per row
    const bf16x8* w;             // packed weights [K / 32][Npad / 16][hi|lo][64]; class z at w + z * w_class
    const float* bias;           // [N] (nullable)
    const float* gamma;          // [N]   (RESID)
    const float* res;            // [M, N] (RESID)
    void* out;
    int M, K, N, Npad;
    int a_mode, epi, act, elu_cols;
    int C, H, W;                 // windows: channels per tap, the source map; PLANAR: H W = pixels per view; QKV: W = rows per view (npad);
                                 // EMBED: H = patches per view, W = rows per view of the residual stream, res = position rows [H + 1, N]
    size_t w_class;
    float q_scale;               // QKV: the leading 768 columns (q) are multiplied by it
};

// Sink: + bias, then the run-time epilogue (epi / act / elu_cols)
struct VdSink {
    const VdGemmArgs& p;
    struct Row {
        int row, orow, view, opix, opixn;                              // view * opixn + opix = the output map's row `orow` (DECONV) or `row`
    };
    __device__ __forceinline__ Row row(int row, int cls) const {
        Row o{row, row, 0, 0, 1};
        if (p.a_mode == TG_A_DECONV) {
            tg_deconv_out(row, p.H, p.W, cls, o.view, o.opix);
            o.opixn = 4 * p.H * p.W;
            o.orow = o.view * o.opixn + o.opix;
        } else if (p.epi >= VD_EPI_PLANAR) {                          // rows per view: PLANAR H W pixels, QKV W rows, EMBED H patches
            o.opixn = p.epi == VD_EPI_PLANAR ? p.H * p.W : (p.epi == VD_EPI_QKV ? p.W : p.H);
            o.view = row / o.opixn;
            o.opix = row - o.view * o.opixn;
        }
        return o;
    }
    __device__ __forceinline__ void store4(const Row& o, int ch, const f32x4& a) const {
        const int row = o.row;
        float v[4] = {a[0], a[1], a[2], a[3]};
        if (p.bias) {
            const float4 bb = *reinterpret_cast<const float4*>(p.bias + ch);
            v[0] += bb.x; v[1] += bb.y; v[2] += bb.z; v[3] += bb.w;
        }
        if (p.epi == VD_EPI_F32) {
            if (ch < p.elu_cols) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = elu1(v[k]);
            }
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + (size_t)row * p.N + ch) = make_float4(v[0], v[1], v[2], v[3]);
        } else if (p.epi == VD_EPI_RESID) {
            const float4 gg = *reinterpret_cast<const float4*>(p.gamma + ch);
            const float4 rr = *reinterpret_cast<const float4*>(p.res + (size_t)row * p.N + ch);
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + (size_t)row * p.N + ch) =
                make_float4(fmaf(gg.x, v[0], rr.x), fmaf(gg.y, v[1], rr.y), fmaf(gg.z, v[2], rr.z), fmaf(gg.w, v[3], rr.w));
        } else if (p.epi == VD_EPI_QKV) {
            // q (x q_scale) | k -> packed-split rows of 64 channels per (view, head); v -> transposed (vit_split.h)
            const int vw = o.view, t = o.opix, part = ch / VD_C, c = ch - part * VD_C;
            bf16x8* sec = reinterpret_cast<bf16x8*>(p.out) + vit_qkv_section(vw, c >> 6, part, p.W);
            if (part == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] *= p.q_scale;
            }
            if (part < 2) vd_store_split4(sec, VD_HD / 32, t, c & 63, v);
            else vit_store_vt4(sec, t, c & 63, v);
        } else if (p.epi == VD_EPI_EMBED) {
            const int vw = o.view, patch = o.opix;
            const float4 pp = *reinterpret_cast<const float4*>(p.res + (size_t)(patch + 1) * p.N + ch);
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + ((size_t)vw * p.W + patch + 1) * p.N + ch) =
                make_float4(v[0] + pp.x, v[1] + pp.y, v[2] + pp.z, v[3] + pp.w);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = vd_act(v[k], p.act);
            if (p.epi == VD_EPI_SPLIT) {
                vd_store_split4(reinterpret_cast<bf16x8*>(p.out), p.N >> 5, o.orow, ch, v);
            } else {
                float* dst = reinterpret_cast<float*>(p.out) + ((size_t)o.view * p.N + ch) * o.opixn + o.opix;
#pragma unroll
                for (int k = 0; k < 4; ++k) dst[(size_t)k * o.opixn] = v[k];
            }
        }
    }
};

template <int NREP>
__global__ __launch_bounds__(256) void vd_gemm_kernel(VdGemmArgs p) {
    token_gemm<NREP, false>(p, TgRows<VdGemmArgs, true, false>{p}, VdSink{p});
}

// ---------------------------------------------------------------------------------------------------------------------------------
// key/value summary and apply (exact fp32 products)
// ---------------------------------------------------------------------------------------------------------------------------------
// kv [NV * n, 1536] fp32: columns 0..767 = elu(Wk .) + 1, 768..1535 = Wv .   Workgroup (slab, head, view); wave = 16 rows d of KV_h.
__global__ __launch_bounds__(256) void vd_kv_partial_kernel(const float* __restrict__ kv, float* __restrict__ part, int n, int per_slab) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int slab = (int)blockIdx.x, h = (int)blockIdx.y, view = (int)blockIdx.z, nslab = (int)gridDim.x;
    const int t0 = slab * per_slab, t1 = t0 + per_slab < n ? t0 + per_slab : n;
    const float* base = kv + (size_t)view * n * (2 * VD_C) + h * VD_HD;
    f32x4 acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    float ks = 0.0f;
    for (int t = t0; t < t1; t += 4) {
        const int tok = t + g;
        const bool ok = tok < t1;
        const float* row = base + (size_t)(ok ? tok : t0) * (2 * VD_C);
        const float kval = ok ? row[16 * wave + li] : 0.0f;
        ks += kval;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const float vval = ok ? row[VD_C + 16 * mb + li] : 0.0f;
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kval, vval, acc[mb], 0, 0, 0);
        }
    }
    ks += __shfl_xor(ks, 16);
    ks += __shfl_xor(ks, 32);
    float* dst = part + (((size_t)view * nslab + slab) * VD_HEADS + h) * VD_KVPART;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(16 * wave + 4 * g + r) * VD_HD + 16 * mb + li] = acc[mb][r];
    if (g == 0) dst[VD_HD * VD_HD + 16 * wave + li] = ks;
}

__global__ __launch_bounds__(256) void vd_kv_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int nslab) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x, h = (int)blockIdx.y, view = (int)blockIdx.z;
    if (e >= VD_KVPART) return;
    float s = 0.0f;
    for (int sl = 0; sl < nslab; ++sl) s += part[(((size_t)view * nslab + sl) * VD_HEADS + h) * VD_KVPART + e];
    out[((size_t)view * VD_HEADS + h) * VD_KVPART + e] = s;
}

// q [NV * n, 768] fp32 (elu + 1 applied), summary [NV / kv_div][12][KV_h | ksum_h] -> a packed-split [NV * n, 768].
// Workgroup (256-token chunk, head, view); a wave holds KV_h (d = 16 g + s on the MFMA k index) and takes 4 x 16 tokens.
__global__ __launch_bounds__(256) void vd_apply_kernel(const float* __restrict__ q, const float* __restrict__ summary, bf16x8* __restrict__ out, int n,
                                                       int kv_div) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int h = (int)blockIdx.y, view = (int)blockIdx.z;
    const int tw = ((int)blockIdx.x * 4 + wave) * 64;
    if (tw >= n) return;                                           // wave-uniform; no workgroup barrier
    const float* sm = summary + ((size_t)(view / kv_div) * VD_HEADS + h) * VD_KVPART;
    float a[4][16], kz[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        kz[s] = sm[VD_HD * VD_HD + 16 * g + s];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) a[mb][s] = sm[(16 * g + s) * VD_HD + 16 * mb + li];
    }
#pragma unroll 1
    for (int tb = 0; tb < 4; ++tb) {
        const int tok = tw + 16 * tb + li;
        if (tw + 16 * tb >= n) break;                              // wave-uniform
        const bool ok = tok < n;
        const float* qr = q + ((size_t)view * n + (ok ? tok : 0)) * VD_C + h * VD_HD + 16 * g;
        float qv[16];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const float4 t = *reinterpret_cast<const float4*>(qr + 4 * s4);
            qv[4 * s4 + 0] = t.x; qv[4 * s4 + 1] = t.y; qv[4 * s4 + 2] = t.z; qv[4 * s4 + 3] = t.w;
        }
        f32x4 acc[4], den = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[mb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb][s], qv[s], acc[mb], 0, 0, 0);
            den = __builtin_amdgcn_mfma_f32_16x16x4f32(kz[s], qv[s], den, 0, 0, 0);
        }
        if (!ok) continue;
        const float z = den[0] + 1e-6f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const float v[4] = {acc[mb][0] / z, acc[mb][1] / z, acc[mb][2] / z, acc[mb][3] / z};
            vd_store_split4(out, VD_C / 32, view * n + tok, h * VD_HD + 16 * mb + 4 * g, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ViT backbone: patch gather, class / padding rows
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int VT_PATCH = 14, VT_K = 3 * VT_PATCH * VT_PATCH, VT_KPAD = 640;       // 588 zero-padded to the GEMM's chunk of 64

struct VtPatchArgs {
    const void* img;             // [NV, 3, 14 gh, 14 gw], read in place: element (v, c, y, x) at v sb + c sc + y sy + x sx
    long long sb, sc, sy, sx;
    bf16x8* out;                 // packed-split [NV gh gw, 640]: column c * 196 + ky * 14 + kx (the order of the convolution's weight)
    int M, gh, gw;
};

template <int DT>
__global__ __launch_bounds__(256) void vt_patches_kernel(VtPatchArgs a) {
    typedef typename FeatT<DT>::type T;
    const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= (long long)a.M * (VT_KPAD / 4)) return;
    const int row = (int)(i / (VT_KPAD / 4)), k0 = (int)(i - (long long)row * (VT_KPAD / 4)) * 4;
    const int n = a.gh * a.gw, view = row / n, patch = row - view * n, py = patch / a.gw, px = patch - py * a.gw;
    const T* src = reinterpret_cast<const T*>(a.img) + (size_t)view * a.sb;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + j;
        v[j] = 0.0f;
        if (k < VT_K) {
            const int c = k / (VT_PATCH * VT_PATCH), rem = k - c * (VT_PATCH * VT_PATCH), ky = rem / VT_PATCH, kx = rem - ky * VT_PATCH;
            v[j] = to_f32(src[(size_t)c * a.sc + (size_t)(py * VT_PATCH + ky) * a.sy + (size_t)(px * VT_PATCH + kx) * a.sx]);
        }
    }
    vd_store_split4(a.out, VT_KPAD / 32, row, k0, v);
}

// row 0 of every view = cls_pos (cls_token + pos[0]); rows ntok .. npad - 1 = 0 (finite padding: masked as keys, never read as results)
__global__ __launch_bounds__(256) void vt_cls_kernel(const float* __restrict__ cls_pos, float* __restrict__ x, int NV, int ntok, int npad) {
    const int slots = 1 + npad - ntok;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= NV * slots * (VD_C / 4)) return;
    const int c4 = i % (VD_C / 4), rs = i / (VD_C / 4), view = rs / slots, slot = rs - view * slots;
    const int row = slot == 0 ? 0 : ntok + slot - 1;
    const float4 v = slot == 0 ? *reinterpret_cast<const float4*>(cls_pos + 4 * c4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    *reinterpret_cast<float4*>(x + ((size_t)view * npad + row) * VD_C + 4 * c4) = v;
}

static int vd_slabs(int n) {
    const int s = (int)ceil_div(n, 64);
    return s < VD_MAX_SLABS ? s : VD_MAX_SLABS;
}

static int vd_launch_gemm(const VdGemmArgs& p, int classes, hipStream_t st) {
    return token_gemm_launch("vd_gemm_kernel", vd_gemm_kernel<1>, vd_gemm_kernel<2>, vd_gemm_kernel<4>, p, classes, st);
}

}  // namespace mvs

using namespace mvs;

extern "C" size_t mvs_vitdec_packed_bytes(long long rows, int channels) {
    if (rows < 1 || channels < 32 || channels % 32) return 0;
    return (size_t)((rows + 15) / 16) * 16 * (size_t)channels * 4;
}

extern "C" size_t mvs_vitdec_summary_bytes(int NV) { return NV < 1 ? 0 : (size_t)NV * VD_HEADS * VD_KVPART * sizeof(float); }

extern "C" size_t mvs_vitdec_kv_workspace_bytes(int NV, int n) {
    if (NV < 1 || n < 1) return 0;
    return (size_t)NV * vd_slabs(n) * VD_HEADS * VD_KVPART * sizeof(float);
}

static int vd_rows(const char* who, const void* in, int in_dtype, long long in_batch_stride, long long in_view_stride, long long in_row_stride,
                   int in_v0, int in_views, const float* prev, const float* prev_value, const float* mix_w, const float* mix_b, float* x,
                   void* x_packed, int out_V, int out_v0, const float* ln_w, const float* ln_b, float ln_eps, void* xn_packed, int NV, int n,
                   int channels, void* stream) {
    if (channels != VD_C) {
        set_error("%s: built for rows of 768 channels (decoder_cfg d_model) [module.py:306]; got %d", who, channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!in || NV < 1 || n < 1 || (long long)NV * n >= (1LL << 24) || in_views < 1 || NV % in_views || in_v0 < 0 || out_v0 < 0 ||
        out_V < out_v0 + in_views || in_row_stride < VD_C || (prev && !prev_value) || (!mix_w != !mix_b) || (xn_packed && (!ln_w || !ln_b)) ||
        (!x && !x_packed && !xn_packed) || in_dtype < MVS_DTYPE_F32 || in_dtype > MVS_DTYPE_F16 || !(ln_eps > 0.0f)) {
        set_error("%s: bad arguments", who);
        return MVS_ERR_ARG;
    }
    VdRowsArgs a{in, in_dtype, in_batch_stride, in_view_stride, in_row_stride, in_v0, in_views, prev, prev_value, mix_w, mix_b, x,
                 reinterpret_cast<bf16x8*>(x_packed), ln_w, ln_b, reinterpret_cast<bf16x8*>(xn_packed), NV * n, n, out_V, out_v0, ln_eps};
    const dim3 grid(ceil_div((long long)NV * n, 4));
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == MVS_DTYPE_F32) hipLaunchKernelGGL((vd_rows_kernel<MVS_DTYPE_F32>), grid, dim3(256), 0, st, a);
    else if (in_dtype == MVS_DTYPE_BF16) hipLaunchKernelGGL((vd_rows_kernel<MVS_DTYPE_BF16>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((vd_rows_kernel<MVS_DTYPE_F16>), grid, dim3(256), 0, st, a);
    return check_launch("vd_rows_kernel");
}

extern "C" int mvs_vitdec_rows_fwd(const void* in, int in_dtype, long long in_batch_stride, long long in_view_stride, long long in_row_stride,
                                   int in_v0, int in_views, const float* prev, const float* prev_value, const float* mix_w, const float* mix_b,
                                   float* x, void* x_packed, int out_V, int out_v0, const float* ln_w, const float* ln_b, void* xn_packed,
                                   int NV, int n, int channels, void* stream) {
    return vd_rows("mvs_vitdec_rows_fwd", in, in_dtype, in_batch_stride, in_view_stride, in_row_stride, in_v0, in_views, prev, prev_value, mix_w,
                   mix_b, x, x_packed, out_V, out_v0, ln_w, ln_b, 1e-5f, xn_packed, NV, n, channels, stream);
}

// the same row pass with the eps of the ln_w / ln_b LayerNorm as an argument (the ViT backbone's norm1 / norm2: 1e-6)
extern "C" int mvs_vit_rows_fwd(const void* in, int in_dtype, long long in_batch_stride, long long in_view_stride, long long in_row_stride,
                                int in_v0, int in_views, const float* prev, const float* prev_value, const float* mix_w, const float* mix_b,
                                float* x, void* x_packed, int out_V, int out_v0, const float* ln_w, const float* ln_b, float ln_eps,
                                void* xn_packed, int NV, int n, int channels, void* stream) {
    return vd_rows("mvs_vit_rows_fwd", in, in_dtype, in_batch_stride, in_view_stride, in_row_stride, in_v0, in_views, prev, prev_value, mix_w,
                   mix_b, x, x_packed, out_V, out_v0, ln_w, ln_b, ln_eps, xn_packed, NV, n, channels, stream);
}

extern "C" int mvs_vitdec_linear_fwd(const void* a_packed, const void* w_packed, const float* bias, const float* gamma, const float* residual,
                                     void* y, int M, int K, int N, int epilogue, int elu_cols, void* stream) {
    // 1536 -> 768 is the data gradient of [k_proj; v_proj]: the same kernel on the transposed weight
    const bool shape = (K == VD_C && (N == VD_C || N == 2 * VD_C || N == VD_HID)) || ((K == VD_HID || K == 2 * VD_C) && N == VD_C);
    if (!shape || epilogue < VD_EPI_F32 || epilogue > VD_EPI_SPLIT) {
        set_error("mvs_vitdec_linear_fwd: built for the CrossBlock linears at d_model 768 (K -> N = 768 -> 768 | 1536 | 3072, 1536 | 3072 -> 768) with "
                  "epilogue 0 (fp32, elu + 1 on the leading columns), 1 (residual + gamma (. + bias)) or 2 (packed-split GELU(. + bias)) "
                  "[block.py:294-329]; got K = %d, N = %d, epilogue %d", K, N, epilogue);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!a_packed || !w_packed || !y || M < 1 || M >= (1 << 24) || elu_cols < 0 || elu_cols > N || elu_cols % 4 ||
        (epilogue == VD_EPI_RESID && (!gamma || !residual || !bias))) {
        set_error("mvs_vitdec_linear_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    VdGemmArgs p{};
    p.a = reinterpret_cast<const bf16x8*>(a_packed);
    p.w = reinterpret_cast<const bf16x8*>(w_packed);
    p.bias = bias; p.gamma = gamma; p.res = residual; p.out = y;
    p.M = M; p.K = K; p.N = N; p.Npad = N;
    p.a_mode = TG_A_ROWS; p.epi = epilogue; p.act = epilogue == VD_EPI_SPLIT ? VD_ACT_GELU : VD_ACT_NONE; p.elu_cols = elu_cols;
    p.C = K; p.H = 1; p.W = 1;
    return vd_launch_gemm(p, 1, (hipStream_t)stream);
}

// layer 0: proj = Conv2d(768, 256, 3, padding 1); 1 / 2: upsampler0 / 1 = ConvTranspose2d(256, 128 | 128, 64, 4, stride 2, padding 1);
// BatchNorm folded into (w_packed, bias), SiLU.  x packed-split tokens [NV * H * W, Cin]; y packed-split tokens of the output map
// (planar = 0) or planar fp32 [NV, Cout, Ho, Wo] (planar = 1).
extern "C" int mvs_vitdec_conv_fwd(const void* x_packed, const void* w_packed, const float* bias, void* y, int layer, int planar, int NV, int H,
                                   int W, void* stream) {
    if (layer < 0 || layer > 2) {
        set_error("mvs_vitdec_conv_fwd: built for layer 0 (proj 768 -> 256, 3x3), 1 (upsampler0 256 -> 128) and 2 (upsampler1 128 -> 64, both "
                  "ConvTranspose2d 4x4 stride 2 padding 1) [module.py:316-321]; got layer %d", layer);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!x_packed || !w_packed || !bias || !y || NV < 1 || H < 1 || W < 1 || H > 32767 || W > 32767 || (long long)NV * H * W >= (1LL << 22)) {
        set_error("mvs_vitdec_conv_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    const VitdecHeadLayer& L = VITDEC_HEAD[layer];
    VdGemmArgs p{};
    p.a = reinterpret_cast<const bf16x8*>(x_packed);
    p.w = reinterpret_cast<const bf16x8*>(w_packed);
    p.bias = bias; p.out = y;
    p.M = NV * H * W; p.K = L.taps * L.cin; p.N = L.cout; p.Npad = (L.cout + TG_TN - 1) / TG_TN * TG_TN;
    p.a_mode = layer == 0 ? TG_A_CONV3 : TG_A_DECONV; p.epi = planar ? VD_EPI_PLANAR : VD_EPI_SPLIT; p.act = VD_ACT_SILU;
    p.C = L.cin; p.H = H; p.W = W;
    p.w_class = (size_t)(p.K / 32) * (p.Npad / 16) * 128;
    return vd_launch_gemm(p, layer == 0 ? 1 : 4, (hipStream_t)stream);
}

extern "C" int mvs_vitdec_kv_fwd(const float* kv, void* workspace, size_t workspace_bytes, float* summary, int NV, int n, int channels,
                                 void* stream) {
    if (channels != 2 * VD_C) {
        set_error("mvs_vitdec_kv_fwd: built for 12 heads of 64 channels: kv = [NV * n, 1536] (elu(k) + 1 | v) [attention.py:268-281]; got %d columns",
                  channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!kv || !workspace || !summary || NV < 1 || NV > 65535 || n < 1 || (long long)NV * n >= (1LL << 24)) {
        set_error("mvs_vitdec_kv_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_vitdec_kv_workspace_bytes(NV, n)) {
        set_error("mvs_vitdec_kv_fwd: workspace smaller than mvs_vitdec_kv_workspace_bytes");
        return MVS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const int slabs = vd_slabs(n), per_slab = ((int)ceil_div(n, slabs) + 3) / 4 * 4;
    hipLaunchKernelGGL(vd_kv_partial_kernel, dim3(slabs, VD_HEADS, NV), dim3(256), 0, st, kv, reinterpret_cast<float*>(workspace), n, per_slab);
    int rc = check_launch("vd_kv_partial_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(vd_kv_reduce_kernel, dim3(ceil_div(VD_KVPART, 256), VD_HEADS, NV), dim3(256), 0, st, reinterpret_cast<const float*>(workspace),
                       summary, slabs);
    return check_launch("vd_kv_reduce_kernel");
}

extern "C" int mvs_vitdec_apply_fwd(const float* q, const float* summary, void* a_packed, int NV, int n, int kv_div, int channels, void* stream) {
    if (channels != VD_C) {
        set_error("mvs_vitdec_apply_fwd: built for 12 heads of 64 channels: q = [NV * n, 768] [attention.py:281-284]; got %d columns", channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!q || !summary || !a_packed || NV < 1 || NV > 65535 || n < 1 || kv_div < 1 || (long long)NV * n >= (1LL << 24)) {
        set_error("mvs_vitdec_apply_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    hipLaunchKernelGGL(vd_apply_kernel, dim3(ceil_div(n, 256), VD_HEADS, NV), dim3(256), 0, (hipStream_t)stream, q, summary,
                       reinterpret_cast<bf16x8*>(a_packed), n, kv_div);
    return check_launch("vd_apply_kernel");
}

// ---- ViT backbone -----------------------------------------------------------------------------------------
extern "C" int mvs_vit_patches_fwd(const void* img, int dtype, long long batch_stride, long long channel_stride, long long row_stride,
                                   long long col_stride, void* a_packed, int NV, int gh, int gw, int patch, int in_chans, void* stream) {
    if (patch != VT_PATCH || in_chans != 3) {
        set_error("mvs_vit_patches_fwd: built for 14 x 14 patches of 3 channels (DINOv2 ViT-B/14 patch_embed) [patch_embed.py]; got patch %d, "
                  "%d channels", patch, in_chans);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!img || !a_packed || NV < 1 || gh < 1 || gw < 1 || (long long)NV * gh * gw >= (1LL << 22) || dtype < MVS_DTYPE_F32 || dtype > MVS_DTYPE_F16 ||
        batch_stride < 0 || channel_stride < 0 || row_stride < 0 || col_stride < 0) {
        set_error("mvs_vit_patches_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    VtPatchArgs a{img, batch_stride, channel_stride, row_stride, col_stride, reinterpret_cast<bf16x8*>(a_packed), NV * gh * gw, gh, gw};
    const dim3 grid(ceil_div((long long)a.M * (VT_KPAD / 4), 256));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVS_DTYPE_F32) hipLaunchKernelGGL((vt_patches_kernel<MVS_DTYPE_F32>), grid, dim3(256), 0, st, a);
    else if (dtype == MVS_DTYPE_BF16) hipLaunchKernelGGL((vt_patches_kernel<MVS_DTYPE_BF16>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((vt_patches_kernel<MVS_DTYPE_F16>), grid, dim3(256), 0, st, a);
    return check_launch("vt_patches_kernel");
}

// x [NV, npad, 768] fp32: row 0 = cls_pos, rows 1 .. n = patches W^T + bias + pos[1 + patch], rows n + 1 .. npad - 1 = 0
extern "C" int mvs_vit_embed_fwd(const void* a_packed, const void* w_packed, const float* bias, const float* pos, const float* cls_pos, float* x,
                                 int NV, int n, int npad, int channels, void* stream) {
    if (channels != VD_C) {
        set_error("mvs_vit_embed_fwd: built for embed_dim 768 (DINOv2 ViT-B/14) [dinov2.py:388-398]; got %d", channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!a_packed || !w_packed || !bias || !pos || !cls_pos || !x || NV < 1 || n < 1 || npad < n + 1 || npad % VIT_KEY_STEP ||
        (long long)NV * npad >= (1LL << 22)) {
        set_error("mvs_vit_embed_fwd: bad arguments (npad = n + 1 tokens per view padded to a multiple of 32)");
        return MVS_ERR_ARG;
    }
    VdGemmArgs p{};
    p.a = reinterpret_cast<const bf16x8*>(a_packed);
    p.w = reinterpret_cast<const bf16x8*>(w_packed);
    p.bias = bias; p.res = pos; p.out = x;
    p.M = NV * n; p.K = VT_KPAD; p.N = VD_C; p.Npad = VD_C;
    p.a_mode = TG_A_ROWS; p.epi = VD_EPI_EMBED; p.act = VD_ACT_NONE;
    p.C = VT_KPAD; p.H = n; p.W = npad;
    int rc = vd_launch_gemm(p, 1, (hipStream_t)stream);
    if (rc != MVS_OK) return rc;
    const int slots = 1 + npad - (n + 1);
    hipLaunchKernelGGL(vt_cls_kernel, dim3(ceil_div((long long)NV * slots * (VD_C / 4), 256)), dim3(256), 0, (hipStream_t)stream, cls_pos, x, NV,
                       n + 1, npad);
    return check_launch("vt_cls_kernel");
}

// qkv [mvs_vit_qkv_bytes(NV, npad)]: the attention core's operands (vit_split.h) = xn W^T + bias, the q columns times q_scale
extern "C" int mvs_vit_qkv_fwd(const void* xn_packed, const void* w_packed, const float* bias, void* qkv, int NV, int npad, float q_scale,
                               int channels, void* stream) {
    if (channels != VD_C) {
        set_error("mvs_vit_qkv_fwd: built for embed_dim 768, 12 heads of 64 (DINOv2 ViT-B/14) [attention.py:68-79]; got %d", channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!xn_packed || !w_packed || !bias || !qkv || NV < 1 || npad < VIT_KEY_STEP || npad % VIT_KEY_STEP || (long long)NV * npad >= (1LL << 22) ||
        !(q_scale > 0.0f)) {
        set_error("mvs_vit_qkv_fwd: bad arguments (npad = tokens per view padded to a multiple of 32)");
        return MVS_ERR_ARG;
    }
    VdGemmArgs p{};
    p.a = reinterpret_cast<const bf16x8*>(xn_packed);
    p.w = reinterpret_cast<const bf16x8*>(w_packed);
    p.bias = bias; p.out = qkv;
    p.M = NV * npad; p.K = VD_C; p.N = 3 * VD_C; p.Npad = 3 * VD_C;
    p.a_mode = TG_A_ROWS; p.epi = VD_EPI_QKV; p.act = VD_ACT_NONE;
    p.C = VD_C; p.H = 1; p.W = npad;
    p.q_scale = q_scale;
    return vd_launch_gemm(p, 1, (hipStream_t)stream);
}
