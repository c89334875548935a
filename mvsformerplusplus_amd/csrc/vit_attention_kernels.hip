// Softmax attention core of the DINOv2 ViT-B/14 backbone: 12 heads of 64, all tokens of a view, fp32-equivalent.
//
// Reference (restated, never copied): models/dino/layers/attention.py (Attention.forward: softmax(q k^T scale) v).
//
// Operands (vit_split.h, written by the qkv projection's epilogue): per (view, head) q | k packed-split rows of 64 channels and v
// transposed, every view padded to npad = a multiple of 32 tokens.  q carries scale * log2(e), so the scores are in log2 units.
//
// Workgroup = (128-query slab, head, view), 4 waves, a wave owns two 16-query tiles.  The workgroup walks the keys in steps of 32: the
// 8 KB k tile and the 8 KB vt tile of the step go through LDS (plain 16-byte copies: the global order IS the lanes' order), the next
// step's global loads in flight during the MFMAs.  Per step and query tile:
//     S^T[key][query]  = K Q^T      2 key tiles x 2 k-steps x 3 terms (k_lo q_hi + k_hi q_lo + k_hi q_hi)
//     online softmax   running max / sum in fp32, exp2; lane (li, g) holds keys 16 j + 4 g + r of query li: max over 8 values in the
//                      lane, then over the 4 lanes of the query (two shuffles); the sum is kept per lane and reduced once at the end
//     O^T[d][query]   += V^T P^T    4 channel blocks x 3 terms (v_lo p_hi + v_hi p_lo + v_hi p_hi); p = the score accumulator itself, split
//                      to hi + lo in registers (accumulator as operand: the vt order of vit_split.h is chosen for it)
// Keys at or past ntok are -inf; every step holds at least one valid key (its first), so a running max is finite after the first
// step and -inf - -inf never occurs.  No atomics, no split over the keys: bit-identical run to run, and a view's result does not
// depend on the other views of the call.  The output is the packed-split row operand of attn.proj's GEMM, row view * npad + token.
#include "mvs_common.h"
#include "split_format.h"
#include "vit_split.h"

namespace mvs {

constexpr int VA_NQ = 2;                      // query tiles per wave

struct VaArgs {
    const bf16x8* qkv;
    bf16x8* out;
    int ntok, npad;
};

__global__ __launch_bounds__(256) void va_attention_kernel(VaArgs a) {
    __shared__ float4 lk4[512], lv4[512];
    bf16x8* lk = reinterpret_cast<bf16x8*>(lk4);                   // [key tile 2][k-step 2][hi|lo][64 lanes]
    bf16x8* lv = reinterpret_cast<bf16x8*>(lv4);                   // [channel block 4][hi|lo][64 lanes]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int head = (int)blockIdx.y, view = (int)blockIdx.z;
    const int qt0 = ((int)blockIdx.x * 4 + wave) * VA_NQ;          // first query tile of the wave
    const bool active = qt0 * 16 < a.npad;                         // wave-uniform (npad % 32 == 0: both tiles exist or neither)
    const bf16x8* qs = a.qkv + vit_qkv_section(view, head, 0, a.npad);
    const bf16x8* ks = a.qkv + vit_qkv_section(view, head, 1, a.npad);
    const bf16x8* vs = a.qkv + vit_qkv_section(view, head, 2, a.npad);

    bf16x8 qh[VA_NQ][2], ql[VA_NQ][2];
    f32x4 o[VA_NQ][4];
    float m[VA_NQ], l[VA_NQ];
#pragma unroll
    for (int t = 0; t < VA_NQ; ++t) {
        const int qt = active ? qt0 + t : 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            qh[t][s] = qs[((size_t)(qt * 2 + s) * 2 + 0) * 64 + lane];
            ql[t][s] = qs[((size_t)(qt * 2 + s) * 2 + 1) * 64 + lane];
        }
#pragma unroll
        for (int db = 0; db < 4; ++db) o[t][db] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        m[t] = -INFINITY;
        l[t] = 0.0f;
    }

    const int steps = (a.ntok + VIT_KEY_STEP - 1) / VIT_KEY_STEP;  // <= npad / 32: every staged tile lies inside the sections
    bf16x8 rk[2], rv[2];
    auto fetch = [&](int st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            rk[i] = ks[(size_t)st * 512 + tid + 256 * i];
            rv[i] = vs[(size_t)st * 512 + tid + 256 * i];
        }
    };
    fetch(0);
#pragma unroll 1
    for (int st = 0; st < steps; ++st) {
        __syncthreads();                                           // the previous step has been read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            lk[tid + 256 * i] = rk[i];
            lv[tid + 256 * i] = rv[i];
        }
        __syncthreads();
        if (st + 1 < steps) fetch(st + 1);                         // in flight during the MFMAs below
        if (!active) continue;
        const bool ragged = (st + 1) * VIT_KEY_STEP > a.ntok;      // workgroup-uniform: only the last step masks
        bf16x8 kh[2][2], kl[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                kh[j][s] = lk[((j * 2 + s) * 2 + 0) * 64 + lane];
                kl[j][s] = lk[((j * 2 + s) * 2 + 1) * 64 + lane];
            }
        bf16x8 ph[VA_NQ], pl[VA_NQ];
#pragma unroll
        for (int t = 0; t < VA_NQ; ++t) {
            f32x4 sc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                sc[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int s = 0; s < 2; ++s) sc[j] = mfma3_bf16(kh[j][s], kl[j][s], qh[t][s], ql[t][s], sc[j]);
            }
            if (ragged) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (st * VIT_KEY_STEP + 16 * j + 4 * g + r >= a.ntok) sc[j][r] = -INFINITY;
            }
            float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m[t], mx);                      // finite: key st * 32 is valid
            const float alpha = __builtin_amdgcn_exp2f(m[t] - mn); // 0 at the first step (m = -inf)
            m[t] = mn;
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sc[j][r] - mn);
                    sum += p;
                    __bf16 h, lo;
                    split_bf16(p, h, lo);
                    ph[t][4 * j + r] = h;
                    pl[t][4 * j + r] = lo;
                }
            l[t] = fmaf(l[t], alpha, sum);
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[t][db][r] *= alpha;
        }
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const bf16x8 vh = lv[(db * 2 + 0) * 64 + lane], vl = lv[(db * 2 + 1) * 64 + lane];
#pragma unroll
            for (int t = 0; t < VA_NQ; ++t) o[t][db] = mfma3_bf16(vh, vl, ph[t], pl[t], o[t][db]);
        }
    }
    if (!active) return;
    // ---- lane (li, g) holds channels 16 db + 4 g .. + 3 of query li ----
#pragma unroll
    for (int t = 0; t < VA_NQ; ++t) {
        float z = l[t];
        z += __shfl_xor(z, 16);
        z += __shfl_xor(z, 32);
        const float inv = 1.0f / z;
        const int row = view * a.npad + (qt0 + t) * 16 + li;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const float v[4] = {o[t][db][0] * inv, o[t][db][1] * inv, o[t][db][2] * inv, o[t][db][3] * inv};
            vd_store_split4(a.out, 768 / 32, row, head * 64 + 16 * db + 4 * g, v);
        }
    }
}

}  // namespace mvs

using namespace mvs;

extern "C" size_t mvs_vit_qkv_bytes(int NV, int npad) {
    if (NV < 1 || npad < VIT_KEY_STEP || npad % VIT_KEY_STEP) return 0;
    return vit_qkv_section(NV, 0, 0, npad) * 16;
}

extern "C" int mvs_vit_attention_fwd(const void* qkv, void* a_packed, int NV, int ntok, int npad, int heads, int head_dim, void* stream) {
    if (heads != 12 || head_dim != 64) {
        set_error("mvs_vit_attention_fwd: built for 12 heads of 64 channels (DINOv2 ViT-B/14) [dinov2.py:388-398]; got %d heads of %d", heads,
                  head_dim);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!qkv || !a_packed || NV < 1 || NV > 65535 || ntok < 1 || npad < ntok || npad % VIT_KEY_STEP || (long long)NV * npad >= (1LL << 24)) {
        set_error("mvs_vit_attention_fwd: bad arguments (npad = tokens per view padded to a multiple of 32)");
        return MVS_ERR_ARG;
    }
    VaArgs a{reinterpret_cast<const bf16x8*>(qkv), reinterpret_cast<bf16x8*>(a_packed), ntok, npad};
    hipLaunchKernelGGL(va_attention_kernel, dim3(ceil_div(npad, 64 * VA_NQ), 12, NV), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("va_attention_kernel");
}
