// The packed-split row-operand store shared by the ViT decoder (vitdec_kernels.hip) and the ViT backbone (vit_attention_kernels.hip):
//     packed[row >> 4][k >> 5][hi|lo][lane = ((k >> 3) & 3) * 16 + (row & 15)][k & 7],       x ~= hi + lo (both bf16, RNE)
#pragma once
#include "mvs_common.h"
#include "split_format.h"

namespace mvs {

// four consecutive channels ch .. ch + 3 (ch % 4 == 0) of row `orow` into a packed-split tensor of `steps` k-steps per row
__device__ __forceinline__ void vd_store_split4(bf16x8* buf, int steps, int orow, int ch, const float (&v)[4]) {
    __bf16 h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_bf16(v[j], h[j], l[j]);
    char* dst = reinterpret_cast<char*>(buf + (((size_t)(orow >> 4) * steps + (ch >> 5)) * 2) * 64 + ((ch >> 3) & 3) * 16 + (orow & 15)) + (ch & 4) * 2;
    *reinterpret_cast<u32x2*>(dst) = (u32x2){pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3])};
    *reinterpret_cast<u32x2*>(dst + 64 * 16) = (u32x2){pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3])};
}

// The operands of the head-dimension-64 attention core, written by the qkv projection's epilogue: per (view, head) three sections of
// npad * 16 16-byte units (npad = tokens per view padded to a multiple of 32): q | k as packed-split rows of 64 channels (two k-steps),
// then v TRANSPOSED: vt[key >> 5][d >> 4][hi|lo][lane = g * 16 + (d & 15)][e] with key & 31 = 16 (e >> 2) + 4 g + (e & 3) - the order in
// which the lanes of a 16x16 accumulator hold the keys of two score tiles, so that p goes from accumulator to operand in registers.
constexpr int VIT_KEY_STEP = 32;
__device__ __host__ __forceinline__ size_t vit_qkv_section(int view, int head, int part, int npad) {
    return ((size_t)(view * 12 + head) * 3 + part) * (size_t)npad * 16;
}

// four consecutive channels d .. d + 3 of key `t` into the vt section `sec` of one (view, head)
__device__ __forceinline__ void vit_store_vt4(bf16x8* sec, int t, int d, const float (&v)[4]) {
    const int r = t & 31, e = ((r >> 4) << 2) | (r & 3), gg = (r >> 2) & 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        __bf16 h, l;
        split_bf16(v[j], h, l);
        __bf16* dst = reinterpret_cast<__bf16*>(sec + (((size_t)(t >> 5) * 4 + ((d + j) >> 4)) * 2) * 64 + gg * 16 + ((d + j) & 15)) + e;
        dst[0] = h;
        dst[64 * 8] = l;
    }
}

}  // namespace mvs
