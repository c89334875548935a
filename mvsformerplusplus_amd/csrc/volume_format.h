// The three storage formats of the cost volume [B, D, H, W, 8] (channel-last, one voxel = the 8 group correlations), written by both
// aggregation passes of the gather and by the conversion kernels of warp_kernels.hip.
#pragma once
#include "split_format.h"

namespace mvs {

// the 8 normalised group values r of voxel `vox` (index over B * D * HW) into the volume `vol` of format FMT:
//   MVS_VOLUME_F16    fp16 octet (16 B), clamped to +-65504; sat_amax follows the largest |r| (sat::commit when the work-item ends)
//   MVS_VOLUME_SPLIT  [hi x8 | lo x8] bf16 (32 B), the split activation format of the bf16x3 U-Net (split_format.h)
//   MVS_VOLUME_F32    fp32 octet (32 B)
template <int FMT>
__device__ __forceinline__ void volume_store8(void* vol, size_t vox, const float (&r)[8], float& sat_amax) {
    if constexpr (FMT == MVS_VOLUME_F16) {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        h8 hv;
#pragma unroll
        for (int g = 0; g < 8; ++g) hv[g] = (_Float16)fminf(fmaxf(r[g], -65504.0f), 65504.0f);
        sat::track(sat_amax, r[0], r[1], r[2], r[3]);
        sat::track(sat_amax, r[4], r[5], r[6], r[7]);
        reinterpret_cast<h8*>(vol)[vox] = hv;
    } else {
        f32x4* o = reinterpret_cast<f32x4*>(vol) + vox * 2;
        if constexpr (FMT == MVS_VOLUME_SPLIT) {
            unsigned hw[4], lw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint16_t h0, h1, l0, l1;
                split_bf16_bits(r[2 * j], h0, l0);
                split_bf16_bits(r[2 * j + 1], h1, l1);
                hw[j] = (unsigned)h0 | ((unsigned)h1 << 16);
                lw[j] = (unsigned)l0 | ((unsigned)l1 << 16);
            }
            o[0] = f32x4{__builtin_bit_cast(float, hw[0]), __builtin_bit_cast(float, hw[1]), __builtin_bit_cast(float, hw[2]), __builtin_bit_cast(float, hw[3])};
            o[1] = f32x4{__builtin_bit_cast(float, lw[0]), __builtin_bit_cast(float, lw[1]), __builtin_bit_cast(float, lw[2]), __builtin_bit_cast(float, lw[3])};
        } else {
            o[0] = f32x4{r[0], r[1], r[2], r[3]};
            o[1] = f32x4{r[4], r[5], r[6], r[7]};
        }
    }
}

}  // namespace mvs
