// The FPN decoder's lateral merge as a convolution source (conv2d_split.h): intra_k = up2(intra_{k-1}) + inner_k(lateral_k),
// models/module.py:262-268.  Shared by the inference kernels (fpn_kernels.hip) and the training kernels (fpn_train_kernels.hip), whose
// adjoint of the upsample gathers with the same coordinate function the forward evaluates.
#pragma once
#include "conv2d_split.h"

namespace mvs {

// One axis of F.interpolate(scale_factor=2, bilinear, align_corners=True) in fp32: fine index gi of a map whose coarse side has n
// entries, s = (n - 1) / (N - 1) -> the first tap i0, the offset of the second tap (1, or 0 on the last entry) and its weight l; the
// first tap's weight is 1 - l.
__device__ __forceinline__ void up2_axis(int gi, float s, int n, int& i0, int& step, float& l) {
    const float f = s * (float)gi;
    i0 = (int)f;
    l = f - (float)i0;
    step = i0 < n - 1 ? 1 : 0;
}

// intra[c] at a full-resolution pixel = up2(prev)[c] + b[c] + sum_ci w[c][ci] * lat[ci]; prev [N, 64, H/2, W/2], lat [N, CLAT, H, W]
template <int CLAT>
struct MergeSrc {
    static constexpr int STAGE_OCTETS = 0;
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
        int y0, x0, ys;
        up2_axis(gy, sy, h, y0, ys, ly);
        up2_axis(gx, sx, w2, x0, dx, lx);
        dy = ys * w2;
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

static inline float up2_scale(int n, int N) { return N > 1 ? (float)(n - 1) / (float)(N - 1) : 0.0f; }

template <int CLAT>
static MergeSrc<CLAT> merge_src(const float* prev, const float* lat, const float* w, const float* b, int H, int W) {
    MergeSrc<CLAT> s{};
    s.prev = prev; s.lat = lat; s.w = w; s.b = b;
    s.H = H; s.W = W; s.h = H / 2; s.w2 = W / 2;
    s.sy = up2_scale(s.h, H);
    s.sx = up2_scale(s.w2, W);
    return s;
}

}  // namespace mvs
