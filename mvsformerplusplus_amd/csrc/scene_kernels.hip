// The two ends of a scene's depth inference (datasets/general_eval.py:112-131, :210-211 and test.py:266-294):
//   mvs_image_prepare_fwd        a decoded uint8 RGB image [h,w,3] -> the normalised fp32 planar view [3,H,W] (the network's input) AND the
//                                resized uint8 [H,W,3] image (what goes out as images/<view>.jpg): the "tt" edge pad (addressed, never
//                                materialised), the 8-bit linear resize, ToTensor and Normalize in one pass
//   mvs_depth_outputs_pack_fwd   refined_depth, photometric_confidence (and stage 4's confidence under --combine_reg_conf) -> one staging
//                                buffer: the depth rows bottom-up (the PFM body) followed by uint8(conf * 255)
//
// Both are memory-bound maps.  A wave owns 256 consecutive output pixels of one row (four per work-item: one 16-byte store per fp32 plane,
// 12 / 4 bytes of the uint8 outputs), a workgroup four rows, as in resize_kernels.hip.
//
// The resize is the fixed-point arithmetic of OpenCV's 8-bit INTER_LINEAR path, per axis:
//   f = (float)((d + 0.5) * (in / out) - 0.5) evaluated in double, s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= in - 1: s = in - 1, f = 0
//   coefficients short(rint((1 - f) * 2048)), short(rint(f * 2048))                 (rint: round half to even)
//   horizontal  S[s] * a0 + S[s + 1] * a1                                           (int)
//   vertical    (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
// Equal sizes give the identity (f = 0 everywhere: 2048 * S, then (2048 * (128 S)) >> 16 = 4 S, then (4 S + 2) >> 2 = S).
// This file is compiled without floating-point contraction (build.py): (d + 0.5) * scale - 0.5 and (pc * 3 + reg) / 4 round after every
// operation, as the host arithmetic they restate does.
#include "mvs_common.h"

namespace mvs {

constexpr int SC_PX = 4;                   // output pixels per work-item
constexpr int SC_ROWS = kBlock / kWave;    // output rows per workgroup (one wave each)
constexpr int SC_TILE_W = kWave * SC_PX;   // output pixels of a row per workgroup
constexpr int SC_COEF = 2048;              // OpenCV's INTER_RESIZE_COEF_SCALE

struct PrepareArgs {
    const uint8_t* src;      // [h, w, 3]
    const float* table;      // [3, 256]: ((u / 255) - mean[c]) / std[c]
    float* planar;           // [3, H, W]
    uint8_t* resized;        // [H, W, 3]
    int h, w, pad, H, W;     // pad: replicated rows above and below the stored image (the virtual source has h + 2 pad rows)
};

// tap index and the two 11-bit coefficients of output index d on an axis resized from `in` to `out`
__device__ __forceinline__ void linear_tap(int d, int in, int out, int& s, int& c0, int& c1) {
    const double scale = (double)in / (double)out;
    float f = (float)((d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    f -= fl;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= in - 1) { s = in - 1; f = 0.0f; }
    c0 = (int)(short)rintf((1.0f - f) * (float)SC_COEF);
    c1 = (int)(short)rintf(f * (float)SC_COEF);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void image_prepare_kernel(PrepareArgs a) {
    const int x0 = ((int)blockIdx.x * kWave + ((int)threadIdx.x & (kWave - 1))) * SC_PX;
    const int y = (int)blockIdx.y * SC_ROWS + ((int)threadIdx.x >> 6);
    if (x0 >= a.W || y >= a.H) return;
    const int npx = a.W - x0 < SC_PX ? a.W - x0 : SC_PX;

    const int hv = a.h + 2 * a.pad;                      // rows of the (virtually) padded source
    int sy, b0, b1;
    linear_tap(y, hv, a.H, sy, b0, b1);
    int ya = sy - a.pad, yb = (sy < hv - 1 ? sy + 1 : sy) - a.pad;
    ya = ya < 0 ? 0 : (ya > a.h - 1 ? a.h - 1 : ya);     // the replicated rows
    yb = yb < 0 ? 0 : (yb > a.h - 1 ? a.h - 1 : yb);
    const uint8_t* r0 = a.src + (long long)ya * a.w * 3;
    const uint8_t* r1 = a.src + (long long)yb * a.w * 3;

    uint8_t u[SC_PX][3];
    for (int p = 0; p < SC_PX; ++p) {
        u[p][0] = u[p][1] = u[p][2] = 0;
        if (p >= npx) continue;
        int sx, a0, a1;
        linear_tap(x0 + p, a.w, a.W, sx, a0, a1);
        const int ca = sx * 3, cb = (sx < a.w - 1 ? sx + 1 : sx) * 3;
        for (int c = 0; c < 3; ++c) {
            const int h0 = (int)r0[ca + c] * a0 + (int)r0[cb + c] * a1;
            const int h1 = (int)r1[ca + c] * a0 + (int)r1[cb + c] * a1;
            const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
            u[p][c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }

    const long long o = (long long)y * a.W + x0;
    const long long plane = (long long)a.H * a.W;
    if (VEC) {                                           // W % 4 == 0 and aligned bases: four pixels in range, every store aligned
        for (int c = 0; c < 3; ++c) {
            const float* t = a.table + c * 256;
            *reinterpret_cast<float4*>(a.planar + c * plane + o) = make_float4(t[u[0][c]], t[u[1][c]], t[u[2][c]], t[u[3][c]]);
        }
        const uint8_t* b = &u[0][0];                     // 12 bytes, pixel-interleaved as the output is
        uint32_t* q = reinterpret_cast<uint32_t*>(a.resized + o * 3);
        for (int k = 0; k < 3; ++k)
            q[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
        for (int p = 0; p < npx; ++p)
            for (int c = 0; c < 3; ++c) {
                a.planar[c * plane + o + p] = a.table[c * 256 + u[p][c]];
                a.resized[(o + p) * 3 + c] = u[p][c];
            }
    }
}

// uint8(v * 255): truncated, clamped to 0..255 (NaN: 0)
__device__ __forceinline__ uint32_t conf_byte(float v) {
    const float t = v * 255.0f;
    return t >= 255.0f ? 255u : (t >= 0.0f ? (uint32_t)(int)t : 0u);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void depth_outputs_pack_kernel(const float* depth, const float* conf, const float* reg, float* rows,
                                                                    uint8_t* bytes, int H, int W) {
    const int x0 = ((int)blockIdx.x * kWave + ((int)threadIdx.x & (kWave - 1))) * SC_PX;
    const int y = (int)blockIdx.y * SC_ROWS + ((int)threadIdx.x >> 6);
    if (x0 >= W || y >= H) return;
    const int npx = W - x0 < SC_PX ? W - x0 : SC_PX;
    const long long o = (long long)y * W + x0, of = (long long)(H - 1 - y) * W + x0;      // the PFM body starts with the bottom row
    float d[SC_PX] = {0.0f, 0.0f, 0.0f, 0.0f}, pc[SC_PX] = {0.0f, 0.0f, 0.0f, 0.0f}, rg[SC_PX] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC) {
        const float4 dv = *reinterpret_cast<const float4*>(depth + o), cv = *reinterpret_cast<const float4*>(conf + o);
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
        pc[0] = cv.x; pc[1] = cv.y; pc[2] = cv.z; pc[3] = cv.w;
        if (reg) {
            const float4 rv = *reinterpret_cast<const float4*>(reg + o);
            rg[0] = rv.x; rg[1] = rv.y; rg[2] = rv.z; rg[3] = rv.w;
        }
    } else {
        for (int p = 0; p < npx; ++p) {
            d[p] = depth[o + p];
            pc[p] = conf[o + p];
            if (reg) rg[p] = reg[o + p];
        }
    }
    uint32_t b[SC_PX];
    for (int p = 0; p < SC_PX; ++p) {
        float v = pc[p];
        if (reg) {                                       // test.py:282: three separately rounded fp32 operations
            v = v * 3.0f;
            v = v + rg[p];
            v = v / 4.0f;
        }
        b[p] = conf_byte(v);
    }
    if (VEC) {
        *reinterpret_cast<float4*>(rows + of) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint32_t*>(bytes + o) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
        for (int p = 0; p < npx; ++p) {
            rows[of + p] = d[p];
            bytes[o + p] = (uint8_t)b[p];
        }
    }
}

static bool scene_aligned(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0; }

}  // namespace mvs

using namespace mvs;

extern "C" int mvs_image_prepare_fwd(const unsigned char* src, int h, int w, int pad_rows, const float* table, float* planar,
                                     unsigned char* resized, int H, int W, void* stream) {
    const int side = 32768;
    if (!src || !table || !planar || !resized || h < 1 || w < 1 || H < 1 || W < 1 || pad_rows < 0 || pad_rows > 64 || h > side ||
        w > side || H > side || W > side) {
        set_error("mvs_image_prepare_fwd: bad arguments (1 <= sizes <= 32768, 0 <= pad_rows <= 64)");
        return MVS_ERR_ARG;
    }
    PrepareArgs a{src, table, planar, resized, h, w, pad_rows, H, W};
    const dim3 grid(ceil_div(W, SC_TILE_W), ceil_div(H, SC_ROWS), 1);
    if ((W % SC_PX) == 0 && scene_aligned(planar, 16) && scene_aligned(resized, 4))
        hipLaunchKernelGGL((image_prepare_kernel<true>), grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((image_prepare_kernel<false>), grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("image_prepare_kernel");
}

extern "C" int mvs_depth_outputs_pack_fwd(const float* depth, const float* conf, const float* reg_conf, void* staging, int H, int W,
                                          void* stream) {
    if (!depth || !conf || !staging || H < 1 || W < 1 || H > 32768 || W > 32768 || !scene_aligned(staging, 4)) {
        set_error("mvs_depth_outputs_pack_fwd: bad arguments (1 <= sizes <= 32768, a 4-byte aligned staging buffer of 5 H W bytes)");
        return MVS_ERR_ARG;
    }
    float* rows = static_cast<float*>(staging);
    uint8_t* bytes = static_cast<uint8_t*>(staging) + (size_t)H * W * sizeof(float);
    const dim3 grid(ceil_div(W, SC_TILE_W), ceil_div(H, SC_ROWS), 1);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (W % SC_PX) == 0 && scene_aligned(depth, 16) && scene_aligned(conf, 16) && (!reg_conf || scene_aligned(reg_conf, 16)) &&
                     scene_aligned(staging, 16);
    if (vec) hipLaunchKernelGGL((depth_outputs_pack_kernel<true>), grid, dim3(kBlock), 0, st, depth, conf, reg_conf, rows, bytes, H, W);
    else hipLaunchKernelGGL((depth_outputs_pack_kernel<false>), grid, dim3(kBlock), 0, st, depth, conf, reg_conf, rows, bytes, H, W);
    return check_launch("depth_outputs_pack_kernel");
}
