// Gipuma-route fusion (misc/gipuma.py:184-205 hands a scene to fusibile, its consistency fusion): every pixel of a reference view
// is projected into EVERY other view of the scene; a pixel with at least num_consistent consistent views becomes one vertex, the
// average of its own and the consistent views' back-projections, and the view pixels it used are marked so that later reference
// views skip them.  The contract is restated here only as far as the code needs it:
//
//   view set      every view of the scene, processed in the caller's order (r = 0, 1, ...)
//   camera        P = K E (first three rows), M = P[:, :3], C = -M^-1 P[:, 3], f = K[0][0] of the reference view (host, fp64)
//   per pixel     d = D_r[y, x] in [depth_min, depth_max], used[r][y, x] == 0;  X = M_r^-1 ([x d, y d, d] - P_r[:, 3])
//   per view c    (u', v', z) = P_c [X; 1]; z > 0, 0 <= u < W, 0 <= v < H; d_c, I_c at (floor(u + .5), floor(v + .5)) clamped;
//                 consistent iff d_c in [depth_min, depth_max] and |f b / z - f b / d_c| < disp_thresh, b = |C_r - C_c|;
//                 then X_c = back-projection of c at (floor(u), floor(v)) with depth d_c (fusibile quirk: read at the rounded
//                 texel, back-project at the truncated one)
//   emit          n >= num_consistent: position (X + sum X_c) / (n + 1), colour floor((I_r + sum I_c) / (n + 1)) per channel,
//                 used[c][floor(v), floor(u)] = 1 for every consistent c
//
// ORDERING.  One gipuma_fuse_kernel launch per reference view r, all on one stream, no host synchronisation between them.  Launch r
// reads only used[r] (once per pixel, before anything else) and writes only used[c != r]; so no work-item of a launch reads a mark
// another work-item of the SAME launch writes, and no ordering between workgroups is needed or assumed (HIP promises none:
// MI355X_MICROARCH.md, "Workgroup dispatch ... inter-workgroup visibility").  Stream order alone makes launch r's marks visible to
// launch r + 1: a kernel boundary on one stream is the one cross-workgroup ordering HIP does guarantee.  Two work-items of one launch
// may store the same byte 1 to the same used[c] pixel; both store the same value.
//
// Layout on the device (9 bytes per pixel and view): depths fp32 [N,H,W] (probability-filtered), colours u32 [N,H,W] (r | g << 8 |
// b << 16: one load per texel), used u8 [N,H,W].  Per view 16 floats {A = M^-1 (9), C (3)}; per (r, c) 16 floats
// {H = M_c M_r^-1 (9), t = M_c C_r + P_c[:, 3] (3), f_r b (1)}: the projection of step 3 is then d * (H [x, y, 1]) + t, one
// 3x3 mat-vec per pixel and view.  Every multiply-add is an explicit fmaf, so the host-emulated build computes the same bits.
#include "mvs_common.h"

#include <math.h>

namespace mvs {

constexpr int kGpThreads = 256;                 // one pixel per work-item, row-major: a wave is 64 consecutive pixels of one row
constexpr int kGpView = 16;                     // floats per view constant block
constexpr int kGpPair = 16;                     // floats per (reference, other) constant block

struct GpHit {
    int tex;                                    // iy * W + ix of the rounded texel (depth / colour read)
    int iu, iv;                                 // truncated pixel (back-projection, mark)
    float dc;
};

// step 3 for one other view: true iff the view is consistent; `pc` = the (r, c) constant block, `dcm` = view c's depth map
__device__ __forceinline__ bool gp_consistent(const float* __restrict__ pc, const float* __restrict__ dcm, float x, float y, float d,
                                              int W, int H, float lo, float hi, float disp_thresh, GpHit& h) {
    const float w0 = fmaf(pc[0], x, fmaf(pc[1], y, pc[2]));
    const float w1 = fmaf(pc[3], x, fmaf(pc[4], y, pc[5]));
    const float w2 = fmaf(pc[6], x, fmaf(pc[7], y, pc[8]));
    const float z = fmaf(d, w2, pc[11]);
    if (!(z > 0.0f)) return false;
    const float u = fmaf(d, w0, pc[9]) / z, v = fmaf(d, w1, pc[10]) / z;
    if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) return false;     // NaN fails here too
    const int rx = (int)floorf(u + 0.5f), ry = (int)floorf(v + 0.5f);                  // >= 0; at most W / H: clamp
    const int ix = rx < W ? rx : W - 1, iy = ry < H ? ry : H - 1;
    h.tex = iy * W + ix;
    h.dc = dcm[h.tex];
    if (!(h.dc >= lo && h.dc <= hi)) return false;
    const float fb = pc[12];
    if (!(fabsf(fb / z - fb / h.dc) < disp_thresh)) return false;
    h.iu = (int)floorf(u);                      // 0 <= u < W, so 0 <= iu <= W - 1
    h.iv = (int)floorf(v);
    return true;
}

// d * (A [px, py, 1]) + C for one view's constant block
__device__ __forceinline__ void gp_backproject(const float* __restrict__ vc, float px, float py, float d, float& X, float& Y, float& Z) {
    X = fmaf(d, fmaf(vc[0], px, fmaf(vc[1], py, vc[2])), vc[9]);
    Y = fmaf(d, fmaf(vc[3], px, fmaf(vc[4], py, vc[5])), vc[10]);
    Z = fmaf(d, fmaf(vc[6], px, fmaf(vc[7], py, vc[8])), vc[11]);
}

// reference view r: mask / points [3,H,W] / rgb [H,W,3] of view r for the point-cloud compaction; marks into used[c != r];
// kSkipped: also store the used[r] this launch read (diagnostic; the product instantiation has no such store)
template <bool kSkipped>
__global__ __launch_bounds__(kGpThreads) void gipuma_fuse_kernel(const float* __restrict__ depths, const uint32_t* __restrict__ colors,
                                                                 uint8_t* __restrict__ used, const float* __restrict__ views,
                                                                 const float* __restrict__ pairs, int N, int H, int W, int r, float lo,
                                                                 float hi, float disp_thresh, int min_n, uint8_t* __restrict__ mask,
                                                                 float* __restrict__ points, uint8_t* __restrict__ rgb,
                                                                 uint8_t* __restrict__ skipped) {
    const int HW = H * W;
    const int p = (int)blockIdx.x * kGpThreads + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t base_r = (size_t)r * HW;
    const uint8_t skip = used[base_r + p];
    if (kSkipped) skipped[p] = skip;
    const float d = depths[base_r + p];
    if (skip != 0 || !(d >= lo && d <= hi)) {
        mask[p] = 0;
        return;
    }
    const float x = (float)(p % W), y = (float)(p / W);
    const float* __restrict__ pr = pairs + (size_t)r * N * kGpPair;
    float sx, sy, sz;
    gp_backproject(views + (size_t)r * kGpView, x, y, d, sx, sy, sz);
    const uint32_t c0 = colors[base_r + p];
    unsigned cr = c0 & 255u, cg = (c0 >> 8) & 255u, cb = (c0 >> 16) & 255u;
    int n = 0;
    for (int c = 0; c < N; ++c) {
        if (c == r) continue;
        GpHit h;
        if (!gp_consistent(pr + (size_t)c * kGpPair, depths + (size_t)c * HW, x, y, d, W, H, lo, hi, disp_thresh, h)) continue;
        ++n;
        float X, Y, Z;
        gp_backproject(views + (size_t)c * kGpView, (float)h.iu, (float)h.iv, h.dc, X, Y, Z);
        sx += X;
        sy += Y;
        sz += Z;
        const uint32_t col = colors[(size_t)c * HW + h.tex];
        cr += col & 255u;
        cg += (col >> 8) & 255u;
        cb += (col >> 16) & 255u;
    }
    if (n < min_n) {
        mask[p] = 0;
        return;
    }
    const float k = (float)(n + 1);
    mask[p] = 1;
    points[p] = sx / k;
    points[(size_t)HW + p] = sy / k;
    points[2 * (size_t)HW + p] = sz / k;
    const unsigned ku = (unsigned)(n + 1);
    rgb[3 * (size_t)p] = (uint8_t)(cr / ku);
    rgb[3 * (size_t)p + 1] = (uint8_t)(cg / ku);
    rgb[3 * (size_t)p + 2] = (uint8_t)(cb / ku);
    // marks: the same decisions again (same code, same inputs, same bits), for the emitted pixels only - cheaper than carrying
    // up to N - 1 remembered (c, iu, iv) per work-item through the first loop
    for (int c = 0; c < N; ++c) {
        if (c == r) continue;
        GpHit h;
        if (gp_consistent(pr + (size_t)c * kGpPair, depths + (size_t)c * HW, x, y, d, W, H, lo, hi, disp_thresh, h))
            used[(size_t)c * HW + (size_t)h.iv * W + h.iu] = 1;
    }
}

// probability filter + colour packing of one view: depth_out = keep ? depth : 0 (misc/gipuma.py:177-179), color_out = r | g << 8 | b << 16
__global__ __launch_bounds__(kGpThreads) void gipuma_prepare_view_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ keep,
                                                                         const uint8_t* __restrict__ rgb, int HW, float* __restrict__ depth_out,
                                                                         uint32_t* __restrict__ color_out) {
    const int p = (int)blockIdx.x * kGpThreads + (int)threadIdx.x;
    if (p >= HW) return;
    depth_out[p] = (keep == nullptr || keep[p] != 0) ? depth[p] : 0.0f;
    color_out[p] = (uint32_t)rgb[3 * (size_t)p] | ((uint32_t)rgb[3 * (size_t)p + 1] << 8) | ((uint32_t)rgb[3 * (size_t)p + 2] << 16);
}

}  // namespace mvs

using namespace mvs;

extern "C" size_t mvs_gipuma_view_floats(void) { return kGpView; }
extern "C" size_t mvs_gipuma_pair_floats(void) { return kGpPair; }

// host, fp64: camera constants of misc/gipuma.py:72-92 (P = [K 0; 0 1] E, first three rows) and the per-pair collapse of steps 2-3
extern "C" int mvs_gipuma_prepare_cams(const float* cams, int N, float* view_consts, float* pair_consts) {
    if (!cams || !view_consts || !pair_consts || N < 1) {
        set_error("mvs_gipuma_prepare_cams: bad arguments");
        return MVS_ERR_ARG;
    }
    double M[3][3], Minv[3][3], C[3], p4[3];
    double* all = new double[(size_t)N * 25];   // per view: M (9), Minv (9), C (3), p4 (3), f (1)
    for (int v = 0; v < N; ++v) {
        const float* E = cams + (size_t)v * 32;
        const float* K = E + 16;                // intrinsic slot, row stride 4
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
                for (int k = 0; k < 3; ++k) s += (double)K[i * 4 + k] * (double)E[k * 4 + j];
                if (j < 3) M[i][j] = s; else p4[i] = s;
            }
        }
        const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2],
                     c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
        const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
        if (!(det != 0.0) || !isfinite(det)) {
            delete[] all;
            set_error("mvs_gipuma_prepare_cams: view %d's projection matrix P[:, :3] is singular", v);
            return MVS_ERR_ARG;
        }
        Minv[0][0] = c00 / det; Minv[1][0] = c01 / det; Minv[2][0] = c02 / det;
        Minv[0][1] = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) / det;
        Minv[1][1] = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) / det;
        Minv[2][1] = (M[0][1] * M[2][0] - M[0][0] * M[2][1]) / det;
        Minv[0][2] = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) / det;
        Minv[1][2] = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) / det;
        Minv[2][2] = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) / det;
        for (int i = 0; i < 3; ++i) C[i] = -(Minv[i][0] * p4[0] + Minv[i][1] * p4[1] + Minv[i][2] * p4[2]);
        double* a = all + (size_t)v * 25;
        for (int i = 0; i < 9; ++i) { a[i] = M[i / 3][i % 3]; a[9 + i] = Minv[i / 3][i % 3]; }
        for (int i = 0; i < 3; ++i) { a[18 + i] = C[i]; a[21 + i] = p4[i]; }
        a[24] = (double)K[0];
        float* out = view_consts + (size_t)v * kGpView;
        for (int i = 0; i < kGpView; ++i) out[i] = 0.0f;
        for (int i = 0; i < 9; ++i) out[i] = (float)a[9 + i];
        for (int i = 0; i < 3; ++i) out[9 + i] = (float)C[i];
    }
    for (int r = 0; r < N; ++r) {
        const double* ar = all + (size_t)r * 25;
        for (int c = 0; c < N; ++c) {
            const double* ac = all + (size_t)c * 25;
            float* out = pair_consts + ((size_t)r * N + c) * kGpPair;
            for (int i = 0; i < kGpPair; ++i) out[i] = 0.0f;
            double b2 = 0.0;
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) {
                    double s = 0.0;
                    for (int k = 0; k < 3; ++k) s += ac[i * 3 + k] * ar[9 + k * 3 + j];      // M_c M_r^-1
                    out[i * 3 + j] = (float)s;
                }
                double t = ac[21 + i];
                for (int k = 0; k < 3; ++k) t += ac[i * 3 + k] * ar[18 + k];                // M_c C_r + p4_c
                out[9 + i] = (float)t;
                const double db = ar[18 + i] - ac[18 + i];
                b2 += db * db;
            }
            out[12] = (float)(ar[24] * sqrt(b2));
        }
    }
    delete[] all;
    return MVS_OK;
}

extern "C" int mvs_gipuma_prepare_view(const float* depth, const uint8_t* keep, const uint8_t* rgb, int h, int w, float* depth_out,
                                       uint32_t* color_out, void* stream) {
    if (!depth || !rgb || !depth_out || !color_out || h < 1 || w < 1 || (long long)h * w > 0x7fffffffLL - kGpThreads) {
        set_error("mvs_gipuma_prepare_view: bad arguments");
        return MVS_ERR_ARG;
    }
    const int HW = h * w;
    hipLaunchKernelGGL(gipuma_prepare_view_kernel, dim3((unsigned)((HW + kGpThreads - 1) / kGpThreads)), dim3(kGpThreads), 0,
                       (hipStream_t)stream, depth, keep, rgb, HW, depth_out, color_out);
    return check_launch("gipuma_prepare_view_kernel");
}

extern "C" int mvs_gipuma_fuse_view(const float* depths, const uint32_t* colors, uint8_t* used, const float* view_consts,
                                    const float* pair_consts, int N, int h, int w, int r, double depth_min, double depth_max,
                                    float disp_thresh, double num_consistent, uint8_t* mask, float* points, uint8_t* rgb,
                                    uint8_t* skipped, void* stream) {
    if (!depths || !colors || !used || !view_consts || !pair_consts || !mask || !points || !rgb || N < 1 || h < 1 || w < 1 ||
        r < 0 || r >= N || (long long)h * w > 0x7fffffffLL - kGpThreads || isnan(depth_min) || isnan(depth_max) ||
        isnan(num_consistent) || isnan(disp_thresh)) {
        set_error("mvs_gipuma_fuse_view: bad arguments");
        return MVS_ERR_ARG;
    }
    // the depth-range test in fp32 decides exactly what it decides in fp64 on the fp32 map values: round the bounds inwards
    float lo = (float)depth_min, hi = (float)depth_max;
    if ((double)lo < depth_min) lo = nextafterf(lo, INFINITY);
    if ((double)hi > depth_max) hi = nextafterf(hi, -INFINITY);
    // n >= num_consistent for an integer n  <=>  n >= ceil(num_consistent)
    const double nc = ceil(num_consistent);
    const int min_n = nc <= 0.0 ? 0 : (nc > (double)N ? N : (int)nc);
    const int HW = h * w;
    const dim3 grid((unsigned)((HW + kGpThreads - 1) / kGpThreads)), block(kGpThreads);
    if (skipped != nullptr)
        hipLaunchKernelGGL(gipuma_fuse_kernel<true>, grid, block, 0, (hipStream_t)stream, depths, colors, used, view_consts, pair_consts,
                           N, h, w, r, lo, hi, disp_thresh, min_n, mask, points, rgb, skipped);
    else
        hipLaunchKernelGGL(gipuma_fuse_kernel<false>, grid, block, 0, (hipStream_t)stream, depths, colors, used, view_consts, pair_consts,
                           N, h, w, r, lo, hi, disp_thresh, min_n, mask, points, rgb, skipped);
    return check_launch("gipuma_fuse_kernel");
}
