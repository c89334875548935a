// The multi-stage depth losses and the validation metrics (models/losses.py, utils.py:156-189 and
// trainer/mvsformer_trainer.py:288-336):
//   mvs_ce_loss_fwd / _bwd      the "ce" stage loss: cross entropy of the logits [B,D,H,W] against the bin of the hypotheses that holds the
//                               ground truth, over the pixels that are masked in and in range
//   mvs_reg_loss_fwd / _bwd     the "reg" stage loss (and reg_loss / simple_loss): smooth L1 (beta 1) of depth / interval, optionally clamped
//                               from above by the hypotheses' range ("dynamic")
//   mvs_depth_metrics           the counts and sums behind Thres_metrics / AbsDepthError_metrics for T thresholds and T bands per image,
//                               and the per-image and batch means
//
// Plain fp32 maps: one work-item per pixel, consecutive lanes take consecutive pixels of the flattened [B,H,W] index, so every plane read
// of a wave is one coalesced 256-byte segment.  A pixel walks its depth column ONCE (with `inverse` from plane D - 1 down: the
// reference's two torch.flip copies are index arithmetic) and reads the target logit once more.
//
// Reductions use no floating-point atomics: every workgroup leaves one partial (a fp64 sum and integer counts: wave shuffles, then the four
// waves through LDS), and a one-workgroup finalize adds the partials in a fixed order (work-item t takes partials t, t + 256, ... in turn,
// then a fixed LDS tree).  Two runs give bit-identical results.
//
// The decisions (bin index, range tests, mask, clamp) are the reference's fp32 operations one by one; contraction is off for this file so
// that none of them is fused.
#include "mvs_common.h"

#pragma clang fp contract(off)

namespace mvs {

constexpr int LS_WAVES = kBlock / kWave;
constexpr int MT_ITEMS = 4;                      // pixels per work-item of the metrics kernel
constexpr int MT_TILE = kBlock * MT_ITEMS;       // pixels per workgroup of the metrics kernel

// ---- workgroup reductions (every work-item of the workgroup calls them) ----
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, (unsigned)o);
    return v;                                     // lane 0 holds the wave's sum
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, (unsigned)o);
    return v;
}

// sum over the workgroup, valid in work-item 0; `slot` is LS_WAVES elements of LDS
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* slot) {
    v = wave_sum(v);
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    __syncthreads();                              // the slot may still be read from the previous call
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    T s = slot[0];
    for (int w = 1; w < LS_WAVES; ++w) s += slot[w];
    return s;
}

// partials[0 .. n) added in a fixed order by one workgroup; valid in work-item 0
template <typename T>
__device__ __forceinline__ T ordered_sum(const T* partials, long long stride, int n, T* slot) {
    T s = 0;
    for (int i = (int)threadIdx.x; i < n; i += kBlock) s += partials[(long long)i * stride];
    return block_sum(s, slot);
}

// ---- cross entropy ----------------------------------------------------------------------------------------------------------------
// losses.py:31-62.  Walk position j reads stored plane k = inverse ? D - 1 - j : j.
__global__ __launch_bounds__(kBlock) void ce_loss_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ hyp,
                                                             const float* __restrict__ gt, const float* __restrict__ mask, int* __restrict__ index,
                                                             float* __restrict__ lse_out, double* __restrict__ part_sum, int* __restrict__ part_cnt,
                                                             long long P, int D, int HW, int inverse) {
    __shared__ double sd[LS_WAVES];
    __shared__ int si[LS_WAVES];
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    double term = 0.0;
    int valid = 0;
    if (p < P) {
        const long long b = p / HW;
        const long long base = b * (long long)D * HW + (p - b * HW);
        const float g = gt[p];
        const int k0 = inverse ? D - 1 : 0, step = inverse ? -1 : 1;
        float dprev = hyp[base + (long long)k0 * HW];
        const float x0 = logits[base + (long long)k0 * HW];
        float m = x0, s = 1.0f;                   // running maximum and sum of exp(x - m)
        float iv = 0.0f, dmin = 0.0f;
        int count = 0;
        for (int j = 1; j < D; ++j) {
            const long long o = base + (long long)(k0 + step * j) * HW;
            const float d = hyp[o], x = logits[o];
            iv = fabsf(d - dprev) / 2.0f;         // iv[j - 1]
            if (j == 1) dmin = dprev - iv;
            count += (dprev + iv <= g) ? 1 : 0;
            dprev = d;
            if (x > m) { s = s * expf(m - x) + 1.0f; m = x; }
            else s += expf(x - m);
        }
        const float dmax = dprev + iv;            // the last interval repeats
        count += (dmax <= g) ? 1 : 0;
        if (count > D - 1) count = D - 1;
        const float lse = m + logf(s);
        const bool out = (g < dmin) || (g > dmax);
        valid = (!out && mask[p] > 0.5f) ? 1 : 0;
        const int k = inverse ? D - 1 - count : count;
        index[p] = valid ? k : -1;
        lse_out[p] = lse;
        if (valid) term = (double)(lse - logits[base + (long long)k * HW]);
    }
    const double bs = block_sum(term, sd);
    const int bc = block_sum(valid, si);
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = bs;
        part_cnt[blockIdx.x] = bc;
    }
}

// loss = weight * sum / N (0 / 0 = NaN, as a mean over nothing), N
__global__ __launch_bounds__(kBlock) void loss_finalize_kernel(const double* __restrict__ part_sum, const int* __restrict__ part_cnt, int nparts,
                                                               double weight, float* __restrict__ loss, int* __restrict__ count) {
    __shared__ double sd[LS_WAVES];
    __shared__ int si[LS_WAVES];
    const double s = ordered_sum(part_sum, 1, nparts, sd);
    const int n = ordered_sum(part_cnt, 1, nparts, si);
    if (threadIdx.x == 0) {
        loss[0] = (float)(weight * (s / (double)n));
        count[0] = n;
    }
}

__global__ __launch_bounds__(kBlock) void ce_loss_bwd_kernel(const float* __restrict__ logits, const int* __restrict__ index,
                                                             const float* __restrict__ lse, const float* __restrict__ gout,
                                                             const int* __restrict__ count, double weight, float* __restrict__ grad, long long P,
                                                             int D, int HW) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const long long b = p / HW;
    const long long base = b * (long long)D * HW + (p - b * HW);
    const int k = index[p];
    if (k < 0) {                                  // masked or out of range (every pixel when N = 0)
        for (int j = 0; j < D; ++j) grad[base + (long long)j * HW] = 0.0f;
        return;
    }
    const float scale = (float)((double)gout[0] * weight / (double)count[0]);
    const float l = lse[p];
    for (int j = 0; j < D; ++j) {
        const long long o = base + (long long)j * HW;
        grad[o] = scale * (expf(logits[o] - l) - (j == k ? 1.0f : 0.0f));
    }
}

// ---- regression -------------------------------------------------------------------------------------------------------------------
// losses.py:64-97 without log_var, :118-149.  interval NULL = 1 (simple_loss), hyp NULL = no clamp.
struct RegPixel {
    float loss, dloss;      // the clamped smooth-L1 value and its derivative with respect to depth / interval
    float itv;
    int valid;
};

__device__ __forceinline__ RegPixel reg_pixel(const float* depth, const float* gt, const float* mask, const float* interval, const float* hyp,
                                              long long p, int D, int HW, int inverse) {
    RegPixel r;
    const long long b = p / HW;
    r.itv = interval ? interval[b] : 1.0f;
    r.valid = mask[p] > 0.5f ? 1 : 0;
    const float diff = depth[p] / r.itv - gt[p] / r.itv;
    const float a = fabsf(diff);
    r.loss = a < 1.0f ? 0.5f * a * a : a - 0.5f;                         // smooth L1, beta = 1
    r.dloss = a < 1.0f ? diff : (diff > 0.0f ? 1.0f : -1.0f);
    if (hyp) {
        const long long base = b * (long long)D * HW + (p - b * HW);
        const float dfirst = hyp[base + (long long)(inverse ? D - 1 : 0) * HW], dlast = hyp[base + (long long)(inverse ? 0 : D - 1) * HW];
        const float range = (dlast - dfirst) / r.itv;
        if (!(r.loss <= range)) r.dloss = 0.0f;                          // clamp_max passes the gradient where loss <= range
        if (r.loss > range || range != range) r.loss = range;           // a NaN on either side stays a NaN, as in torch.clamp_max
    }
    return r;
}

__global__ __launch_bounds__(kBlock) void reg_loss_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ gt,
                                                              const float* __restrict__ mask, const float* __restrict__ interval,
                                                              const float* __restrict__ hyp, double* __restrict__ part_sum,
                                                              int* __restrict__ part_cnt, long long P, int D, int HW, int inverse) {
    __shared__ double sd[LS_WAVES];
    __shared__ int si[LS_WAVES];
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    double term = 0.0;
    int valid = 0;
    if (p < P) {
        const RegPixel r = reg_pixel(depth, gt, mask, interval, hyp, p, D, HW, inverse);
        valid = r.valid;
        if (valid) term = (double)r.loss;
    }
    const double bs = block_sum(term, sd);
    const int bc = block_sum(valid, si);
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = bs;
        part_cnt[blockIdx.x] = bc;
    }
}

__global__ __launch_bounds__(kBlock) void reg_loss_bwd_kernel(const float* __restrict__ depth, const float* __restrict__ gt,
                                                              const float* __restrict__ mask, const float* __restrict__ interval,
                                                              const float* __restrict__ hyp, const float* __restrict__ gout,
                                                              const int* __restrict__ count, double weight, float* __restrict__ grad, long long P,
                                                              int D, int HW, int inverse) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const RegPixel r = reg_pixel(depth, gt, mask, interval, hyp, p, D, HW, inverse);
    if (!r.valid) {
        grad[p] = 0.0f;
        return;
    }
    const float scale = (float)((double)gout[0] * weight / (double)count[0]);
    grad[p] = scale * r.dloss / r.itv;
}

// ---- metrics ----------------------------------------------------------------------------------------------------------------------
// The thresholds are formed here: base = interval ? (double)interval[per_sample ? b : 0] / divisor : 1, value = (float)(base * factor) - the
// fp64 product of the reference's Python scalars, rounded to fp32 as torch rounds a scalar it compares with a fp32 tensor.  A band whose
// lower factor is NaN is "no band": every valid pixel, and NaN (not 0) when there is none.
struct MetricTable {
    double thres[MVS_METRICS_MAX_T], lo[MVS_METRICS_MAX_T], hi[MVS_METRICS_MAX_T];
    double divisor;
    int per_sample;
};

// workspace: doubles [B, nblk, T] (band sums), then ints [B, nblk, 1 + 2 T] (valid, T counts above the threshold, T counts inside the band)
__global__ __launch_bounds__(kBlock) void depth_metrics_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                               const void* __restrict__ mask, int mask_bytes, const float* __restrict__ interval,
                                                               MetricTable tab, int T, double* __restrict__ ws_sum, int* __restrict__ ws_cnt,
                                                               int HW) {
    __shared__ double sd[LS_WAVES];
    __shared__ int si[LS_WAVES];
    const int b = (int)blockIdx.y, nblk = (int)gridDim.x;
    const double base = interval ? (double)interval[tab.per_sample ? b : 0] / tab.divisor : 1.0;
    float thr[MVS_METRICS_MAX_T], lo[MVS_METRICS_MAX_T], hi[MVS_METRICS_MAX_T];
    int above[MVS_METRICS_MAX_T], inside[MVS_METRICS_MAX_T];
    double sum[MVS_METRICS_MAX_T];
    for (int t = 0; t < MVS_METRICS_MAX_T; ++t) {
        thr[t] = t < T ? (float)(base * tab.thres[t]) : 0.0f;
        lo[t] = t < T ? (float)(base * tab.lo[t]) : 0.0f;
        hi[t] = t < T ? (float)(base * tab.hi[t]) : 0.0f;
        above[t] = 0;
        inside[t] = 0;
        sum[t] = 0.0;
    }
    int valid = 0;
    const long long img = (long long)b * HW;
    for (int i = 0; i < MT_ITEMS; ++i) {
        const int q = (int)blockIdx.x * MT_TILE + i * kBlock + (int)threadIdx.x;
        if (q >= HW) break;
        const bool on = mask_bytes ? static_cast<const uint8_t*>(mask)[img + q] != 0 : static_cast<const float*>(mask)[img + q] > 0.5f;
        if (!on) continue;
        ++valid;
        const float err = fabsf(est[img + q] - gt[img + q]);
        for (int t = 0; t < MVS_METRICS_MAX_T; ++t) {
            if (t >= T) break;
            above[t] += err > thr[t] ? 1 : 0;
            if (lo[t] != lo[t] || (err >= lo[t] && err <= hi[t])) {
                ++inside[t];
                sum[t] += (double)err;
            }
        }
    }
    const long long slot = (long long)b * nblk + blockIdx.x;
    const int nv = block_sum(valid, si);
    if (threadIdx.x == 0) ws_cnt[slot * (1 + 2 * T)] = nv;
    for (int t = 0; t < MVS_METRICS_MAX_T; ++t) {
        if (t >= T) break;                        // T is uniform: every work-item leaves together
        const int na = block_sum(above[t], si), ni = block_sum(inside[t], si);
        const double s = block_sum(sum[t], sd);
        if (threadIdx.x == 0) {
            ws_cnt[slot * (1 + 2 * T) + 1 + t] = na;
            ws_cnt[slot * (1 + 2 * T) + 1 + T + t] = ni;
            ws_sum[slot * T + t] = s;
        }
    }
}

// one workgroup: counts [B, 1 + 2 T], sums [B, T], means [B + 1, 2 T] (per image: T ratios above the threshold, T band means; row B: the
// mean over the images)
__global__ __launch_bounds__(kBlock) void depth_metrics_finalize_kernel(const double* __restrict__ ws_sum, const int* __restrict__ ws_cnt, int nblk,
                                                                        int B, int T, int noband, int* __restrict__ counts,
                                                                        double* __restrict__ sums, float* __restrict__ means) {
    __shared__ double sd[LS_WAVES];
    __shared__ int si[LS_WAVES];
    __shared__ double batch[2 * MVS_METRICS_MAX_T];
    const int C = 1 + 2 * T;
    if (threadIdx.x < 2 * MVS_METRICS_MAX_T) batch[threadIdx.x] = 0.0;
    __syncthreads();
    for (int b = 0; b < B; ++b) {
        const int* wc = ws_cnt + (long long)b * nblk * C;
        const double* wd = ws_sum + (long long)b * nblk * T;
        const int nv = ordered_sum(wc, C, nblk, si);
        if (threadIdx.x == 0) counts[b * C] = nv;
        for (int t = 0; t < T; ++t) {
            const int na = ordered_sum(wc + 1 + t, C, nblk, si), ni = ordered_sum(wc + 1 + T + t, C, nblk, si);
            const double s = ordered_sum(wd + t, T, nblk, sd);
            if (threadIdx.x == 0) {
                counts[b * C + 1 + t] = na;
                counts[b * C + 1 + T + t] = ni;
                sums[b * T + t] = s;
                const double ratio = (double)na / (double)nv;                          // no valid pixel: 0 / 0 = NaN
                const double mean = (ni > 0 || ((noband >> t) & 1)) ? s / (double)ni : 0.0;     // an empty band: 0; no band, no pixel: NaN
                means[b * 2 * T + t] = (float)ratio;
                means[b * 2 * T + T + t] = (float)mean;
                batch[t] += ratio;
                batch[T + t] += mean;
            }
        }
    }
    if (threadIdx.x == 0)
        for (int t = 0; t < 2 * T; ++t) means[B * 2 * T + t] = (float)(batch[t] / (double)B);
}

static bool loss_dims_ok(int B, int D, int H, int W) {
    return B >= 1 && D >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL && (long long)B * H * W <= 0x7fffffffLL &&
           ceil_div((long long)B * H * W, kBlock) <= 0x7fffffffu;
}

}  // namespace mvs

using namespace mvs;

extern "C" size_t mvs_loss_workspace_bytes(long long pixels) {
    if (pixels < 1 || pixels > 0x7fffffffLL) return 0;
    return (size_t)ceil_div(pixels, kBlock) * (sizeof(double) + sizeof(int));
}

extern "C" int mvs_ce_loss_fwd(const float* logits, const float* hyp, const float* gt, const float* mask, int inverse, double weight, int* index,
                               float* lse, void* workspace, size_t workspace_bytes, float* loss, int* count, int B, int D, int H, int W,
                               void* stream) {
    if (!logits || !hyp || !gt || !mask || !index || !lse || !workspace || !loss || !count || !loss_dims_ok(B, D, H, W) || D < 2) {
        set_error("mvs_ce_loss_fwd: bad arguments (B, H, W >= 1, D >= 2, B H W < 2^31)");
        return MVS_ERR_ARG;
    }
    const long long P = (long long)B * H * W;
    const unsigned nb = ceil_div(P, kBlock);
    if (workspace_bytes < mvs_loss_workspace_bytes(P) || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
        set_error("mvs_ce_loss_fwd: the workspace needs mvs_loss_workspace_bytes(B H W) bytes, 8-byte aligned");
        return MVS_ERR_ARG;
    }
    double* ps = static_cast<double*>(workspace);
    int* pc = reinterpret_cast<int*>(ps + nb);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_loss_fwd_kernel, dim3(nb), dim3(kBlock), 0, st, logits, hyp, gt, mask, index, lse, ps, pc, P, D, H * W, inverse ? 1 : 0);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ps, (const int*)pc, (int)nb, weight, loss, count);
    return check_launch("ce_loss_fwd_kernel");
}

extern "C" int mvs_ce_loss_bwd(const float* logits, const int* index, const float* lse, const float* grad_loss, const int* count, double weight,
                               float* grad_logits, int B, int D, int H, int W, void* stream) {
    if (!logits || !index || !lse || !grad_loss || !count || !grad_logits || !loss_dims_ok(B, D, H, W) || D < 2) {
        set_error("mvs_ce_loss_bwd: bad arguments (B, H, W >= 1, D >= 2, B H W < 2^31)");
        return MVS_ERR_ARG;
    }
    const long long P = (long long)B * H * W;
    hipLaunchKernelGGL(ce_loss_bwd_kernel, dim3(ceil_div(P, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, logits, index, lse, grad_loss, count,
                       weight, grad_logits, P, D, H * W);
    return check_launch("ce_loss_bwd_kernel");
}

extern "C" int mvs_reg_loss_fwd(const float* depth, const float* gt, const float* mask, const float* interval, const float* hyp, int inverse,
                                double weight, void* workspace, size_t workspace_bytes, float* loss, int* count, int B, int D, int H, int W,
                                void* stream) {
    if (!depth || !gt || !mask || !workspace || !loss || !count || !loss_dims_ok(B, D, H, W)) {
        set_error("mvs_reg_loss_fwd: bad arguments (B, D, H, W >= 1, B H W < 2^31)");
        return MVS_ERR_ARG;
    }
    const long long P = (long long)B * H * W;
    const unsigned nb = ceil_div(P, kBlock);
    if (workspace_bytes < mvs_loss_workspace_bytes(P) || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
        set_error("mvs_reg_loss_fwd: the workspace needs mvs_loss_workspace_bytes(B H W) bytes, 8-byte aligned");
        return MVS_ERR_ARG;
    }
    double* ps = static_cast<double*>(workspace);
    int* pc = reinterpret_cast<int*>(ps + nb);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reg_loss_fwd_kernel, dim3(nb), dim3(kBlock), 0, st, depth, gt, mask, interval, hyp, ps, pc, P, D, H * W, inverse ? 1 : 0);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ps, (const int*)pc, (int)nb, weight, loss, count);
    return check_launch("reg_loss_fwd_kernel");
}

extern "C" int mvs_reg_loss_bwd(const float* depth, const float* gt, const float* mask, const float* interval, const float* hyp, int inverse,
                                const float* grad_loss, const int* count, double weight, float* grad_depth, int B, int D, int H, int W,
                                void* stream) {
    if (!depth || !gt || !mask || !grad_loss || !count || !grad_depth || !loss_dims_ok(B, D, H, W)) {
        set_error("mvs_reg_loss_bwd: bad arguments (B, D, H, W >= 1, B H W < 2^31)");
        return MVS_ERR_ARG;
    }
    const long long P = (long long)B * H * W;
    hipLaunchKernelGGL(reg_loss_bwd_kernel, dim3(ceil_div(P, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, depth, gt, mask, interval, hyp,
                       grad_loss, count, weight, grad_depth, P, D, H * W, inverse ? 1 : 0);
    return check_launch("reg_loss_bwd_kernel");
}

static bool metrics_dims_ok(int B, int H, int W, int T) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - MT_TILE && (long long)B * H * W <= 0x7fffffffLL &&
           T >= 1 && T <= MVS_METRICS_MAX_T;
}

extern "C" size_t mvs_depth_metrics_workspace_bytes(int B, int H, int W, int T) {
    if (!metrics_dims_ok(B, H, W, T)) return 0;
    return (size_t)B * ceil_div((long long)H * W, MT_TILE) * ((size_t)T * sizeof(double) + (size_t)(1 + 2 * T) * sizeof(int));
}

extern "C" int mvs_depth_metrics(const float* est, const float* gt, const void* mask, int mask_bytes, const float* interval, double divisor,
                                 int per_sample, const double* thres, const double* band_lo, const double* band_hi, int T, void* workspace,
                                 size_t workspace_bytes, int* counts, double* sums, float* means, int B, int H, int W, void* stream) {
    if (!est || !gt || !mask || !thres || !band_lo || !band_hi || !workspace || !counts || !sums || !means || !metrics_dims_ok(B, H, W, T) ||
        !(divisor > 0.0)) {
        set_error("mvs_depth_metrics: bad arguments (1 <= B <= 65535, H, W >= 1, B H W < 2^31, 1 <= T <= %d, divisor > 0)", MVS_METRICS_MAX_T);
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_depth_metrics_workspace_bytes(B, H, W, T) || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
        set_error("mvs_depth_metrics: the workspace needs mvs_depth_metrics_workspace_bytes(B, H, W, T) bytes, 8-byte aligned");
        return MVS_ERR_ARG;
    }
    MetricTable tab;
    int noband = 0;
    for (int t = 0; t < MVS_METRICS_MAX_T; ++t) {
        tab.thres[t] = t < T ? thres[t] : 0.0;
        tab.lo[t] = t < T ? band_lo[t] : 0.0;
        tab.hi[t] = t < T ? band_hi[t] : 0.0;
        if (t < T && band_lo[t] != band_lo[t]) noband |= 1 << t;
    }
    tab.divisor = divisor;
    tab.per_sample = per_sample ? 1 : 0;
    const unsigned nblk = ceil_div((long long)H * W, MT_TILE);
    double* wd = static_cast<double*>(workspace);
    int* wc = reinterpret_cast<int*>(wd + (size_t)B * nblk * T);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_kernel, dim3(nblk, B), dim3(kBlock), 0, st, est, gt, mask, mask_bytes ? 1 : 0, interval, tab, T, wd, wc, H * W);
    hipLaunchKernelGGL(depth_metrics_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)wd, (const int*)wc, (int)nblk, B, T, noband,
                       counts, sums, means);
    return check_launch("depth_metrics_kernel");
}
