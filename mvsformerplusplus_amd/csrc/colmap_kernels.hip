// colmap2mvsnet view selection (colmap2mvsnet.py:378-410) and depth values (:344-357) on the device, fp64 throughout
// (DESIGN.md section 4.9).  For images i < j the score is
//
//   score[i][j] = sum over the entries p of image i's point3D_ids (duplicates counted, -1 skipped) that occur in image j's list of
//                 g(theta),  cos = (dot(Ci - p, Cj - p) / |Ci - p|) / |Cj - p|,  theta = (180 / pi) acos(clamp(cos, -1, 1)),
//                 g = exp(-(theta - theta0)^2 / (2 sigma^2)), sigma = sigma1 if theta <= theta0 else sigma2
//
// mirrored to score[j][i]; the diagonal and pairs that share nothing stay 0.  A point at a camera centre contributes 0.
//
// The host hands over a per-image CSR of sorted unique dense point indices with their multiplicity in that image, and a per-point
// CSR of its unique images in ascending order (the track).  Five launches on the caller's stream, none waits for another
// workgroup, no atomics, so the result is the same bits on every run:
//   A  colmap_covis_kernel     one work-item per point: flags[a][b] = 1 for every pair a < b of its track (plain stores of one
//                              constant: order-free);
//   B  colmap_count_kernel,    compaction of the flagged pairs into a list i * N + j in row-major order: per-tile counts, one
//      colmap_scan_kernel,     workgroup's scan of the tile counts (writes the pair count), scatter - the point-cloud compaction
//      colmap_scatter_kernel   pattern of pointcloud_kernels.hip;
//   C  colmap_score_kernel     one wave per pair: walk the shorter sorted list, binary-search the longer, weight each hit by the
//                              multiplicity in image i, sum per lane in index order, then a fixed xor-butterfly across the wave;
//                              one lane writes score[i][j] and score[j][i].
// The flag and score matrices take 9 N^2 bytes; the caller keeps N <= 16384.
#include "mvs_common.h"

namespace mvs {

constexpr int kCmThreads = 256;
constexpr int kCmBytes = 4;                            // flag bytes per work-item in the compaction
constexpr int kCmTile = kCmThreads * kCmBytes;         // flag bytes per workgroup
constexpr int kCmMaxScoreBlocks = 16384;               // pass C: 65536 waves at most, each loops over its share of pairs

struct ColmapScoreParams {
    double theta0, den1, den2;                         // den = 2 * sigma^2, formed by the caller as the reference forms it
};

// exclusive prefix sum over the workgroup in threadIdx.x order (same scheme as pointcloud_kernels.hip's pc_block_scan)
__device__ __forceinline__ unsigned cm_block_scan(unsigned v, unsigned* wsum, unsigned& total) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl(x, lane - d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kCmThreads / 64; ++i) {
        const unsigned s = wsum[i];
        before += i < wave ? s : 0u;
        total += s;
    }
    __syncthreads();
    return before + x - v;
}

__device__ __forceinline__ unsigned cm_flag_bits(const uint8_t* __restrict__ flags, int f0, int NN) {
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < kCmBytes; ++j)
        if (f0 + j < NN && flags[f0 + j] != 0) bits |= 1u << j;
    return bits;
}

__device__ __forceinline__ unsigned cm_count4(unsigned b) { return (b & 1u) + ((b >> 1) & 1u) + ((b >> 2) & 1u) + ((b >> 3) & 1u); }

// z of observation k under [R | t] of its image: erow = row 2 of E, [N, 4]; summed left to right, no fused multiply-adds
__global__ __launch_bounds__(kCmThreads) void colmap_depth_kernel(const int* __restrict__ obs_img, const int* __restrict__ obs_pt, int n,
                                                                  const double* __restrict__ xyz, const double* __restrict__ erow,
                                                                  double* __restrict__ z) {
#pragma clang fp contract(off)
    const int k = (int)blockIdx.x * kCmThreads + (int)threadIdx.x;
    if (k >= n) return;
    const double* e = erow + 4 * (size_t)obs_img[k];
    const double* X = xyz + 3 * (size_t)obs_pt[k];
    z[k] = e[0] * X[0] + e[1] * X[1] + e[2] * X[2] + e[3];
}

__global__ __launch_bounds__(kCmThreads) void colmap_covis_kernel(const int* __restrict__ pt_ptr, const int* __restrict__ pt_imgs, int P, int N,
                                                                  uint8_t* __restrict__ flags) {
    const int p = (int)blockIdx.x * kCmThreads + (int)threadIdx.x;
    if (p >= P) return;
    const int a1 = pt_ptr[p + 1];
    for (int a = pt_ptr[p]; a < a1; ++a) {
        uint8_t* row = flags + (size_t)pt_imgs[a] * N;
        for (int b = a + 1; b < a1; ++b) row[pt_imgs[b]] = 1;
    }
}

__global__ __launch_bounds__(kCmThreads) void colmap_count_kernel(const uint8_t* __restrict__ flags, int NN, unsigned* __restrict__ tile_counts) {
    __shared__ unsigned wsum[kCmThreads / 64];
    const unsigned bits = cm_flag_bits(flags, (int)blockIdx.x * kCmTile + (int)threadIdx.x * kCmBytes, NN);
    unsigned total;
    cm_block_scan(cm_count4(bits), wsum, total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one workgroup: tile_offsets[t] = sum of tile_counts[< t]; counter[0] = number of flagged pairs
__global__ __launch_bounds__(kCmThreads) void colmap_scan_kernel(const unsigned* __restrict__ tile_counts, unsigned* __restrict__ tile_offsets,
                                                                 int ntiles, unsigned* __restrict__ counter) {
    __shared__ unsigned wsum[kCmThreads / 64];
    const int per = (ntiles + kCmThreads - 1) / kCmThreads;
    const int t0 = (int)threadIdx.x * per < ntiles ? (int)threadIdx.x * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    unsigned s = 0;
    for (int t = t0; t < t1; ++t) s += tile_counts[t];
    unsigned total;
    unsigned off = cm_block_scan(s, wsum, total);
    for (int t = t0; t < t1; ++t) {
        tile_offsets[t] = off;
        off += tile_counts[t];
    }
    if (threadIdx.x == 0) counter[0] = total;
}

__global__ __launch_bounds__(kCmThreads) void colmap_scatter_kernel(const uint8_t* __restrict__ flags, int NN, const unsigned* __restrict__ tile_offsets,
                                                                    unsigned* __restrict__ pairs, unsigned cap) {
    __shared__ unsigned wsum[kCmThreads / 64];
    const int f0 = (int)blockIdx.x * kCmTile + (int)threadIdx.x * kCmBytes;
    const unsigned bits = cm_flag_bits(flags, f0, NN);
    unsigned total;
    unsigned r = tile_offsets[blockIdx.x] + cm_block_scan(cm_count4(bits), wsum, total);
#pragma unroll
    for (int j = 0; j < kCmBytes; ++j) {
        if (!((bits >> j) & 1u)) continue;
        if (r < cap) pairs[r] = (unsigned)(f0 + j);
        ++r;
    }
}

// g(theta) of point X seen from centres ci, cj; every product and sum in the oracle's order, no fused multiply-adds
__device__ __forceinline__ double colmap_g(const double* __restrict__ X, const double ci[3], const double cj[3], const ColmapScoreParams& prm) {
#pragma clang fp contract(off)
    const double ax = ci[0] - X[0], ay = ci[1] - X[1], az = ci[2] - X[2];
    const double bx = cj[0] - X[0], by = cj[1] - X[1], bz = cj[2] - X[2];
    const double na = sqrt(ax * ax + ay * ay + az * az), nb = sqrt(bx * bx + by * by + bz * bz);
    if (na == 0.0 || nb == 0.0) return 0.0;
    double c = (ax * bx + ay * by + az * bz) / na / nb;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double theta = (180.0 / 3.14159265358979311600) * acos(c);
    const double d = theta - prm.theta0;
    return exp(-d * d / (theta <= prm.theta0 ? prm.den1 : prm.den2));
}

__global__ __launch_bounds__(kCmThreads) void colmap_score_kernel(const unsigned* __restrict__ pairs, const unsigned* __restrict__ counter,
                                                                  unsigned cap, int N, const int* __restrict__ img_ptr,
                                                                  const int* __restrict__ img_pts, const int* __restrict__ img_mult,
                                                                  const double* __restrict__ xyz, const double* __restrict__ centres,
                                                                  ColmapScoreParams prm, double* __restrict__ score) {
    const unsigned n = counter[0] < cap ? counter[0] : cap;
    const int lane = (int)(threadIdx.x & 63);
    const unsigned nw = gridDim.x * (kCmThreads / 64);
    for (unsigned q = blockIdx.x * (kCmThreads / 64) + (threadIdx.x >> 6); q < n; q += nw) {     // wave-uniform loop
        const unsigned ij = pairs[q];
        const int i = (int)(ij / (unsigned)N), j = (int)(ij % (unsigned)N);
        const int a0 = img_ptr[i], a1 = img_ptr[i + 1], b0 = img_ptr[j], b1 = img_ptr[j + 1];
        const bool i_short = a1 - a0 <= b1 - b0;
        const int s0 = i_short ? a0 : b0, s1 = i_short ? a1 : b1, l0 = i_short ? b0 : a0, l1 = i_short ? b1 : a1;
        const double ci[3] = {centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]};
        const double cj[3] = {centres[3 * j], centres[3 * j + 1], centres[3 * j + 2]};
        double acc = 0.0;
        for (int k = s0 + lane; k < s1; k += 64) {
            const int p = img_pts[k];
            int lo = l0, hi = l1;                      // lower bound of p in the longer list
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (img_pts[mid] < p) lo = mid + 1;
                else hi = mid;
            }
            if (lo < l1 && img_pts[lo] == p) acc += (double)img_mult[i_short ? k : lo] * colmap_g(xyz + 3 * (size_t)p, ci, cj, prm);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) {
            score[(size_t)i * N + j] = acc;
            score[(size_t)j * N + i] = acc;
        }
    }
}

}  // namespace mvs

using namespace mvs;

static long long cm_tiles(int N) { return ((long long)N * N + kCmTile - 1) / kCmTile; }

extern "C" size_t mvs_colmap_workspace_bytes(int N) {
    if (N < 1 || N > 16384) return 0;
    return sizeof(unsigned) * (2 * (size_t)cm_tiles(N) + 1);
}

extern "C" int mvs_colmap_depths(const int* obs_img, const int* obs_pt, long long n, const double* xyz, const double* erow, double* z,
                                 void* stream) {
    if (!obs_img || !obs_pt || !xyz || !erow || !z || n < 0 || n > 0x7fffffffLL - kCmThreads) {
        set_error("mvs_colmap_depths: bad arguments (n = %lld)", n);
        return MVS_ERR_ARG;
    }
    if (n == 0) return MVS_OK;
    hipLaunchKernelGGL(colmap_depth_kernel, dim3((unsigned)((n + kCmThreads - 1) / kCmThreads)), dim3(kCmThreads), 0, (hipStream_t)stream,
                       obs_img, obs_pt, (int)n, xyz, erow, z);
    return check_launch("colmap_depth_kernel");
}

extern "C" int mvs_colmap_scores(const int* img_ptr, const int* img_pts, const int* img_mult, int N, const int* pt_ptr, const int* pt_imgs,
                                 int P, const double* xyz, const double* centres, double theta0, double den1, double den2,
                                 long long max_pairs, uint8_t* flags, unsigned* pairs, void* workspace, size_t workspace_bytes,
                                 double* score, void* stream) {
    if (!img_ptr || !img_pts || !img_mult || !pt_ptr || !pt_imgs || !xyz || !centres || !flags || !score || !workspace || P < 0 ||
        max_pairs < 0 || (max_pairs > 0 && !pairs)) {
        set_error("mvs_colmap_scores: bad arguments");
        return MVS_ERR_ARG;
    }
    if (N < 1 || N > 16384 || max_pairs > (long long)N * (N - 1) / 2 || P > 0x7fffffffLL - kCmThreads) {
        set_error("mvs_colmap_scores: N = %d (1..16384), P = %d or max_pairs = %lld out of range", N, P, max_pairs);
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_colmap_workspace_bytes(N)) { set_error("mvs_colmap_scores: workspace too small"); return MVS_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const size_t NN = (size_t)N * N;
    if (hipMemsetAsync(flags, 0, NN, st) != hipSuccess || hipMemsetAsync(score, 0, NN * sizeof(double), st) != hipSuccess) {
        set_error("mvs_colmap_scores: hipMemsetAsync failed");
        return MVS_ERR_LAUNCH;
    }
    if (max_pairs == 0 || P == 0) return MVS_OK;
    const int nt = (int)cm_tiles(N);
    unsigned* tile_counts = static_cast<unsigned*>(workspace);
    unsigned* tile_offsets = tile_counts + nt;
    unsigned* counter = tile_offsets + nt;
    hipLaunchKernelGGL(colmap_covis_kernel, dim3((unsigned)((P + kCmThreads - 1) / kCmThreads)), dim3(kCmThreads), 0, st, pt_ptr, pt_imgs, P, N, flags);
    int rc = check_launch("colmap_covis_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(colmap_count_kernel, dim3((unsigned)nt), dim3(kCmThreads), 0, st, (const uint8_t*)flags, (int)NN, tile_counts);
    if ((rc = check_launch("colmap_count_kernel")) != MVS_OK) return rc;
    hipLaunchKernelGGL(colmap_scan_kernel, dim3(1), dim3(kCmThreads), 0, st, (const unsigned*)tile_counts, tile_offsets, nt, counter);
    if ((rc = check_launch("colmap_scan_kernel")) != MVS_OK) return rc;
    hipLaunchKernelGGL(colmap_scatter_kernel, dim3((unsigned)nt), dim3(kCmThreads), 0, st, (const uint8_t*)flags, (int)NN,
                       (const unsigned*)tile_offsets, pairs, (unsigned)max_pairs);
    if ((rc = check_launch("colmap_scatter_kernel")) != MVS_OK) return rc;
    const long long waves_per_block = kCmThreads / 64;
    const long long blocks = (max_pairs + waves_per_block - 1) / waves_per_block;
    const ColmapScoreParams prm{theta0, den1, den2};
    hipLaunchKernelGGL(colmap_score_kernel, dim3((unsigned)(blocks < kCmMaxScoreBlocks ? blocks : kCmMaxScoreBlocks)), dim3(kCmThreads), 0, st,
                       (const unsigned*)pairs, (const unsigned*)counter, (unsigned)max_pairs, N, img_ptr, img_pts, img_mult, xyz, centres, prm, score);
    return check_launch("colmap_score_kernel");
}
