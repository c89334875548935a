// Point-cloud output of the depth-map filtering ("back-project -> PLY"): the per-view body of the two
// drivers in test.py after the filter (filter_depth :414-442, dynamic_filter_depth :485-517) - keep the pixels of the final mask,
// take their world points and the reference image's colours, and concatenate the views into ONE binary PLY.
//
// Here the kept pixels of a view are compacted on the device, in row-major order, into packed 15-byte little-endian records
// {float x, y, z; uchar r, g, b} - exactly the PLY body - appended to a scene buffer at the offset held in a device counter.  Three
// launches on the caller's stream, no workgroup ever waits for another (dispatch order is undefined):
//   1. pc_count_kernel    kept pixels per tile of 1024 pixels;
//   2. pc_scan_kernel     ONE workgroup: exclusive scan of the tile counts from the scene counter, advances the counter;
//   3. pc_scatter_kernel  every tile re-derives its in-tile offsets, stages its records in LDS and writes its contiguous byte
//                         range with dword stores (bytes only at the two partial dwords of the range).
// Bytes per pixel: 1 (mask, step 1) + 1 (mask, step 3) + kept fraction * (12 points + 3 colours + 15 record).
#include "mvs_common.h"

namespace mvs {

constexpr int kPcThreads = 256;
constexpr int kPcPix = 4;                              // consecutive pixels per work-item
constexpr int kPcTile = kPcThreads * kPcPix;           // pixels per workgroup
constexpr int kPcRecord = 15;                          // bytes per PLY vertex record

// exclusive prefix sum of `v` over the workgroup (threadIdx.x order); `total` = the workgroup's sum.  Wave scan with __shfl from
// lane - d, then the four wave sums through LDS.  Every work-item of the workgroup must call it.
__device__ __forceinline__ unsigned pc_block_scan(unsigned v, unsigned* wsum, unsigned& total) {
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
    for (int i = 0; i < kPcThreads / 64; ++i) {
        const unsigned s = wsum[i];
        before += i < wave ? s : 0u;
        total += s;
    }
    __syncthreads();                                   // wsum may be reused after the return
    return before + x - v;
}

// bit j set = pixel p0 + j is kept
__device__ __forceinline__ unsigned pc_keep_bits(const uint8_t* __restrict__ mask, int p0, int HW) {
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < kPcPix; ++j)
        if (p0 + j < HW && mask[p0 + j] != 0) keep |= 1u << j;
    return keep;
}

__device__ __forceinline__ unsigned pc_count4(unsigned keep) { return (keep & 1u) + ((keep >> 1) & 1u) + ((keep >> 2) & 1u) + ((keep >> 3) & 1u); }

__global__ __launch_bounds__(kPcThreads) void pc_count_kernel(const uint8_t* __restrict__ mask, int HW, unsigned* __restrict__ tile_counts) {
    __shared__ unsigned wsum[kPcThreads / 64];
    const int p0 = (int)blockIdx.x * kPcTile + (int)threadIdx.x * kPcPix;
    const unsigned keep = pc_keep_bits(mask, p0, HW);
    unsigned total;
    pc_block_scan(pc_count4(keep), wsum, total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one workgroup: tile_offsets[t] = *counter + sum of tile_counts[< t]; *counter += total; view_counts[view_slot] = total
__global__ __launch_bounds__(kPcThreads) void pc_scan_kernel(const unsigned* __restrict__ tile_counts, unsigned* __restrict__ tile_offsets,
                                                             int ntiles, unsigned* __restrict__ counter, unsigned* __restrict__ view_counts,
                                                             int view_slot) {
    __shared__ unsigned wsum[kPcThreads / 64];
    const unsigned base = counter[0];
    const int per = (ntiles + kPcThreads - 1) / kPcThreads;
    const int t0 = (int)threadIdx.x * per < ntiles ? (int)threadIdx.x * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    unsigned s = 0;
    for (int t = t0; t < t1; ++t) s += tile_counts[t];
    unsigned total;
    unsigned off = base + pc_block_scan(s, wsum, total);
    for (int t = t0; t < t1; ++t) {
        tile_offsets[t] = off;
        off += tile_counts[t];
    }
    if (threadIdx.x == 0) {                           // every work-item read `base` before the scan's barriers
        counter[0] = base + total;
        if (view_counts != nullptr) view_counts[view_slot] = total;
    }
}

__global__ __launch_bounds__(kPcThreads) void pc_scatter_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ points,
                                                                const uint8_t* __restrict__ rgb, int HW, const unsigned* __restrict__ tile_offsets,
                                                                uint8_t* __restrict__ records, unsigned long long cap_bytes) {
    __shared__ unsigned wsum[kPcThreads / 64];
    __shared__ unsigned stage[(kPcTile * kPcRecord) / 4 + 2];   // the tile's records, shifted by the range's misalignment (<= 3 B)
    uint8_t* st = reinterpret_cast<uint8_t*>(stage);
    const int p0 = (int)blockIdx.x * kPcTile + (int)threadIdx.x * kPcPix;
    const unsigned keep = pc_keep_bits(mask, p0, HW);
    unsigned total;
    unsigned r = pc_block_scan(pc_count4(keep), wsum, total);
    if (total == 0) return;                            // uniform over the workgroup
    const unsigned long long g0 = (unsigned long long)tile_offsets[blockIdx.x] * kPcRecord, g1 = g0 + (unsigned long long)total * kPcRecord;
    const unsigned head = (unsigned)(g0 & 3ull);
#pragma unroll
    for (int j = 0; j < kPcPix; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const int p = p0 + j;
        uint8_t* d = st + head + r * kPcRecord;
        const float xyz[3] = {points[p], points[(size_t)HW + p], points[2 * (size_t)HW + p]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            union { float f; uint32_t u; } c;
            c.f = xyz[k];
            d[4 * k] = (uint8_t)c.u; d[4 * k + 1] = (uint8_t)(c.u >> 8); d[4 * k + 2] = (uint8_t)(c.u >> 16); d[4 * k + 3] = (uint8_t)(c.u >> 24);
        }
        d[12] = rgb[3 * (size_t)p]; d[13] = rgb[3 * (size_t)p + 1]; d[14] = rgb[3 * (size_t)p + 2];
        ++r;
    }
    __syncthreads();
    // global byte a0 + i sits at stage byte i; whole dwords inside [g0, g1) go out as dword stores, the <= 2 partial ones byte-wise
    const unsigned long long a0 = g0 - head, end = g1 < cap_bytes ? g1 : cap_bytes;
    const int ndw = (int)((g1 - a0 + 3) >> 2);
    for (int i = (int)threadIdx.x; i < ndw; i += kPcThreads) {
        const unsigned long long a = a0 + 4ull * (unsigned long long)i;
        if (a >= g0 && a + 4 <= end) {
            *reinterpret_cast<uint32_t*>(records + a) = stage[i];
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (a + b >= g0 && a + b < end) records[a + b] = st[4 * i + b];
        }
    }
}

}  // namespace mvs

using namespace mvs;

static int pc_tiles(int h, int w) { return (int)(((long long)h * w + kPcTile - 1) / kPcTile); }

extern "C" size_t mvs_pointcloud_workspace_bytes(int h, int w) {
    if (h < 1 || w < 1) return 0;
    return 2 * sizeof(unsigned) * (size_t)pc_tiles(h, w);
}

extern "C" int mvs_pointcloud_append(const uint8_t* mask, const float* points, const uint8_t* rgb, int h, int w, void* workspace,
                                     size_t workspace_bytes, unsigned* counter, unsigned* view_counts, int view_slot, uint8_t* records,
                                     long long capacity, void* stream) {
    if (!mask || !points || !rgb || !workspace || !counter || !records || h < 1 || w < 1 || capacity < 0 || view_slot < 0) {
        set_error("mvs_pointcloud_append: bad arguments");
        return MVS_ERR_ARG;
    }
    if ((long long)h * w > 0x7fffffffLL - kPcTile || capacity > 0xffffffffLL) { set_error("mvs_pointcloud_append: view or capacity too large"); return MVS_ERR_ARG; }
    if (((uintptr_t)records & 3) != 0) { set_error("mvs_pointcloud_append: records must be 4-byte aligned"); return MVS_ERR_ARG; }
    if (workspace_bytes < mvs_pointcloud_workspace_bytes(h, w)) { set_error("mvs_pointcloud_append: workspace too small"); return MVS_ERR_WORKSPACE; }
    const int HW = h * w, nt = pc_tiles(h, w);
    unsigned* tile_counts = static_cast<unsigned*>(workspace);
    unsigned* tile_offsets = tile_counts + nt;
    hipLaunchKernelGGL(pc_count_kernel, dim3((unsigned)nt), dim3(kPcThreads), 0, (hipStream_t)stream, mask, HW, tile_counts);
    int rc = check_launch("pc_count_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(kPcThreads), 0, (hipStream_t)stream, (const unsigned*)tile_counts, tile_offsets, nt, counter,
                       view_counts, view_slot);
    rc = check_launch("pc_scan_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL(pc_scatter_kernel, dim3((unsigned)nt), dim3(kPcThreads), 0, (hipStream_t)stream, mask, points, rgb, HW,
                       (const unsigned*)tile_offsets, records, (unsigned long long)capacity * kPcRecord);
    return check_launch("pc_scatter_kernel");
}
