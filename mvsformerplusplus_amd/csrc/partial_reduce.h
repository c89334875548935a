// Fixed-order reduction of per-workgroup fp32 partials: the weight-gradient kernels of the feature side (fmt_kernels.hip,
// fpn_train_kernels.hip, fpn_encoder_train_kernels.hip) leave one partial per workgroup and this kernel adds them; no atomics, so a gradient is the same bits from
// run to run.
#pragma once
#include "mvs_common.h"

namespace mvs {

constexpr int FT_RED_SEG = 16;                // segments of consecutive partials per output element in the reduction

// out[e] = the sum of part[p][e] over the launch's partials in a fixed order: FT_RED_SEG segments of consecutive partials, each added
// front to back by one thread, then the segment sums front to back.
static __global__ __launch_bounds__(256) void fmt_partial_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts, int nelem) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* seg = reinterpret_cast<float*>(lds4);                  // [FT_RED_SEG][16]
    const int tid = (int)threadIdx.x, e = (int)blockIdx.x * 16 + (tid & 15), s = tid >> 4;
    const int per = (nparts + FT_RED_SEG - 1) / FT_RED_SEG, p0 = s * per, p1 = p0 + per < nparts ? p0 + per : nparts;
    float sum = 0.0f;
    if (e < nelem)
        for (int p = p0; p < p1; ++p) sum += part[(size_t)p * nelem + e];
    seg[tid] = sum;
    __syncthreads();
    if (tid < 16 && e < nelem) {
        float t = seg[tid];
#pragma unroll
        for (int k = 1; k < FT_RED_SEG; ++k) t += seg[k * 16 + tid];
        out[e] = t;
    }
}

static int ft_reduce_partials(const float* part, float* out, int nparts, int nelem, hipStream_t st) {
    hipLaunchKernelGGL(fmt_partial_reduce_kernel, dim3(ceil_div(nelem, 16)), dim3(256), 256 * sizeof(float), st, part, out, nparts, nelem);
    return check_launch("fmt_partial_reduce_kernel");
}

}  // namespace mvs
