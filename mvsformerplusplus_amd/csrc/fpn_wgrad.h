// Weight gradients of the FPN's convolutions on the exact-fp32 v_mfma_f32_16x16x4_f32: the kernel template that the decoder's training
// unit (fpn_train_kernels.hip: stride 1, 64 input channels, merge source) and the encoder's (fpn_encoder_train_kernels.hip: 3 .. 64 input
// channels, 3x3 .. 7x7 taps, stride 1 | 2) instantiate.
//
// dW[co][ci][ky][kx] = sum_pixels dY[co][y][x] X[ci][S y + ky - K/2][S x + kx - K/2] as a GEMM: rows = co (16 per row block), columns =
// (ci, tap) = the weights of one output channel in memory order, K dimension = the pixels of a TH x 64 tile of dY.  The source's tile and
// halo ((TH - 1) S + K rows x 63 S + K columns) are staged into LDS (zero outside the image) and the B operand is read at stride S.  Wave v
// owns the column blocks v, v + 4, ..: its accumulators are final for the workgroup, which keeps them over all of its tiles and writes one
// partial.  Partials are added in a fixed order (partial_reduce.h): no atomic, the same bits from run to run.
#pragma once
#include "conv2d_split.h"
#include "partial_reduce.h"

namespace mvs {

template <int COUT, int CIN, int K, bool ONES, int S = 1>
struct FpnWgradShape {
    static constexpr int P = K / 2, TH = COUT >= 32 ? 2 : 4, TW = 64, NPIX = TH * TW;
    static constexpr int CT = CIN + (ONES ? 1 : 0);                   // staged planes: the input channels (+ the plane of ones)
    static constexpr int SH = (TH - 1) * S + K, SW = (TW - 1) * S + K; // staged rows / columns of X
    static constexpr int RS = SW > TW + 4 ? SW : TW + 4, PL = SH * RS + 1;  // staged row / channel-plane strides of X
    static constexpr int DSS = NPIX + 4;                              // channel stride of the staged dY: lane (co, k) reads bank 4 co + k
    static constexpr int NRB = (COUT + 15) / 16, NCOL = CT * K * K, NCB = (NCOL + 15) / 16, NCBW = (NCB + 3) / 4;
    static constexpr int LDS = (CT * PL + COUT * DSS) * (int)sizeof(float);
    static_assert((CIN % 8 == 0 || CIN == 3) && LDS <= 160 * 1024, "input channels come in octets (or the image's three); the tile must fit the LDS");
    static_assert(S == 1 || S == 2, "stride 1 or 2");
};

constexpr long long FW_PART_BYTES = 8 << 20;  // partials of one launch: at most this much workspace ..
constexpr int FW_MAX_PARTS = 256;             // .. and at most this many (= workgroups)

template <int COUT, int CIN, int K, bool ONES>
static int fw_parts(long long ntile) {
    typedef FpnWgradShape<COUT, CIN, K, ONES> F;
    long long cap = FW_PART_BYTES / ((long long)COUT * F::NCOL * (long long)sizeof(float));
    cap = cap < FW_MAX_PARTS ? cap : FW_MAX_PARTS;
    return (int)(ntile < cap ? ntile : cap);
}

// tiles of dY [N, COUT, OH, OW]
template <int COUT, int CIN, int K, bool ONES>
static long long fw_tiles(int N, int OH, int OW) {
    typedef FpnWgradShape<COUT, CIN, K, ONES> F;
    return (long long)N * ceil_div(OH, F::TH) * ceil_div(OW, F::TW);
}

template <int COUT, int CIN, int K, bool ONES>
static size_t fw_workspace(int N, int OH, int OW) {
    const long long tiles = fw_tiles<COUT, CIN, K, ONES>(N, OH, OW);
    if (tiles > 0x7fffffffLL) return 0;
    return (size_t)fw_parts<COUT, CIN, K, ONES>(tiles) * COUT * FpnWgradShape<COUT, CIN, K, ONES>::NCOL * sizeof(float);
}

// src: X [N, CIN, H, W]; dy [N, COUT, OH, OW], OH = (H - 1) / S + 1
template <int COUT, int CIN, int K, bool ONES, int S, class Src>
__global__ __launch_bounds__(256) void fpn_wgrad_kernel(Src src, const float* __restrict__ dy, float* __restrict__ part, int H, int W, int OH, int OW,
                                                        int tiles_x, int tiles_per_view, int ntile) {
    typedef FpnWgradShape<COUT, CIN, K, ONES, S> F;
    constexpr int P = F::P, SH = F::SH, SW = F::SW;
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* ms = reinterpret_cast<float*>(lds4);                   // [CT][SH][RS]
    float* ds = ms + F::CT * F::PL;                               // [COUT][DSS]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    int off[F::NCBW];                                             // this lane's column (ci, ky, kx) in the staged tile, -1 past the end
#pragma unroll
    for (int t = 0; t < F::NCBW; ++t) {
        const int col = (wave + 4 * t) * 16 + li, ci = col / (K * K), tap = col % (K * K);
        off[t] = col < F::NCOL ? ci * F::PL + (tap / K) * F::RS + tap % K : -1;
    }
    f32x4 acc[F::NRB][F::NCBW];
#pragma unroll
    for (int rb = 0; rb < F::NRB; ++rb)
#pragma unroll
        for (int t = 0; t < F::NCBW; ++t) acc[rb][t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < ntile; tile += (int)gridDim.x) {
        const int n = tile / tiles_per_view, tv = tile % tiles_per_view;
        const int y0 = (tv / tiles_x) * F::TH, x0 = (tv % tiles_x) * F::TW;
        __syncthreads();                                          // the previous tile's readers are done
#pragma unroll 1
        for (int pos = tid; pos < SH * SW; pos += 256) {
            const int py = pos / SW, px = pos % SW, gy = y0 * S - P + py, gx = x0 * S - P + px;
            float* m = ms + py * F::RS + px;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            if (inside) {
                Src s = src;
                s.at(n, gy, gx);
#pragma unroll 1
                for (int c0 = 0; c0 < CIN; c0 += 8) {
                    float v[8];
                    s.load8(c0, v);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (CIN % 8 == 0 || c0 + k < CIN) m[(c0 + k) * F::PL] = v[k];
                }
            } else {
#pragma unroll 8
                for (int c = 0; c < CIN; ++c) m[c * F::PL] = 0.0f;
            }
            if (ONES) m[CIN * F::PL] = inside ? 1.0f : 0.0f;
        }
#pragma unroll 1
        for (int e = tid; e < COUT * F::NPIX; e += 256) {
            const int c = e / F::NPIX, pix = e % F::NPIX, gy = y0 + pix / F::TW, gx = x0 + pix % F::TW;
            ds[c * F::DSS + pix] = gy < OH && gx < OW ? dy[(((size_t)n * COUT + c) * OH + gy) * OW + gx] : 0.0f;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < F::NPIX / 4; ++q) {
            const int pix = 4 * q + g, at = (pix / F::TW) * S * F::RS + (pix % F::TW) * S;
            float a[F::NRB];
#pragma unroll
            for (int rb = 0; rb < F::NRB; ++rb) a[rb] = rb * 16 + li < COUT ? ds[(rb * 16 + li) * F::DSS + pix] : 0.0f;
#pragma unroll
            for (int t = 0; t < F::NCBW; ++t) {
                if (wave + 4 * t >= F::NCB) continue;             // wave-uniform
                const float b = off[t] >= 0 ? ms[off[t] + at] : 0.0f;
#pragma unroll
                for (int rb = 0; rb < F::NRB; ++rb) acc[rb][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], b, acc[rb][t], 0, 0, 0);
            }
        }
    }
    // lane (li, g) holds rows 16 rb + 4 g + r of column 16 cb + li
    float* dst = part + (size_t)blockIdx.x * COUT * F::NCOL;
#pragma unroll
    for (int t = 0; t < F::NCBW; ++t) {
        const int col = (wave + 4 * t) * 16 + li;
        if (col >= F::NCOL) continue;
#pragma unroll
        for (int rb = 0; rb < F::NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = rb * 16 + 4 * g + r;
                if (co < COUT) dst[co * F::NCOL + col] = acc[rb][t][r];
            }
    }
}

// H, W: the source's size; dY is (H - 1) / S + 1 by (W - 1) / S + 1
template <int COUT, int CIN, int K, bool ONES, int S = 1, class Src>
static int launch_fpn_wgrad(const Src& src, const float* dy, float* dw, float* part, int N, int H, int W, hipStream_t st) {
    typedef FpnWgradShape<COUT, CIN, K, ONES, S> F;
    const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;
    const int tiles_x = (int)ceil_div(OW, F::TW), tpv = tiles_x * (int)ceil_div(OH, F::TH), ntile = N * tpv;
    const int parts = fw_parts<COUT, CIN, K, ONES>(ntile);
    if (F::LDS > 48 * 1024)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fpn_wgrad_kernel<COUT, CIN, K, ONES, S, Src>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
    hipLaunchKernelGGL((fpn_wgrad_kernel<COUT, CIN, K, ONES, S, Src>), dim3(parts), dim3(256), F::LDS, st, src, dy, part, H, W, OH, OW, tiles_x, tpv, ntile);
    const int rc = check_launch("fpn_wgrad_kernel");
    return rc != MVS_OK ? rc : ft_reduce_partials(part, dw, parts, COUT * F::NCOL, st);
}

}  // namespace mvs
