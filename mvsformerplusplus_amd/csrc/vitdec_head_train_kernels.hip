// Training of the CrossVITDecoder's head: proj = Conv2d(768, 256, 3, padding 1), upsampler0 / 1 =
// ConvTranspose2d(256, 128 | 128, 64, 4, stride 2, padding 1), each followed by batch-statistics BatchNorm2d and SiLU, forward and
// backward on token-major maps, fp32-equivalent.
//
// Reference (restated, never copied): models/module.py:316-321 and 357-363.
//
// Layout.  A map [NV, H, W] of C channels is its tokens one after the other, row = (view * H + y) * W + x: fp32 [M, C], and as a GEMM's
// row operand the packed-split tensor of vitdec_kernels.hip (vit_split.h).  A transposed convolution's output rows are in fine-map
// order, view * 4 H W + (2 y + py) * 2 W + 2 x + px.  Only the last layer's BatchNorm pass writes planar fp32 [NV, 64, 4 h, 4 w], and
// its backward reads the planar cotangent.
//
// Kernels:
//   1. vh_gemm_kernel<NREP>: vd_gemm_kernel's tile, staging and three-term products (2 x 2 waves, 32 NREP tokens x 128 channels, K in
//      chunks of 64 through LDS, the next chunk's loads in flight during the MFMAs) with an fp32 epilogue that honours the output row
//      mapping and no bias, and a two-level sum: every 64-k chunk is added up on its own and the chunk sums into the total, both
//      ascending, so the roundings of a chain of up to K = 6912 happen at the size of a chunk sum.  Row operand through a 3x3 window (proj forward; proj's data gradient on the flipped, channel-transposed
//      taps), through the 2x2 window of one parity class (upsampler forward, blockIdx.z = class) or through the 4x4 stride-2 window of
//      the FINE map (upsampler data gradient: coarse token (y, x) reads fine (2 y - 1 + ky, 2 x - 1 + kx)).
//   2. vh_wgrad_kernel<MODE>: vd_wgrad_kernel's 128 x 128 tile of dw over token slabs (transpose and split while staging, 32 tokens per
//      chunk, partial tiles added in slab order by fmt_partial_reduce_kernel) with a per-tap row mapping on one operand.  MODE 0 (proj):
//      dw[co][tap * 768 + c] = sum_m dz[m][co] x[shift_tap(m)][c]; a K tile lies inside one tap.  MODE 1 (upsamplers): dw[tap * Cout + co]
//      [ci] = sum_m dz[fine_tap(m)][co] x[m][ci]; the tap belongs to the staged channel (a wave stages 64 consecutive channels: one tap).
//   3. vh_bn_reduce_kernel / vh_bn_finalize_kernel / vh_bn_apply_kernel: batch-statistics BatchNorm + SiLU over [M, C] rows on
//      64-row x 64-channel tiles.  Column sums ([sum z | sum z^2], or [sum du | sum du xhat] in the backward) are accumulated in fp64 per
//      thread over the rows it walks, added over a workgroup's 16 row groups in group order, and the per-workgroup partials in a fixed
//      order by the finalize (16 segments front to back, then the segment sums; it also takes the running-statistics step, on the
//      device).  The apply writes SiLU(gamma xhat + beta) as fp32 rows and / or packed-split rows, or planar; backward: dz = gamma
//      invstd (du - sum du / M - xhat sum du xhat / M) as fp32 rows (the weight gradient's operand) and packed-split rows (the data
//      gradient's).  Planar tiles go through an LDS transpose so that both the token-major and the planar side are read and written
//      in whole lines.
// No atomics and no arrival counters: every result is the same bits from run to run and on any stream.  Rows past the end and window
// positions outside the map contribute zero from a branch, never from an out-of-range load; a window never crosses into a neighbouring
// row or view.
#include "mvs_common.h"
#include "partial_reduce.h"
#include "split_format.h"
#include "vit_split.h"

namespace mvs {

constexpr int VH_KC = 64;                     // contraction per LDS chunk: two MFMA k-steps
constexpr int VH_TN = 128;                    // output channels per workgroup
constexpr int VH_CIN[3] = {768, 256, 128}, VH_COUT[3] = {256, 128, 64};

enum { VH_A_CONV3 = 0, VH_A_DECONV = 1, VH_A_FINE4 = 2 };

// ---------------------------------------------------------------------------------------------------------------------------------
// window GEMM
// ---------------------------------------------------------------------------------------------------------------------------------
struct VhGemmArgs {
    const bf16x8* a;             // packed-split rows of the source map, C channels per row
    const bf16x8* w;             // pack_linear_bf16x3 [K / 32][Npad / 16][hi|lo][64]; class z at w + z * w_class
    float* out;                  // fp32 [rows of the output map, N]
    int M, K, N, Npad;
    int a_mode;
    int C, H, W;                 // channels per tap; the map of the M rows (FINE4: the source map is [2 H, 2 W])
    size_t w_class;
};

struct VhRow {
    int view, yx;                // view = -1: past the end; yx = (y << 16) | x
};

__device__ __forceinline__ VhRow vh_row(const VhGemmArgs& p, int row) {
    VhRow r{-1, 0};
    if (row >= p.M) return r;
    const int hw = p.H * p.W, view = row / hw, pix = row - view * hw, y = pix / p.W;
    r.view = view;
    r.yx = (y << 16) | (pix - y * p.W);
    return r;
}

// index (in 16-byte units) of the fragment piece (k-step, hi|lo, lane group gl) of the row that tap `tap` of class `cls` reads for the
// staged row r, or -1 = zero
__device__ __forceinline__ long long vh_a_piece(const VhGemmArgs& p, const VhRow& r, int tap, int cls, int steps, int kstep, int hl, int gl) {
    if (r.view < 0) return -1;
    const int y = r.yx >> 16, x = r.yx & 0xffff;
    int sy, sx, SH = p.H, SW = p.W;
    if (p.a_mode == VH_A_CONV3) {
        sy = y + tap / 3 - 1;
        sx = x + tap - (tap / 3) * 3 - 1;
    } else if (p.a_mode == VH_A_DECONV) {
        // output (2 y + py, 2 x + px) reads input (y + py - ay, x + px - ax) with ky = 1 - py + 2 ay
        sy = y + (cls >> 1) - (tap >> 1);
        sx = x + (cls & 1) - (tap & 1);
    } else {
        sy = 2 * y - 1 + (tap >> 2);
        sx = 2 * x - 1 + (tap & 3);
        SH = 2 * p.H;
        SW = 2 * p.W;
    }
    if (sy < 0 || sy >= SH || sx < 0 || sx >= SW) return -1;
    const int srow = (r.view * SH + sy) * SW + sx;
    return ((((long long)(srow >> 4) * steps + kstep) * 2 + hl) * 64) + gl * 16 + (srow & 15);
}

template <int NREP>
__global__ __launch_bounds__(256) void vh_gemm_kernel(VhGemmArgs p) {
    constexpr int NTB = 2 * NREP, TM = 16 * NTB;
    HIP_DYNAMIC_SHARED(float4, lds4)
    bf16x8* la = reinterpret_cast<bf16x8*>(lds4);                 // [NTB token blocks][2 steps][hi|lo][64 lanes]
    bf16x8* lw = la + NTB * 256;                                  // [2 steps][8 channel blocks][hi|lo][64 lanes]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = (int)blockIdx.x * TM, nb0 = (int)blockIdx.y * (VH_TN / 16), cls = (int)blockIdx.z;
    const bf16x8* wsrc = p.w + (size_t)cls * p.w_class;
    const int nmb = p.Npad >> 4, steps = p.C >> 5;
    // staging: piece (token block i, tid) of the row operand; pieces tid + 256 i (i < 8) of the weight chunk
    const int ps = tid >> 7, phl = (tid >> 6) & 1, pgl = lane >> 4;
    bf16x8 ra[NTB], rw[8];
    bf16x8 zero;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero[e] = (__bf16)0.0f;

    VhRow rows[NTB];
#pragma unroll
    for (int i = 0; i < NTB; ++i) rows[i] = vh_row(p, m0 + 16 * i + li);

    auto fetch = [&](int k0) {
        const int tap = k0 / p.C, kstep = ((k0 - tap * p.C) >> 5) + ps;            // the chunk's tap is workgroup-uniform
#pragma unroll
        for (int i = 0; i < NTB; ++i) {
            const long long idx = vh_a_piece(p, rows[i], tap, cls, steps, kstep, phl, pgl);
            ra[i] = idx >= 0 ? p.a[idx] : zero;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = tid + 256 * i, s = j >> 10, rest = j & 1023;
            rw[i] = wsrc[((size_t)((k0 >> 5) + s) * nmb + nb0) * 128 + rest];
        }
    };

    f32x4 acc[4][NREP];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < NREP; ++nb) acc[mb][nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    fetch(0);
#pragma unroll 1
    for (int k0 = 0; k0 < p.K; k0 += VH_KC) {
        __syncthreads();                                           // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < NTB; ++i) la[i * 256 + tid] = ra[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) lw[tid + 256 * i] = rw[i];
        __syncthreads();
        if (k0 + VH_KC < p.K) fetch(k0 + VH_KC);                   // in flight during the MFMAs below
        // two-level sum: the chunk's 64 k go into a fresh accumulator, k ascending, and the chunk sums into the total, chunks ascending.
        // The chunks are the same for every tile, so an element still does not depend on the tile that computes it; the rounding of
        // a long chain (K up to 6912) then happens at the magnitude of a chunk sum, not of the running total.
        f32x4 seg[4][NREP];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int nb = 0; nb < NREP; ++nb) seg[mb][nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 ah[4], al[4], bh[NREP], bl[NREP];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                ah[mb] = lw[((s * 8 + wn * 4 + mb) * 2 + 0) * 64 + lane];
                al[mb] = lw[((s * 8 + wn * 4 + mb) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int nb = 0; nb < NREP; ++nb) {
                bh[nb] = la[(((wm * NREP + nb) * 2 + s) * 2 + 0) * 64 + lane];
                bl[nb] = la[(((wm * NREP + nb) * 2 + s) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int nb = 0; nb < NREP; ++nb) seg[mb][nb] = mfma3_bf16(ah[mb], al[mb], bh[nb], bl[nb], seg[mb][nb]);
        }
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int nb = 0; nb < NREP; ++nb) acc[mb][nb] += seg[mb][nb];
    }

    // ---- epilogue: lane (li, g) holds channels 16 mb + 4 g .. + 3 of token li of block nb ----
#pragma unroll
    for (int nb = 0; nb < NREP; ++nb) {
        const int row = m0 + (wm * NREP + nb) * 16 + li;
        if (row >= p.M) continue;
        size_t orow = (size_t)row;
        if (p.a_mode == VH_A_DECONV) {
            const int hw = p.H * p.W, view = row / hw, pix = row - view * hw, y = pix / p.W, x = pix - y * p.W;
            orow = (size_t)view * 4 * hw + (size_t)(2 * y + (cls >> 1)) * 2 * p.W + 2 * x + (cls & 1);
        }
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const int ch = (nb0 + wn * 4 + mb) * 16 + 4 * g;
            if (ch >= p.N) continue;
            *reinterpret_cast<float4*>(p.out + orow * p.N + ch) = make_float4(acc[mb][nb][0], acc[mb][nb][1], acc[mb][nb][2], acc[mb][nb][3]);
        }
    }
}

static int vh_launch_gemm(const VhGemmArgs& p, int classes, hipStream_t st) {
    const int nrep = p.M <= 32 ? 1 : (p.M <= 2048 ? 2 : 4);
    const size_t lds = (size_t)(2 * nrep * 256 + 2048) * 16;
    const dim3 grid(ceil_div(p.M, 32 * nrep), p.Npad / VH_TN, classes);
    // more than 48 KB of dynamic LDS needs the attribute, once per kernel and device
    static bool raised[3][64] = {};
    int dev = 0;
    hipGetDevice(&dev);
#define MVS_VH_GO(NR, SLOT) \
    if (nrep == NR) { \
        if (lds > 48 * 1024 && !(dev >= 0 && dev < 64 && raised[SLOT][dev])) { \
            hipFuncSetAttribute(reinterpret_cast<const void*>(&vh_gemm_kernel<NR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (dev >= 0 && dev < 64) raised[SLOT][dev] = true; \
        } \
        hipLaunchKernelGGL((vh_gemm_kernel<NR>), grid, dim3(256), lds, st, p); \
    }
    MVS_VH_GO(1, 0) MVS_VH_GO(2, 1) MVS_VH_GO(4, 2)
#undef MVS_VH_GO
    return check_launch("vh_gemm_kernel");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// window weight gradient
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int VHW_T = 128;                    // dw tile: 128 x 128
constexpr int VHW_TOK = 32;                   // tokens per staged chunk = one MFMA k-step
constexpr int VHW_TARGET = 512;               // workgroups wanted in a launch: two per compute unit

// vd_wgrad_kernel's slab rule: slabs of whole 32-token chunks, enough for VHW_TARGET workgroups over the tiles, never more than chunks
static void vhw_slabs(long long M, int N, int K, int& slabs, int& chunks_per_slab) {
    const int chunks = (int)ceil_div(M, VHW_TOK), tiles = (N / VHW_T) * (K / VHW_T);
    int want = (int)ceil_div(VHW_TARGET, tiles);
    if (want > chunks) want = chunks;
    chunks_per_slab = (int)ceil_div(chunks, want);
    slabs = (int)ceil_div(chunks, chunks_per_slab);
}

struct VhWgradArgs {
    const float* dz;             // MODE 0: [M, N]; MODE 1: the fine map's rows [4 M, Cy]
    const float* x;              // MODE 0: [M, Cx]; MODE 1: [M, K]
    float* part;                 // [slabs][N][K]
    int M, N, K, Cy, Cx, H, W;   // the contraction runs over the M tokens of the map [NV, H, W]
    int tok_per_slab;
};

template <int MODE>
__global__ __launch_bounds__(256) void vh_wgrad_kernel(VhWgradArgs p) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    bf16x8* ly = reinterpret_cast<bf16x8*>(lds4);                 // [8 channel blocks][hi|lo][64 lanes]: dz
    bf16x8* lx = ly + 8 * 128;                                    // the same for x
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int wn = wave >> 1, wk = wave & 1;
    const int slab = (int)blockIdx.x, k0 = (int)blockIdx.y * VHW_T, n0 = (int)blockIdx.z * VHW_T;
    const int t0 = slab * p.tok_per_slab, t1 = t0 + p.tok_per_slab < p.M ? t0 + p.tok_per_slab : p.M;
    const int c = tid & 127, o0 = (tid >> 7) * 2;                 // staged channel of the tile, first of this thread's two token octets
    // the tap of the mapped operand: of the K tile (MODE 0, workgroup-uniform) or of the staged dz column (MODE 1, wave-uniform)
    const int tap = MODE == 0 ? k0 / p.Cx : (n0 + c) / p.Cy;
    const float* ysrc = MODE == 0 ? p.dz + n0 + c : p.dz + (n0 + c - tap * p.Cy);
    const float* xsrc = MODE == 0 ? p.x + (k0 - tap * p.Cx) + c : p.x + k0 + c;
    const int ystride = MODE == 0 ? p.N : p.Cy, xstride = MODE == 0 ? p.Cx : p.K;
    const int hw = p.H * p.W;
    float ry[16], rx[16];

    auto fetch = [&](int t) {
        const int first = t + 8 * o0;                              // 16 consecutive tokens: (view, y, x) once, then counted on
        int view = first / hw, pix = first - view * hw, y = pix / p.W, x = pix - y * p.W;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tok = first + e;
            long long yr = tok, xr = tok;
            if (MODE == 0) {
                const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1, sy = y + dy, sx = x + dx;
                xr = (sy < 0 || sy >= p.H || sx < 0 || sx >= p.W) ? -1 : (long long)tok + dy * p.W + dx;
            } else {
                const int fy = 2 * y - 1 + (tap >> 2), fx = 2 * x - 1 + (tap & 3);
                yr = (fy < 0 || fy >= 2 * p.H || fx < 0 || fx >= 2 * p.W) ? -1 : ((long long)view * 2 * p.H + fy) * 2 * p.W + fx;
            }
            const bool ok = tok < t1;
            ry[e] = ok && yr >= 0 ? ysrc[(size_t)yr * ystride] : 0.0f;
            rx[e] = ok && xr >= 0 ? xsrc[(size_t)xr * xstride] : 0.0f;
            if (++x == p.W) {
                x = 0;
                if (++y == p.H) {
                    y = 0;
                    ++view;
                }
            }
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    fetch(t0);
#pragma unroll 1
    for (int t = t0; t < t1; t += VHW_TOK) {
        __syncthreads();                                           // the previous chunk has been read
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            float vy[8], vx[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                vy[e] = ry[8 * o + e];
                vx[e] = rx[8 * o + e];
            }
            bf16x8 hi, lo;
            const int piece = (c >> 4) * 128 + (o0 + o) * 16 + (c & 15);
            split8(vy, hi, lo);
            ly[piece] = hi;
            ly[piece + 64] = lo;
            split8(vx, hi, lo);
            lx[piece] = hi;
            lx[piece + 64] = lo;
        }
        __syncthreads();
        if (t + VHW_TOK < t1) fetch(t + VHW_TOK);                  // in flight during the MFMAs below
        bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            ah[a] = ly[(wn * 4 + a) * 128 + lane];
            al[a] = ly[(wn * 4 + a) * 128 + 64 + lane];
            bh[a] = lx[(wk * 4 + a) * 128 + lane];
            bl[a] = lx[(wk * 4 + a) * 128 + 64 + lane];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = mfma3_bf16(ah[a], al[a], bh[b], bl[b], acc[a][b]);
    }

    // ---- partial tile: lane (li, g) holds dw[n = 16 a + 4 g + r][k = 16 b + li] ----
    float* dst = p.part + (size_t)slab * p.N * p.K;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* row = dst + (size_t)(n0 + wn * 64 + 16 * a + 4 * g + r) * p.K + k0 + wk * 64 + li;
#pragma unroll
            for (int b = 0; b < 4; ++b) row[16 * b] = acc[a][b][r];
        }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// token-major batch-statistics BatchNorm + SiLU
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int VB_T = 64;                      // tile: 64 rows x 64 channels
constexpr int VB_PITCH = 65;                  // of the transpose tile (floats)
constexpr int VB_MAX_PARTS = 256;             // partials per channel: the finalize adds them in 16 segments

__device__ __forceinline__ float vb_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }

// thread (rr = tid >> 4, q = tid & 15) holds rows row0 + rr + 16 i (i < 4), channels c0 + 4 q .. + 3; rows past M read as zero
__device__ __forceinline__ void vb_load_rows(const float* __restrict__ src, int C, int row0, int c0, int M, int tid, float (&v)[4][4]) {
    const int rr = tid >> 4, q = tid & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + rr + 16 * i;
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row < M) t = *reinterpret_cast<const float4*>(src + (size_t)row * C + c0 + 4 * q);
        v[i][0] = t.x; v[i][1] = t.y; v[i][2] = t.z; v[i][3] = t.w;
    }
}

// the same tile of a planar map [views, C, P]: lanes along the pixels, transposed through `tile` [64 channels][VB_PITCH]
__device__ __forceinline__ void vb_load_planar(const float* __restrict__ src, float* tile, int C, int P, int row0, int c0, int M, int tid,
                                               float (&v)[4][4]) {
    const int lane = tid & 63, w = tid >> 6, row = row0 + lane, rr = tid >> 4, q = tid & 15;
    __syncthreads();                                               // the tile's previous contents have been read
    if (row < M) {
        const int view = row / P, pix = row - view * P;
        const float* base = src + ((size_t)view * C + c0) * P + pix;
#pragma unroll
        for (int j = 0; j < 16; ++j) tile[(w + 4 * j) * VB_PITCH + lane] = base[(size_t)(w + 4 * j) * P];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[i][k] = row0 + rr + 16 * i < M ? tile[(4 * q + k) * VB_PITCH + rr + 16 * i] : 0.0f;
}

__device__ __forceinline__ void vb_store_planar(float* __restrict__ dst, float* tile, int C, int P, int row0, int c0, int M, int tid,
                                                const float (&v)[4][4]) {
    const int lane = tid & 63, w = tid >> 6, row = row0 + lane, rr = tid >> 4, q = tid & 15;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[(4 * q + k) * VB_PITCH + rr + 16 * i] = v[i][k];
    __syncthreads();
    if (row < M) {
        const int view = row / P, pix = row - view * P;
        float* base = dst + ((size_t)view * C + c0) * P + pix;
#pragma unroll
        for (int j = 0; j < 16; ++j) base[(size_t)(w + 4 * j) * P] = tile[(w + 4 * j) * VB_PITCH + lane];
    }
}

struct VbArgs {
    const float* z;              // [M, C] pre-activation (without the conv bias)
    const float* dy;             // backward: [M, C], or planar [M / P, C, P]
    const float* stats;          // [3][C] mean | biased variance | invstd
    const float* gamma;
    const float* beta;
    const double* sums;          // backward apply: [2][C] sum du | sum du xhat
    double* part;                // reduce: [parts][2][C]
    float* out;                  // apply: fp32 [M, C] (nullable), or planar
    bf16x8* out_packed;          // apply: packed-split rows (nullable)
    double count;
    int M, C, P, tiles_per_part;
};

// per-thread channel constants of the four channels c0 + 4 q ..
struct VbChan {
    float mean[4], invstd[4], g[4], b[4];
};

__device__ __forceinline__ VbChan vb_chan(const VbArgs& a, int c0, int tid) {
    VbChan k;
    const int ch = c0 + 4 * (tid & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k.mean[j] = a.stats[ch + j];
        k.invstd[j] = a.stats[2 * a.C + ch + j];
        k.g[j] = a.gamma[ch + j];
        k.b[j] = a.beta[ch + j];
    }
    return k;
}

// du = dy silu'(u)
__device__ __forceinline__ float vb_silu_bwd(float dy, float u) {
    const float s = vb_sigmoid(u);
    return dy * (s + u * s * (1.0f - s));
}

// MODE 0: [sum z | sum z^2]; MODE 1: [sum du | sum du xhat].  grid = (parts, C / 64).
template <int MODE, int PLANAR>
__global__ __launch_bounds__(256) void vh_bn_reduce_kernel(VbArgs a) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    double* sh = reinterpret_cast<double*>(lds4);                 // [16 row groups][16 quads][2][4]
    float* tile = reinterpret_cast<float*>(sh + 2048);            // [64][VB_PITCH]
    const int tid = (int)threadIdx.x, part = (int)blockIdx.x, c0 = (int)blockIdx.y * VB_T;
    const int ntiles = (a.M + VB_T - 1) / VB_T;
    const int first = part * a.tiles_per_part, last = first + a.tiles_per_part < ntiles ? first + a.tiles_per_part : ntiles;
    VbChan k{};
    if (MODE == 1) k = vb_chan(a, c0, tid);
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int tl = first; tl < last; ++tl) {
        const int row0 = tl * VB_T;
        float v[4][4], d[4][4];
        vb_load_rows(a.z, a.C, row0, c0, a.M, tid, v);
        if (MODE == 1) {
            if (PLANAR) vb_load_planar(a.dy, tile, a.C, a.P, row0, c0, a.M, tid, d);
            else vb_load_rows(a.dy, a.C, row0, c0, a.M, tid, d);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (MODE == 0) {
                    s0[j] += (double)v[i][j];
                    s1[j] += (double)v[i][j] * (double)v[i][j];
                } else {
                    const float xh = (v[i][j] - k.mean[j]) * k.invstd[j], u = xh * k.g[j] + k.b[j];
                    const float du = vb_silu_bwd(d[i][j], u);       // a row past the end has dy = 0: du = 0
                    s0[j] += (double)du;
                    s1[j] += (double)du * (double)xh;
                }
            }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sh[tid * 8 + j] = s0[j];
        sh[tid * 8 + 4 + j] = s1[j];
    }
    __syncthreads();
    if (tid < VB_T) {                                              // channel c0 + tid: the 16 row groups in group order
        double t0 = 0.0, t1 = 0.0;
        for (int rr = 0; rr < 16; ++rr) {
            t0 += sh[(rr * 16 + (tid >> 2)) * 8 + (tid & 3)];
            t1 += sh[(rr * 16 + (tid >> 2)) * 8 + 4 + (tid & 3)];
        }
        a.part[((size_t)part * 2 + 0) * a.C + c0 + tid] = t0;
        a.part[((size_t)part * 2 + 1) * a.C + c0 + tid] = t1;
    }
}

// MODE 0: stats from the sums; running_mean / running_var (nullable) take one momentum step with mean + conv_bias and the unbiased
// variance.  MODE 1: out0 = d_gamma | d_beta [2][C].  sums [2][C] keeps the totals for the backward's apply.
// grid = C / 16: thread (segment = tid >> 4, channel = 16 blockIdx.x + (tid & 15)) adds its segment of consecutive partials front to
// back, then the first 16 threads add the 16 segment sums front to back (the order of fmt_partial_reduce_kernel).
template <int MODE>
__global__ __launch_bounds__(256) void vh_bn_finalize_kernel(const double* __restrict__ part, double* __restrict__ sums, float* __restrict__ out0,
                                                             const float* __restrict__ conv_bias, float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, double count, float eps, float momentum, int C,
                                                             int parts) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    double* seg = reinterpret_cast<double*>(lds4);                // [2][16 segments][16 channels]
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x * 16 + (tid & 15), s = tid >> 4;
    const int per = (parts + 15) / 16, p0 = s * per, p1 = p0 + per < parts ? p0 + per : parts;
    double s0 = 0.0, s1 = 0.0;
    for (int p = p0; p < p1; ++p) {
        s0 += part[((size_t)p * 2 + 0) * C + c];
        s1 += part[((size_t)p * 2 + 1) * C + c];
    }
    seg[tid] = s0;
    seg[256 + tid] = s1;
    __syncthreads();
    if (tid >= 16) return;
    s0 = seg[tid];
    s1 = seg[256 + tid];
    for (int k = 1; k < 16; ++k) {
        s0 += seg[k * 16 + tid];
        s1 += seg[256 + k * 16 + tid];
    }
    sums[c] = s0;
    sums[C + c] = s1;
    if (MODE == 1) {
        out0[c] = (float)s1;
        out0[C + c] = (float)s0;
        return;
    }
    const double mean = s0 / count, m2 = s1 / count - mean * mean, var = m2 > 0.0 ? m2 : 0.0;
    out0[c] = (float)mean;
    out0[C + c] = (float)var;
    out0[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double m = (double)momentum, unbiased = var * (count / (count > 1.0 ? count - 1.0 : 1.0));
        running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * (mean + (conv_bias ? (double)conv_bias[c] : 0.0)));
        running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * unbiased);
    }
}

// MODE 0: SiLU(gamma xhat + beta); MODE 1: dz.  PLANAR: the forward writes planar / the backward reads the planar cotangent.
// grid = (row tiles, C / 64).
template <int MODE, int PLANAR>
__global__ __launch_bounds__(256) void vh_bn_apply_kernel(VbArgs a) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    float* tile = reinterpret_cast<float*>(lds4);                 // [64][VB_PITCH]
    const int tid = (int)threadIdx.x, row0 = (int)blockIdx.x * VB_T, c0 = (int)blockIdx.y * VB_T;
    const int rr = tid >> 4, ch = c0 + 4 * (tid & 15);
    const VbChan k = vb_chan(a, c0, tid);
    float k0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, k1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float v[4][4], d[4][4];
    vb_load_rows(a.z, a.C, row0, c0, a.M, tid, v);
    if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k0[j] = (float)(a.sums[ch + j] / a.count);
            k1[j] = (float)(a.sums[a.C + ch + j] / a.count);
        }
        if (PLANAR) vb_load_planar(a.dy, tile, a.C, a.P, row0, c0, a.M, tid, d);
        else vb_load_rows(a.dy, a.C, row0, c0, a.M, tid, d);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (v[i][j] - k.mean[j]) * k.invstd[j], u = xh * k.g[j] + k.b[j];
            if (MODE == 0) v[i][j] = u * vb_sigmoid(u);
            else v[i][j] = k.g[j] * k.invstd[j] * (vb_silu_bwd(d[i][j], u) - k0[j] - xh * k1[j]);
        }
    if (MODE == 0 && PLANAR) {
        vb_store_planar(a.out, tile, a.C, a.P, row0, c0, a.M, tid, v);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + rr + 16 * i;
        if (row >= a.M) continue;
        if (a.out) *reinterpret_cast<float4*>(a.out + (size_t)row * a.C + ch) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
        if (a.out_packed) vd_store_split4(a.out_packed, a.C >> 5, row, ch, v[i]);
    }
}

static bool vb_shape(long long M, int C) { return M >= 1 && M < (1LL << 24) && (C == 64 || C == 128 || C == 256); }

static void vb_parts(long long M, int& parts, int& tiles_per_part) {
    const int ntiles = (int)ceil_div(M, VB_T);
    tiles_per_part = (int)ceil_div(ntiles, VB_MAX_PARTS);
    parts = (int)ceil_div(ntiles, tiles_per_part);
}

constexpr size_t VB_REDUCE_LDS = 2048 * sizeof(double) + VB_T * VB_PITCH * sizeof(float);
constexpr size_t VB_APPLY_LDS = VB_T * VB_PITCH * sizeof(float);

}  // namespace mvs

using namespace mvs;

// ---- window GEMMs ---------------------------------------------------------------------------------------------------------------------
static bool vh_map(int layer, int NV, int H, int W) {
    // the finest map a layer touches has 4 NV H W rows (layers 1 / 2); rows are held in 24 bits
    return NV >= 1 && H >= 1 && W >= 1 && H <= 16383 && W <= 16383 && (long long)NV * H * W * (layer == 0 ? 1 : 4) < (1LL << 24);
}

static int vh_layer(const char* who, int layer) {
    if (layer >= 0 && layer <= 2) return MVS_OK;
    set_error("%s: built for layer 0 (proj 768 -> 256, 3x3), 1 (upsampler0 256 -> 128) and 2 (upsampler1 128 -> 64, both ConvTranspose2d 4x4 "
              "stride 2 padding 1) [module.py:316-321]; got layer %d", who, layer);
    return MVS_ERR_UNSUPPORTED;
}

extern "C" int mvs_vitdec_head_conv_fwd(const void* x_packed, const void* w_packed, float* z, int layer, int NV, int H, int W, void* stream) {
    int rc = vh_layer("mvs_vitdec_head_conv_fwd", layer);
    if (rc != MVS_OK) return rc;
    if (!x_packed || !w_packed || !z || !vh_map(layer, NV, H, W)) {
        set_error("mvs_vitdec_head_conv_fwd: bad arguments");
        return MVS_ERR_ARG;
    }
    VhGemmArgs p{};
    p.a = reinterpret_cast<const bf16x8*>(x_packed);
    p.w = reinterpret_cast<const bf16x8*>(w_packed);
    p.out = z;
    p.M = NV * H * W; p.K = (layer == 0 ? 9 : 4) * VH_CIN[layer]; p.N = VH_COUT[layer]; p.Npad = (p.N + VH_TN - 1) / VH_TN * VH_TN;
    p.a_mode = layer == 0 ? VH_A_CONV3 : VH_A_DECONV;
    p.C = VH_CIN[layer]; p.H = H; p.W = W;
    p.w_class = (size_t)(p.K / 32) * (p.Npad / 16) * 128;
    return vh_launch_gemm(p, layer == 0 ? 1 : 4, (hipStream_t)stream);
}

extern "C" int mvs_vitdec_head_dgrad(const void* dz_packed, const void* wt_packed, float* d_x, int layer, int NV, int H, int W, void* stream) {
    int rc = vh_layer("mvs_vitdec_head_dgrad", layer);
    if (rc != MVS_OK) return rc;
    if (!dz_packed || !wt_packed || !d_x || !vh_map(layer, NV, H, W)) {
        set_error("mvs_vitdec_head_dgrad: bad arguments");
        return MVS_ERR_ARG;
    }
    VhGemmArgs p{};
    p.a = reinterpret_cast<const bf16x8*>(dz_packed);
    p.w = reinterpret_cast<const bf16x8*>(wt_packed);
    p.out = d_x;
    p.M = NV * H * W; p.K = (layer == 0 ? 9 : 16) * VH_COUT[layer]; p.N = VH_CIN[layer]; p.Npad = p.N;
    p.a_mode = layer == 0 ? VH_A_CONV3 : VH_A_FINE4;
    p.C = VH_COUT[layer]; p.H = H; p.W = W;
    return vh_launch_gemm(p, 1, (hipStream_t)stream);
}

// ---- window weight gradients ----------------------------------------------------------------------------------------------------------
// dw as the kernel's [N, K]: layer 0 [256, 9 x 768], layers 1 / 2 [16 Cout, Cin]
static void vh_wgrad_dims(int layer, int& N, int& K) {
    N = layer == 0 ? VH_COUT[0] : 16 * VH_COUT[layer];
    K = layer == 0 ? 9 * VH_CIN[0] : VH_CIN[layer];
}

extern "C" size_t mvs_vitdec_head_wgrad_workspace_bytes(int layer, int NV, int H, int W) {
    if (layer < 0 || layer > 2 || !vh_map(layer, NV, H, W)) return 0;
    int N, K, slabs, per;
    vh_wgrad_dims(layer, N, K);
    vhw_slabs((long long)NV * H * W, N, K, slabs, per);
    return (size_t)slabs * N * K * sizeof(float);
}

extern "C" int mvs_vitdec_head_wgrad(const float* d_z, const float* x, float* dw, void* workspace, size_t workspace_bytes, int layer, int NV, int H,
                                     int W, void* stream) {
    int rc = vh_layer("mvs_vitdec_head_wgrad", layer);
    if (rc != MVS_OK) return rc;
    if (!d_z || !x || !dw || !workspace || !vh_map(layer, NV, H, W)) {
        set_error("mvs_vitdec_head_wgrad: bad arguments");
        return MVS_ERR_ARG;
    }
    if (workspace_bytes < mvs_vitdec_head_wgrad_workspace_bytes(layer, NV, H, W)) {
        set_error("mvs_vitdec_head_wgrad: workspace smaller than mvs_vitdec_head_wgrad_workspace_bytes");
        return MVS_ERR_ARG;
    }
    int N, K, slabs, per;
    vh_wgrad_dims(layer, N, K);
    const int M = NV * H * W;
    vhw_slabs(M, N, K, slabs, per);
    hipStream_t st = (hipStream_t)stream;
    // one slab: its "partial" is the result, written in place with no second launch
    VhWgradArgs p{d_z, x, slabs == 1 ? dw : reinterpret_cast<float*>(workspace), M, N, K, VH_COUT[layer], VH_CIN[layer], H, W, per * VHW_TOK};
    const dim3 grid(slabs, K / VHW_T, N / VHW_T);
    const size_t lds = 2 * 8 * 128 * sizeof(bf16x8);
    if (layer == 0) hipLaunchKernelGGL((vh_wgrad_kernel<0>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((vh_wgrad_kernel<1>), grid, dim3(256), lds, st, p);
    rc = check_launch("vh_wgrad_kernel");
    if (rc != MVS_OK || slabs == 1) return rc;
    return ft_reduce_partials(p.part, dw, slabs, N * K, st);
}

// ---- BatchNorm + SiLU -----------------------------------------------------------------------------------------------------------------
extern "C" size_t mvs_vitdec_head_bn_workspace_bytes(long long M, int channels) {
    if (!vb_shape(M, channels)) return 0;
    int parts, per;
    vb_parts(M, parts, per);
    return ((size_t)parts * 2 * channels + 2 * (size_t)channels) * sizeof(double);
}

static int vb_check(const char* who, long long M, int channels, int pixels_per_view, bool planar, const void* workspace, size_t workspace_bytes) {
    if (!vb_shape(M, channels)) {
        set_error("%s: built for token-major rows of 256, 128 or 64 channels (the BatchNorms of proj, upsampler0, upsampler1) and 1 <= M < 2^24 "
                  "[module.py:316-321]; got M = %lld, %d channels", who, M, channels);
        return MVS_ERR_UNSUPPORTED;
    }
    if (!workspace || workspace_bytes < mvs_vitdec_head_bn_workspace_bytes(M, channels) ||
        (planar && (pixels_per_view < 1 || M % pixels_per_view))) {
        set_error("%s: bad arguments (the workspace is mvs_vitdec_head_bn_workspace_bytes; a planar map has M = views x pixels_per_view rows)", who);
        return MVS_ERR_ARG;
    }
    return MVS_OK;
}

extern "C" int mvs_vitdec_head_bn_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                      float* running_mean, float* running_var, float* stats, float* y, void* y_packed, float* y_planar,
                                      void* workspace, size_t workspace_bytes, long long M, int channels, int pixels_per_view, void* stream) {
    int rc = vb_check("mvs_vitdec_head_bn_fwd", M, channels, pixels_per_view, y_planar != nullptr, workspace, workspace_bytes);
    if (rc != MVS_OK) return rc;
    if (!z || !gamma || !beta || !stats || !(eps > 0.0f) || (running_mean == nullptr) != (running_var == nullptr) ||
        (y_planar ? (y || y_packed) : (!y && !y_packed))) {
        set_error("mvs_vitdec_head_bn_fwd: bad arguments (the output is y and / or y_packed, or y_planar alone)");
        return MVS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int parts, per;
    vb_parts(M, parts, per);
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = part + (size_t)parts * 2 * channels;
    VbArgs a{};
    a.z = z; a.stats = stats; a.gamma = gamma; a.beta = beta; a.part = part;
    a.count = (double)M; a.M = (int)M; a.C = channels; a.P = y_planar ? pixels_per_view : 1; a.tiles_per_part = per;
    hipLaunchKernelGGL((vh_bn_reduce_kernel<0, 0>), dim3(parts, channels / VB_T), dim3(256), VB_REDUCE_LDS, st, a);
    rc = check_launch("vh_bn_reduce_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL((vh_bn_finalize_kernel<0>), dim3(channels / 16), dim3(256), 512 * sizeof(double), st, (const double*)part, sums, stats, conv_bias, running_mean, running_var,
                       a.count, eps, momentum, channels, parts);
    rc = check_launch("vh_bn_finalize_kernel");
    if (rc != MVS_OK) return rc;
    const dim3 grid(ceil_div(M, VB_T), channels / VB_T);
    if (y_planar) {
        a.out = y_planar;
        hipLaunchKernelGGL((vh_bn_apply_kernel<0, 1>), grid, dim3(256), VB_APPLY_LDS, st, a);
    } else {
        a.out = y;
        a.out_packed = reinterpret_cast<bf16x8*>(y_packed);
        hipLaunchKernelGGL((vh_bn_apply_kernel<0, 0>), grid, dim3(256), VB_APPLY_LDS, st, a);
    }
    return check_launch("vh_bn_apply_kernel");
}

extern "C" int mvs_vitdec_head_bn_bwd(const float* d_y, int d_y_planar, const float* z, const float* stats, const float* gamma, const float* beta,
                                      float* d_z, void* d_z_packed, float* d_gb, void* workspace, size_t workspace_bytes, long long M, int channels,
                                      int pixels_per_view, void* stream) {
    int rc = vb_check("mvs_vitdec_head_bn_bwd", M, channels, pixels_per_view, d_y_planar != 0, workspace, workspace_bytes);
    if (rc != MVS_OK) return rc;
    if (!d_y || !z || !stats || !gamma || !beta || !d_gb || (!d_z && !d_z_packed)) {
        set_error("mvs_vitdec_head_bn_bwd: bad arguments");
        return MVS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int parts, per;
    vb_parts(M, parts, per);
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = part + (size_t)parts * 2 * channels;
    VbArgs a{};
    a.z = z; a.dy = d_y; a.stats = stats; a.gamma = gamma; a.beta = beta; a.part = part; a.sums = sums;
    a.out = d_z; a.out_packed = reinterpret_cast<bf16x8*>(d_z_packed);
    a.count = (double)M; a.M = (int)M; a.C = channels; a.P = d_y_planar ? pixels_per_view : 1; a.tiles_per_part = per;
    const dim3 rgrid(parts, channels / VB_T), agrid(ceil_div(M, VB_T), channels / VB_T);
    if (d_y_planar) hipLaunchKernelGGL((vh_bn_reduce_kernel<1, 1>), rgrid, dim3(256), VB_REDUCE_LDS, st, a);
    else hipLaunchKernelGGL((vh_bn_reduce_kernel<1, 0>), rgrid, dim3(256), VB_REDUCE_LDS, st, a);
    rc = check_launch("vh_bn_reduce_kernel");
    if (rc != MVS_OK) return rc;
    hipLaunchKernelGGL((vh_bn_finalize_kernel<1>), dim3(channels / 16), dim3(256), 512 * sizeof(double), st, (const double*)part, sums, d_gb, (const float*)nullptr, (float*)nullptr,
                       (float*)nullptr, a.count, 0.0f, 0.0f, channels, parts);
    rc = check_launch("vh_bn_finalize_kernel");
    if (rc != MVS_OK) return rc;
    if (d_y_planar) hipLaunchKernelGGL((vh_bn_apply_kernel<1, 1>), agrid, dim3(256), VB_APPLY_LDS, st, a);
    else hipLaunchKernelGGL((vh_bn_apply_kernel<1, 0>), agrid, dim3(256), VB_APPLY_LDS, st, a);
    return check_launch("vh_bn_apply_kernel");
}
