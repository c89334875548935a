// The token weight gradient: ONE kernel body for dw[N, K] = sum_m dz[ymap(m), n] x[xmap(m), k] over token-major fp32 rows - the
// CrossBlock linears (vd_wgrad_kernel, vitdec_train_kernels.hip) and the head's window convolutions (vh_wgrad_kernel,
// vitdec_head_train_kernels.hip) are instances of it.
//
// The contraction index is the TOKEN, so an MFMA lane wants 8 consecutive tokens of one channel: the transpose of the forward's
// packed-split rows.  A workgroup (2 x 2 waves, wave = 64 x 64 of a 128 x 128 tile of dw) stages 32 tokens at a time: thread t reads
// channel t & 127 of tokens 8 o .. 8 o + 7 for the two octets o = 2 (t >> 7), 2 (t >> 7) + 1 (4-byte loads, a wave's lanes on 64
// consecutive channels of one token row), splits the eight values into hi + lo bf16 (split_format.h) and writes them as ONE 16-byte
// piece in the order the lanes read them,
//     lds[channel >> 4][hi|lo][lane = octet * 16 + (channel & 15)]           (conflict-free ds_write_b128 / ds_read_b128)
// Products are the three-term ones of the forward (mfma3_bf16), fp32 accumulate, tokens ascending.  The next 32 tokens' global loads
// are in flight during the MFMAs.  grid = (token slabs, K / 128, N / 128): every workgroup writes its partial tile and
// fmt_partial_reduce_kernel (partial_reduce.h) adds the slabs in slab order: no atomics, no arrival counters, bit-identical run to run.
// A launch of one slab writes the result directly.
//
// An instance differs from another in two things only:
//   Map   which row of dz and which row of x a token reads (TwMap<KIND>: identity, 3x3 shift on x, 4x4 stride-2 fine window on dz).
//         It holds the operands' base pointers and row strides; m.tile(n0, k0, c) once per thread moves the bases to c = its staged
//         channel of the tile; m.at(first) = the position of a run's first token, m.rows(pos, tok, yr, xr) = the two rows, m.next(pos)
//         counts the position on to the next token: no division per element.  The operand a window is on (Y_WINDOW / X_WINDOW) gets
//         row -1 = zero for a position outside the map.  Tokens past the slab and those zeros come from a branch, never from an
//         out-of-range load;
//   BIAS  whether the bias partial bpart[slab][n] = sum_m dz[m, n] is produced (by the workgroups of the first K tile, when bpart is
//         not null).
#pragma once
#include "mvs_common.h"
#include "partial_reduce.h"
#include "split_format.h"
#include "token_gemm.h"

namespace mvs {

constexpr int TW_T = 128;                     // dw tile: 128 output channels (n) x 128 input channels (k)
constexpr int TW_TOK = 32;                    // tokens per staged chunk = one MFMA k-step
constexpr int TW_TARGET = 512;                // workgroups wanted in a launch: two per compute unit
constexpr size_t TW_LDS = 2 * 8 * 128 * sizeof(bf16x8);

// slabs of whole 32-token chunks: enough for TW_TARGET workgroups over the launch's tiles, never more than there are chunks
static void token_wgrad_slabs(long long M, int N, int K, int& slabs, int& chunks_per_slab) {
    const int chunks = (int)ceil_div(M, TW_TOK), tiles = (N / TW_T) * (K / TW_T);
    int want = (int)ceil_div(TW_TARGET, tiles);
    if (want > chunks) want = chunks;
    chunks_per_slab = (int)ceil_div(chunks, want);
    slabs = (int)ceil_div(chunks, chunks_per_slab);
}

// ---- maps ----

// TW_IDENTITY: dz [M, N = Cy] and x [M, K = Cx] row by row (the linears).
// TW_CONV3 (proj): dw[co][tap * Cx + c] = sum_m dz[m][co] x[shift_tap(m)][c]; a K tile lies inside one tap (workgroup-uniform).
// TW_FINE4 (upsamplers): dw[tap * Cy + co][ci] = sum_m dz[fine_tap(m)][co] x[m][ci], dz = the fine map's rows [4 M, Cy]; the tap belongs
// to the staged channel (a wave stages 64 consecutive channels: one tap).
// The window maps walk the map [views, H, W] of the M tokens; every row index is below 2^24 (the entry points' ranges).
enum { TW_IDENTITY = 0, TW_CONV3 = 1, TW_FINE4 = 2 };

template <int KIND>
struct TwMap {
    static constexpr bool Y_WINDOW = KIND == TW_FINE4, X_WINDOW = KIND == TW_CONV3;
    const float* ysrc;           // the operands at the thread's staged channel (after tile()): dz rows of Cy channels, x rows of Cx
    const float* xsrc;
    int Cy, Cx, H, W, tap;
    struct Pos {
        int view, y, x;
    };
    __device__ __forceinline__ void tile(int n0, int k0, int c) {
        tap = KIND == TW_CONV3 ? k0 / Cx : (KIND == TW_FINE4 ? (n0 + c) / Cy : 0);
        ysrc += n0 + c - (KIND == TW_FINE4 ? tap * Cy : 0);
        xsrc += k0 + c - (KIND == TW_CONV3 ? tap * Cx : 0);
    }
    __device__ __forceinline__ Pos at(int first) const {
        Pos q{0, 0, 0};
        if (KIND != TW_IDENTITY) tg_pixel(first, H, W, q.view, q.y, q.x);
        return q;
    }
    __device__ __forceinline__ void rows(const Pos& q, int tok, int& yr, int& xr) const {
        int dy, dx;
        yr = xr = tok;
        if (KIND == TW_CONV3) {
            tg_conv3_offset(tap, dy, dx);
            const int sy = q.y + dy, sx = q.x + dx;
            xr = (sy < 0 || sy >= H || sx < 0 || sx >= W) ? -1 : tok + dy * W + dx;
        } else if (KIND == TW_FINE4) {
            tg_fine4_offset(tap, dy, dx);
            const int fy = 2 * q.y + dy, fx = 2 * q.x + dx;
            yr = (fy < 0 || fy >= 2 * H || fx < 0 || fx >= 2 * W) ? -1 : (q.view * 2 * H + fy) * 2 * W + fx;
        }
    }
    __device__ __forceinline__ void next(Pos& q) const {
        if (KIND != TW_IDENTITY && ++q.x == W) {
            q.x = 0;
            if (++q.y == H) {
                q.y = 0;
                ++q.view;
            }
        }
    }
};

// ---- the kernel body ----

template <bool BIAS, class Map>
__device__ __forceinline__ void token_wgrad(Map map, float* __restrict__ part, float* __restrict__ bpart, int M, int N, int K, int tok_per_slab) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    bf16x8* ly = reinterpret_cast<bf16x8*>(lds4);                 // [8 channel blocks][hi|lo][64 lanes]: dz
    bf16x8* lx = ly + 8 * 128;                                    // the same for x
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int wn = wave >> 1, wk = wave & 1;
    const int slab = (int)blockIdx.x, k0 = (int)blockIdx.y * TW_T, n0 = (int)blockIdx.z * TW_T;
    const int t0 = slab * tok_per_slab, t1 = t0 + tok_per_slab < M ? t0 + tok_per_slab : M;
    const int c = tid & 127, o0 = (tid >> 7) * 2;                 // staged channel of the tile, first of this thread's two token octets
    map.tile(n0, k0, c);
    float ry[16], rx[16];
    float bsum = 0.0f;

    auto fetch = [&](int t) {
        const int first = t + 8 * o0;                              // 16 consecutive tokens: the position once, then counted on
        typename Map::Pos pos = map.at(first);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tok = first + e;
            int yr, xr;
            map.rows(pos, tok, yr, xr);
            const bool ok = tok < t1;
            ry[e] = ok && (!Map::Y_WINDOW || yr >= 0) ? map.ysrc[(size_t)yr * map.Cy] : 0.0f;
            rx[e] = ok && (!Map::X_WINDOW || xr >= 0) ? map.xsrc[(size_t)xr * map.Cx] : 0.0f;
            map.next(pos);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    fetch(t0);
#pragma unroll 1
    for (int t = t0; t < t1; t += TW_TOK) {
        __syncthreads();                                           // the previous chunk has been read
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            float vy[8], vx[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                vy[e] = ry[8 * o + e];
                vx[e] = rx[8 * o + e];
                if (BIAS) bsum += vy[e];
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
        if (t + TW_TOK < t1) fetch(t + TW_TOK);                    // in flight during the MFMAs below
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
    float* dst = part + (size_t)slab * N * K;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* row = dst + (size_t)(n0 + wn * 64 + 16 * a + 4 * g + r) * K + k0 + wk * 64 + li;
#pragma unroll
            for (int b = 0; b < 4; ++b) row[16 * b] = acc[a][b][r];
        }
    // ---- bias partial: the workgroups of the first K tile; the two thread halves hold the two octet pairs of a chunk ----
    if (BIAS && bpart && blockIdx.y == 0) {
        float* red = reinterpret_cast<float*>(lds4);
        __syncthreads();
        if (tid >= 128) red[c] = bsum;
        __syncthreads();
        if (tid < 128) bpart[(size_t)slab * N + n0 + c] = bsum + red[c];
    }
}

// ---- the host side ----

// bytes of the partial tiles [slabs][N][K] and, with_bias, of the bias partials [slabs][N] behind them
static size_t token_wgrad_workspace_bytes(long long M, int N, int K, bool with_bias) {
    int slabs, per;
    token_wgrad_slabs(M, N, K, slabs, per);
    return (size_t)slabs * ((size_t)N * K + (with_bias ? N : 0)) * sizeof(float);
}

// launch(grid, part, bpart, tok_per_slab) starts the instance with TW_LDS bytes of dynamic LDS.  One slab: its "partial" is the result,
// written in place with no second launch; otherwise the partials are added in slab order.  dbias is nullable.
template <class Launch>
static int token_wgrad_run(const char* name, Launch launch, float* dw, float* dbias, void* workspace, long long M, int N, int K, hipStream_t st) {
    int slabs, per;
    token_wgrad_slabs(M, N, K, slabs, per);
    float* part = slabs == 1 ? dw : reinterpret_cast<float*>(workspace);
    float* bpart = !dbias ? nullptr : (slabs == 1 ? dbias : reinterpret_cast<float*>(workspace) + (size_t)slabs * N * K);
    launch(dim3(slabs, K / TW_T, N / TW_T), part, bpart, per * TW_TOK);
    int rc = check_launch(name);
    if (rc != MVS_OK || slabs == 1) return rc;
    rc = ft_reduce_partials(part, dw, slabs, N * K, st);
    if (rc != MVS_OK || !dbias) return rc;
    return ft_reduce_partials(bpart, dbias, slabs, N, st);
}

}  // namespace mvs
