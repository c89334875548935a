// The token GEMM: ONE kernel body for Y = sink(A W^T) over token-major rows - the CrossVITDecoder's linears, its head's window
// convolutions and the ViT backbone's linears (vd_gemm_kernel, vitdec_kernels.hip) and the forward and the data gradients of the
// head's training (vh_gemm_kernel, vitdec_head_train_kernels.hip) are instances of it.
//
// A is a packed-split tensor (vit_split.h), W is packing.pack_linear_bf16x3: [k >> 5][out >> 4][hi|lo][lane][k & 7]; every product is
// the three-term one (mfma3_bf16: lo*hi + hi*lo + hi*hi, fp32 accumulate), k ascending.  Workgroup = 2 x 2 waves, wave = 16 NREP tokens x
// 64 channels, tile 32 NREP x 128; K in chunks of 64 through LDS (both operands, staged with plain 16-byte copies in the order the
// lanes read them), the next chunk's global loads in flight during the MFMAs; blockIdx.z = class (of a transposed convolution).
//
// An instance differs from another in four things only:
//   NREP  1, 2 or 4 token blocks per wave (the launcher picks it from M);
//   Rows  where staged row m of the chunk at k0, class cls comes from (TgRows): r.row(m) ONCE per workgroup and staged row, r.chunk(k0,
//         cls) once per chunk (workgroup-uniform: the k-steps of a source row, the chunk's first k-step in it, the tap's window offset),
//         then r.source(row, chunk) = the source row, or -1 = zero.  Zero padding comes from that branch, never from an out-of-range
//         load, and a window never crosses into a neighbouring row or view.  The mode is a run-time argument; which modes an instance
//         HAS is compile-time: the forward has no FINE4, the head no ROWS, and neither pays for the other's;
//   Sum   TWO_LEVEL = false: one running sum.  true: a fresh accumulator per 64-k chunk, the chunk sums added in ascending order;
//   Sink  everything after the accumulators: s.row(row, cls) per output row, then s.store4(o, ch, acc) with the lane's four consecutive
//         output channels ch .. ch + 3.  A sink reads its pointers from the kernel's argument struct, as the kernels always did: what
//         the compiler knows about aliasing is what it knew (profiles/conv2d_unify_ab.json, earlier_forms, has the price of less).
// Args is the kernel's argument struct: a, w, w_class, M, K, N, Npad are read by the body, a_mode, C, H, W by TgRows, the rest by the Sink.
#pragma once
#include "mvs_common.h"
#include "split_format.h"
#include "vit_split.h"

namespace mvs {

constexpr int TG_KC = 64;                     // contraction per LDS chunk: two MFMA k-steps
constexpr int TG_TN = 128;                    // output channels per workgroup

// The CrossVITDecoder's head [module.py:316-321]: proj = Conv2d(768, 256, 3, padding 1), upsampler0 / 1 = ConvTranspose2d(256, 128 |
// 128, 64, 4, stride 2, padding 1).  taps = of the forward's window (3x3; the 2x2 of one parity class), dgrad_taps = of the data
// gradient's (3x3; the 4x4 stride-2 window of the fine map).
struct VitdecHeadLayer {
    int cin, cout, taps, dgrad_taps;
};
constexpr VitdecHeadLayer VITDEC_HEAD[3] = {{768, 256, 9, 9}, {256, 128, 4, 16}, {128, 64, 4, 16}};

// ---- windows ----

// (view, y, x) of row `row` of a map [views, H, W]
__device__ __forceinline__ void tg_pixel(int row, int H, int W, int& view, int& y, int& x) {
    const int hw = H * W;
    view = row / hw;
    const int pix = row - view * hw;
    y = pix / W;
    x = pix - y * W;
}

// window offset of tap `tap`: Conv2d(3, padding 1)
__device__ __forceinline__ void tg_conv3_offset(int tap, int& dy, int& dx) { dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1; }

// the 2x2 window of parity class cls = 2 py + px of ConvTranspose2d(4, stride 2, padding 1): output (2 y + py, 2 x + px) reads input
// (y + py - ay, x + px - ax) with ky = 1 - py + 2 ay, tap = 2 ay + ax
__device__ __forceinline__ void tg_deconv_offset(int tap, int cls, int& dy, int& dx) { dy = (cls >> 1) - (tap >> 1), dx = (cls & 1) - (tap & 1); }

// the 4x4 stride-2 window of the FINE map [2 H, 2 W]: coarse (y, x) reads fine (2 y + dy, 2 x + dx), tap = 4 ky + kx
__device__ __forceinline__ void tg_fine4_offset(int tap, int& dy, int& dx) { dy = (tap >> 2) - 1, dx = (tap & 3) - 1; }

// output row of a transposed convolution's class: row `row` of the coarse map [views, H, W] -> its view and its pixel of the fine map
__device__ __forceinline__ void tg_deconv_out(int row, int H, int W, int cls, int& view, int& opix) {
    int y, x;
    tg_pixel(row, H, W, view, y, x);
    opix = (2 * y + (cls >> 1)) * 2 * W + 2 * x + (cls & 1);
}

// index (in 16-byte units) of the fragment piece (k-step `kstep` of `steps`, hi|lo, lane group gl) of row srow of a packed-split tensor
__device__ __forceinline__ long long tg_piece(int srow, int steps, int kstep, int hl, int gl) {
    return ((((long long)(srow >> 4) * steps + kstep) * 2 + hl) * 64) + gl * 16 + (srow & 15);
}

// ---- rows ----

// a_mode: the row itself (the linears) | the 3x3 window | the 2x2 window of the class | the 4x4 stride-2 window of the fine map, of the
// map [views, H, W] of the M rows.  A staged row is `base` = first row of its view in the SOURCE map (ROWS: the row itself), -1 = past
// the end, and yx = (y << 16) | x of its pixel.  C = channels per tap.
enum { TG_A_ROWS = 0, TG_A_CONV3 = 1, TG_A_DECONV = 2, TG_A_FINE4 = 3 };

template <class Args, bool HAS_ROWS, bool HAS_FINE4>
struct TgRows {
    const Args& p;
    struct Row {
        int base, yx;
    };
    struct Chunk {
        int steps, kstep, dy, dx;
    };
    __device__ __forceinline__ bool in_place() const { return HAS_ROWS && p.a_mode == TG_A_ROWS; }
    __device__ __forceinline__ bool fine() const { return HAS_FINE4 && p.a_mode == TG_A_FINE4; }
    __device__ __forceinline__ Row row(int m) const {
        Row r{-1, 0};
        if (m >= p.M) return r;
        r.base = m;
        if (in_place()) return r;
        int view, y, x;
        tg_pixel(m, p.H, p.W, view, y, x);
        r.base = view * (p.H * p.W) * (fine() ? 4 : 1);
        r.yx = (y << 16) | x;
        return r;
    }
    __device__ __forceinline__ Chunk chunk(int k0, int cls) const {
        Chunk c{p.K >> 5, k0 >> 5, 0, 0};
        if (in_place()) return c;
        const int tap = k0 / p.C;
        c.steps = p.C >> 5;
        c.kstep = (k0 - tap * p.C) >> 5;
        if (p.a_mode == TG_A_CONV3) tg_conv3_offset(tap, c.dy, c.dx);
        else if (!fine()) tg_deconv_offset(tap, cls, c.dy, c.dx);
        else tg_fine4_offset(tap, c.dy, c.dx);
        return c;
    }
    __device__ __forceinline__ int source(const Row& r, const Chunk& c) const {
        if (r.base < 0 || in_place()) return r.base;
        int sy = (r.yx >> 16) + c.dy, sx = (r.yx & 0xffff) + c.dx, SH = p.H, SW = p.W;
        if (fine()) {                                                  // coarse (y, x) reads fine (2 y + dy, 2 x + dx) of [2 H, 2 W]
            sy += r.yx >> 16;
            sx += r.yx & 0xffff;
            SH *= 2;
            SW *= 2;
        }
        if (sy < 0 || sy >= SH || sx < 0 || sx >= SW) return -1;
        return r.base + sy * SW + sx;
    }
};

// ---- the kernel body ----

template <int NREP, bool TWO_LEVEL, class Args, class Rows, class Sink>
__device__ __forceinline__ void token_gemm(const Args& p, const Rows& rmap, const Sink& sink) {
    constexpr int NTB = 2 * NREP, TM = 16 * NTB;
    HIP_DYNAMIC_SHARED(float4, lds4)
    bf16x8* la = reinterpret_cast<bf16x8*>(lds4);                 // [NTB token blocks][2 steps][hi|lo][64 lanes]
    bf16x8* lw = la + NTB * 256;                                  // [2 steps][8 channel blocks][hi|lo][64 lanes]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = (int)blockIdx.x * TM, nb0 = (int)blockIdx.y * (TG_TN / 16), cls = (int)blockIdx.z;
    const bf16x8* wsrc = p.w + (size_t)cls * p.w_class;
    const int nmb = p.Npad >> 4;
    // staging: piece (token block i, tid) of the row operand; pieces tid + 256 i (i < 8) of the weight chunk
    const int ps = tid >> 7, phl = (tid >> 6) & 1, pgl = lane >> 4;
    bf16x8 ra[NTB], rw[8];
    bf16x8 zero;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero[e] = (__bf16)0.0f;

    typename Rows::Row rows[NTB];
#pragma unroll
    for (int i = 0; i < NTB; ++i) rows[i] = rmap.row(m0 + 16 * i + li);

    auto fetch = [&](int k0) {
        const typename Rows::Chunk ck = rmap.chunk(k0, cls);
#pragma unroll
        for (int i = 0; i < NTB; ++i) {
            const int srow = rmap.source(rows[i], ck);
            ra[i] = srow >= 0 ? p.a[tg_piece(srow, ck.steps, ck.kstep + ps, phl, pgl)] : zero;
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
    for (int k0 = 0; k0 < p.K; k0 += TG_KC) {
        __syncthreads();                                           // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < NTB; ++i) la[i * 256 + tid] = ra[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) lw[tid + 256 * i] = rw[i];
        __syncthreads();
        if (k0 + TG_KC < p.K) fetch(k0 + TG_KC);                   // in flight during the MFMAs below
        // two-level sum: the chunk's 64 k go into a fresh accumulator, k ascending, and the chunk sums into the total, chunks ascending.
        // The chunks are the same for every tile, so an element still does not depend on the tile that computes it; the rounding of
        // a long chain (K up to 6912) then happens at the magnitude of a chunk sum, not of the running total.
        f32x4 seg[4][NREP];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int nb = 0; nb < NREP; ++nb) seg[mb][nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        f32x4(&sum)[4][NREP] = TWO_LEVEL ? seg : acc;
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
                for (int nb = 0; nb < NREP; ++nb) sum[mb][nb] = mfma3_bf16(ah[mb], al[mb], bh[nb], bl[nb], sum[mb][nb]);
        }
        if (TWO_LEVEL) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int nb = 0; nb < NREP; ++nb) acc[mb][nb] += seg[mb][nb];
        }
    }

    // ---- epilogue: lane (li, g) holds channels 16 mb + 4 g .. + 3 of token li of block nb ----
#pragma unroll
    for (int nb = 0; nb < NREP; ++nb) {
        const int row = m0 + (wm * NREP + nb) * 16 + li;
        if (row >= p.M) continue;
        const typename Sink::Row o = sink.row(row, cls);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const int ch = (nb0 + wn * 4 + mb) * 16 + 4 * g;
            if (ch >= p.N) continue;
            sink.store4(o, ch, acc[mb][nb]);
        }
    }
}

// ---- the launcher ----

// k1, k2, k4 = the kernel's instances NREP = 1, 2, 4.  One instantiation per argument struct, i.e. per kernel: `raised` is the kernel's own.
template <class Args>
static int token_gemm_launch(const char* name, void (*k1)(Args), void (*k2)(Args), void (*k4)(Args), const Args& p, int classes,
                             hipStream_t st) {
    const int slot = p.M <= 32 ? 0 : (p.M <= 2048 ? 1 : 2), nrep = 1 << slot;
    void (*const kernel)(Args) = slot == 0 ? k1 : (slot == 1 ? k2 : k4);
    const size_t lds = (size_t)(2 * nrep * 256 + 2048) * 16;
    const dim3 grid(ceil_div(p.M, 32 * nrep), p.Npad / TG_TN, classes);
    // more than 48 KB of dynamic LDS needs the attribute, once per kernel and device
    static bool raised[3][64] = {};
    int dev = 0;
    hipGetDevice(&dev);
    if (lds > 48 * 1024 && !(dev >= 0 && dev < 64 && raised[slot][dev])) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (dev >= 0 && dev < 64) raised[slot][dev] = true;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, p);
    return check_launch(name);
}

}  // namespace mvs
