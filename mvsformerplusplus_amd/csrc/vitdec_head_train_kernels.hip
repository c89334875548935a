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
//   1. vh_gemm_kernel<NREP>: the token GEMM of token_gemm.h with the two-level sum (every 64-k chunk is added up on its own and the
//      chunk sums into the total, both ascending, so the roundings of a chain of up to K = 6912 happen at the size of a chunk sum),
//      Rows through a 3x3 window (proj forward; proj's data gradient on the flipped, channel-transposed taps), through the 2x2 window
//      of one parity class (upsampler forward, blockIdx.z = class) or through the 4x4 stride-2 window of the FINE map (upsampler data
//      gradient: coarse token (y, x) reads fine (2 y - 1 + ky, 2 x - 1 + kx)), and a Sink that stores fp32 at the output row, no bias.
//   2. vh_wgrad_kernel<MODE>: the token weight gradient of token_wgrad.h with a window map on one operand and no bias partial.
//      MODE 0 (proj, TW_CONV3) shifts x; MODE 1 (upsamplers, TW_FINE4) reads dz through the fine window.
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
#include "split_format.h"
#include "token_gemm.h"
#include "token_wgrad.h"
#include "vit_split.h"

namespace mvs {

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

// Sink: fp32 rows of the output map, no bias
struct VhSink {
    const VhGemmArgs& p;
    typedef size_t Row;
    __device__ __forceinline__ Row row(int row, int cls) const {
        if (p.a_mode != TG_A_DECONV) return (size_t)row;
        int view, opix;
        tg_deconv_out(row, p.H, p.W, cls, view, opix);
        return (size_t)view * 4 * p.H * p.W + opix;
    }
    __device__ __forceinline__ void store4(const Row& orow, int ch, const f32x4& a) const {
        *reinterpret_cast<float4*>(p.out + orow * p.N + ch) = make_float4(a[0], a[1], a[2], a[3]);
    }
};

template <int NREP>
__global__ __launch_bounds__(256) void vh_gemm_kernel(VhGemmArgs p) {
    token_gemm<NREP, true>(p, TgRows<VhGemmArgs, false, true>{p}, VhSink{p});
}

static int vh_launch_gemm(const VhGemmArgs& p, int classes, hipStream_t st) {
    return token_gemm_launch("vh_gemm_kernel", vh_gemm_kernel<1>, vh_gemm_kernel<2>, vh_gemm_kernel<4>, p, classes, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// window weight gradient
// ---------------------------------------------------------------------------------------------------------------------------------
struct VhWgradArgs {
    const float* dz;             // MODE 0: [M, N]; MODE 1: the fine map's rows [4 M, Cy]
    const float* x;              // MODE 0: [M, Cx]; MODE 1: [M, K]
    float* part;                 // [slabs][N][K]
    int M, N, K, Cy, Cx, H, W;   // the contraction runs over the M tokens of the map [NV, H, W]
    int tok_per_slab;
};

// MODE 0: proj (3x3 shift on x); MODE 1: upsamplers (4x4 stride-2 fine window on dz)
template <int MODE>
__global__ __launch_bounds__(256) void vh_wgrad_kernel(VhWgradArgs p) {
    token_wgrad<false>(TwMap<MODE == 0 ? TW_CONV3 : TW_FINE4>{p.dz, p.x, p.Cy, p.Cx, p.H, p.W, 0}, p.part, nullptr, p.M, p.N, p.K, p.tok_per_slab);
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
    const VitdecHeadLayer& L = VITDEC_HEAD[layer];
    p.M = NV * H * W; p.K = L.taps * L.cin; p.N = L.cout; p.Npad = (p.N + TG_TN - 1) / TG_TN * TG_TN;
    p.a_mode = layer == 0 ? TG_A_CONV3 : TG_A_DECONV;
    p.C = L.cin; p.H = H; p.W = W;
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
    const VitdecHeadLayer& L = VITDEC_HEAD[layer];
    p.M = NV * H * W; p.K = L.dgrad_taps * L.cout; p.N = L.cin; p.Npad = p.N;
    p.a_mode = layer == 0 ? TG_A_CONV3 : TG_A_FINE4;
    p.C = L.cout; p.H = H; p.W = W;
    return vh_launch_gemm(p, 1, (hipStream_t)stream);
}

// ---- window weight gradients ----------------------------------------------------------------------------------------------------------
// dw as the kernel's [N, K]: layer 0 [256, 9 x 768], layers 1 / 2 [16 Cout, Cin]
static void vh_wgrad_dims(int layer, int& N, int& K) {
    const VitdecHeadLayer& L = VITDEC_HEAD[layer];
    N = layer == 0 ? L.cout : L.dgrad_taps * L.cout;
    K = layer == 0 ? L.taps * L.cin : L.cin;
}

extern "C" size_t mvs_vitdec_head_wgrad_workspace_bytes(int layer, int NV, int H, int W) {
    if (layer < 0 || layer > 2 || !vh_map(layer, NV, H, W)) return 0;
    int N, K;
    vh_wgrad_dims(layer, N, K);
    return token_wgrad_workspace_bytes((long long)NV * H * W, N, K, false);
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
    int N, K;
    vh_wgrad_dims(layer, N, K);
    const int M = NV * H * W;
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](dim3 grid, float* part, float*, int tok_per_slab) {
        VhWgradArgs p{d_z, x, part, M, N, K, VITDEC_HEAD[layer].cout, VITDEC_HEAD[layer].cin, H, W, tok_per_slab};
        if (layer == 0) hipLaunchKernelGGL((vh_wgrad_kernel<0>), grid, dim3(256), TW_LDS, st, p);
        else hipLaunchKernelGGL((vh_wgrad_kernel<1>), grid, dim3(256), TW_LDS, st, p);
    };
    return token_wgrad_run("vh_wgrad_kernel", launch, dw, nullptr, workspace, M, N, K, st);
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
