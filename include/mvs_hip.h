/* mvs_hip.h - C ABI of libmvs_hip.so: the MI355X (gfx950) implementation of MVSFormer++'s
 * depth-inference hot path (homography warp -> group-wise correlation cost volume ->
 * 3D-conv regularisation -> depth regression), SURVEY.md section 8.
 *
 * The reference (maybeLx/MVSFormerPlusPlus @ 2025-01-14) is pure Python/PyTorch and has no
 * FFI of its own; the seam a maintainer binds is the set of Python callables cited next to each
 * entry point below (file:line relative to the reference tree).  INTEGRATION.md shows the ctypes
 * stub and the `patch_model()` swap.  The feature side of the network has its own sections further
 * down: the FPN, FMT_with_pathway, the ViT feature decoder and the DINOv2 ViT-B/14 backbone
 * (`patch_fpn`, `patch_fmt`, `patch_vit_decoder`, `patch_vit`; `patch_all` composes the five swaps).
 *
 * Calling convention
 *   - every pointer is a DEVICE pointer unless its name ends in _host
 *   - tensors are dense row-major with the shape given in the comment; B = batch
 *   - `stream` is a hipStream_t passed as void*; work is only enqueued, never synchronised
 *   - return value: MVS_OK (0) or an MVS_ERR_* code; mvs_last_error() gives the message
 *   - no hidden global state, no allocation: scratch memory is passed in by the caller
 *     (mvs_*_workspace_bytes tells how much)
 *
 * Internal activation layout ("channel-last"): [B, D, H, W, C] fp32, C in {8,16,32,64}.
 */
#ifndef MVS_HIP_H
#define MVS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_ABI_VERSION 11

enum { MVS_OK = 0, MVS_ERR_ARG = 1, MVS_ERR_UNSUPPORTED = 2, MVS_ERR_LAUNCH = 3, MVS_ERR_WORKSPACE = 4 };
/* The return type of every function whose int is MVS_OK or an MVS_ERR_* code; predicates (*_is_built, *_is_tuned, mvs_gather_*) and
 * mvs_abi_version keep plain int.  This header is the only statement of the ABI: the Python binding reads its prototypes, these
 * constants and, from this typedef, which results to check (mvsformerplusplus_amd/_header.py), so it stays plain C in a closed type
 * vocabulary: int, float, double, size_t, long long, unsigned long long, pointers, const char* results.  The typedef names int: it
 * changes no symbol and no calling convention, MVS_ABI_VERSION stays 11 and the definitions keep writing int.                     */
typedef int mvs_status;
enum { MVS_DTYPE_F32 = 0, MVS_DTYPE_BF16 = 1, MVS_DTYPE_F16 = 2 };
/* feature-map layouts accepted by the two gather passes:
 *   MVS_LAYOUT_PLANAR       [B,V,C,H,W]          what the reference's FPN / FMT emit (models/module.py:257-270, models/FMT.py:195-197)
 *   MVS_LAYOUT_OCTET_TILED  [B,V,C/8,H,W,8]      the hand-off layout: the 8 channels of an octet are one
 *                                                contiguous 32-byte (fp32) / 16-byte (bf16, fp16) run; mvs_pack_features converts,
 *                                                a producer that writes it directly skips that pass              */
enum { MVS_LAYOUT_PLANAR = 0, MVS_LAYOUT_OCTET_TILED = 1 };
/* depth / confidence head modes, cost_volume.py:108-128 */
enum { MVS_HEAD_CE_EVAL = 0, MVS_HEAD_CE_TRAIN = 1, MVS_HEAD_REG = 2 };
/* regulariser kinds, cost_volume.py:41-49 */
enum { MVS_REG_COSTREGNET = 0, MVS_REG_COSTREGNET3D = 1 };
/* contraction precision of the MFMA convolutions:
 *   MVS_PREC_FP32    v_mfma_f32_16x16x4_f32, bit-exact fp32 fmaf chain (weights packed fp32)
 *   MVS_PREC_BF16X3  three-term split-bf16 product on v_mfma_f32_16x16x32_bf16 (hi*hi + hi*lo + lo*hi, fp32
 *                    accumulate, ~2^-16 relative product error; weights packed as hi/lo bf16)
 *   MVS_PREC_BF16P   mvs_tr_attention_fwd only: as BF16X3 (four-term scores, split v) but the softmax probabilities
 *                    enter p.v as one bf16 term (the reference's flash-attn path keeps q, k, v and p in bf16)
 *   MVS_PREC_BF16X3_SPLIT  the BF16X3 contraction with the activations IN HBM already split: every x_cl / skip_cl / y_cl / feat_cl /
 *                    volume_cl of the call is channel-last with, per voxel, C / 8 octets of [hi x8 | lo x8] bf16 (hi = bf16(x),
 *                    lo = bf16(x - hi); the same 4 bytes per element as fp32, element type still declared float).  The producing
 *                    epilogue splits once, the consumers' staging is a copy.  Logits stay planar fp32.  The inference U-Net runs in
 *                    this form (mvs_regnet_fwd / mvs_regnet_logits_fwd / mvs_conv3d_logits_fwd and the single layers accept it);
 *                    the training path and the fp32-contraction path keep fp32 activations.
 *   MVS_PREC_F16X2   fp16 ACTIVATIONS: every x_cl / skip_cl / y_cl / feat_cl / volume_cl of the call is channel-last _Float16 (declared
 *                    float*; 2 bytes per element), weights packed as fp16 hi + lo, two MFMA terms w_hi.x + w_lo.x on
 *                    v_mfma_f32_16x16x32_f16, fp32 accumulation, fp32 logits.  Final depth vs the fp32 oracle: 5.5e-5 relative L1 on plain
 *                    inputs, 4.2e-4 on the x30-logits stress set (bar 1e-3); the reference's own GPU path runs these layers under bf16
 *                    autocast (test.py:250).  Values beyond +-65504 overflow: the aggregate pass clamps the volume it writes.
 *   MVS_PREC_F16     as MVS_PREC_F16X2 with ONE fp16 term per weight (w_lo never read: half the MFMAs, half the weight bytes); the packed
 *                    weights are the MVS_PREC_F16X2 ones.  Depth error vs the fp32 oracle: 7e-5 plain / 4.8e-4 on the x30-logits stress set
 *                    (F16X2: 5.5e-5 / 4.2e-4; scripts/study_weight_precision.py).  mvs_conv3d_logits_fwd keeps both terms.
 *   MVS_PREC_F16MIX  one term on the layers with >= 32 channels on both sides or 64 on one (the U-Net's conv4 .. conv7), two on the others -
 *                    indistinguishable from MVS_PREC_F16X2 in the error study.  The format of the fine stages (ndepth <= model_th) under the
 *                    host mirror's default policy "stagemix" (round 5; its coarse stages run MVS_PREC_BF16X3_SPLIT), and of a bare regulariser.
 */
enum { MVS_PREC_FP32 = 0, MVS_PREC_BF16X3 = 1, MVS_PREC_BF16P = 2, MVS_PREC_BF16X3_SPLIT = 3, MVS_PREC_F16X2 = 4, MVS_PREC_ATTN16 = 5, MVS_PREC_F16 = 6, MVS_PREC_F16MIX = 7 };
/* format of the cost volume mvs_warp_corr_aggregate_fwd / mvs_volume_normalise leave behind: fp32 [B,D,H,W,8], the split activation
 * format of MVS_PREC_BF16X3_SPLIT, or fp16 [B,D,H,W,8] for MVS_PREC_F16X2 (aggregate only; normalised volumes of 8 groups only;
 * partial sums are always fp32) */
enum { MVS_VOLUME_F32 = 0, MVS_VOLUME_SPLIT = 1, MVS_VOLUME_F16 = 2 };
/* how the LDS-staged gather holds the SOURCE-view window: fp32 (exact; the fp32-equivalent formats), or one fp16 octet per position -
 * half the LDS reads; the source features are rounded to fp16 once (exact for fp16 / in-range bf16 features), everything else stays fp32.
 * MVS_VOLUME_F16 (aggregate) and mvs_warp_corr_entropy_keep_fwd imply MVS_GATHER_F16; kernels outside the LDS-staged form ignore it.
 * The reference rounds the features to a 16-bit type under its autocast (test.py:250, cost_volume.py:67).                              */
enum { MVS_GATHER_F32 = 0, MVS_GATHER_F16 = 1 };
/* format of the per-view group correlations mvs_warp_corr_entropy_keep_fwd keeps for mvs_corr_aggregate_fwd ([B,V-1,D,H,W,8]):
 * MVS_CORR_F16 = fp16 octets from fp16 source windows (16 B per voxel and view; the fp16 formats' fine stages), MVS_CORR_F32 = fp32 octets
 * from fp32 windows (32 B; EXACT: the streamed pass 2 then equals the second gather - the coarse stages of the default policy, whose
 * depth schedules the next stage's hypotheses: the fp16 correlations' 2^-11 is what an ill-conditioned cascade amplifies).               */
enum { MVS_CORR_F16 = 0, MVS_CORR_F32 = 1 };
/* epilogues of mvs_tr_linear_fwd */
enum { MVS_TR_EPI_BIAS = 0, MVS_TR_EPI_GELU = 1, MVS_TR_EPI_RES_LN = 2 };

int mvs_abi_version(void);

/* fp16 activation format (MVS_PREC_F16X2): every store of an activation tensor clamps to +-65504.  A clamp that really fired means the
 * default format degraded a value the fp32-equivalent format (MVS_PREC_BF16X3) would have kept.  Returns the number of work-items, summed
 * over all launches on the CURRENT device since the last reset, that stored at least one value beyond the fp16 range (cost volume writes
 * of mvs_warp_corr_aggregate_fwd / mvs_volume_to_f16, every convolution / transposed-convolution epilogue); reset != 0 clears it.
 * Synchronises the device (a device-to-host copy of three counters): call it between batches, not per launch.                        */
unsigned long long mvs_f16_saturation_count(int reset);
const char* mvs_last_error(void);

/* ---- a1 + warping.py:80-82 ---------------------------------------------------------------------
 * proj [B,V,2,4,4] (0 = extrinsic, 1 = intrinsic; datasets/general_eval.py:211-216).
 * For every source view v>=1: P = E.clone(); P[:3,:4] = K[:3,:3] @ E[:3,:4] (cost_volume.py:68-71),
 * M = P_v @ inverse(P_0); homography[b, v-1] = {M[:3,:3] row-major (9), M[:3,3] (3)}.          */
mvs_status mvs_compose_homography(const float* proj, int B, int V, float* homography /*[B,V-1,12]*/, void* stream);
/* Round 5, cascade prologue (DINOv2_mvsformer_model.py:127-150): the homographies of ALL stages (n_stages <= 8 proj tensors [B,V,2,4,4],
 * host array of device pointers) -> homography [n_stages,B,V-1,12], and - hyp != NULL - stage 1's hypotheses (mvs_init_range_fwd:
 * depth_values [B,N] -> hyp [B,D,H,W]) in ONE launch instead of n_stages + 1.                                                */
mvs_status mvs_cascade_prologue_fwd(const float* const* proj_host_ptrs, int n_stages, int B, int V, float* homography,
                                    const float* depth_values, int N, int inverse, float* hyp, int D, int H, int W, void* stream);
/* same from already-composed 4x4 projections (the argument form of homo_warping_3D_with_mask) */
mvs_status mvs_homography_from_proj(const float* src_proj /*[B,4,4]*/, const float* ref_proj /*[B,4,4]*/, int B,
                                    float* homography /*[B,12]*/, void* stream);

/* ---- a2/a3: models/warping.py:69-109 homo_warping_3D_with_mask ---------------------------------
 * src_fea [B,C,H,W] (dtype), depth [B,D] (depth_is_volume=0) or [B,D,H,W] (1)
 * -> warped [B,C,D,H,W] fp32, proj_mask [B,D,H,W] uint8 (either may be NULL).                   */
mvs_status mvs_homo_warp_fwd(const void* src_fea, int dtype, const float* homography /*[B,12]*/, const float* depth,
                             int depth_is_volume, float* warped, uint8_t* proj_mask, int B, int C, int D, int H, int W,
                             void* stream);

/* ---- a2-a5 fused: warp + group-wise correlation + softmax-entropy, cost_volume.py:65-92 --------
 * features [B,V,C,H,W] (dtype; view 0 = reference), hyp [B,D,H,W]
 * -> entropy [B,V-1,H,W].  No [C,D,H,W] or [G,D,H,W] intermediate is materialised.
 * Only source views in [view_begin, view_end) (1-based view indices) are processed.
 * gather_format: MVS_GATHER_F32 / MVS_GATHER_F16 (above).                                        */
mvs_status mvs_warp_corr_entropy_fwd(const void* features, int dtype, int layout, const float* homography /*[B,V-1,12]*/,
                                     const float* hyp, float* entropy, int B, int V, int C, int G, int D, int H, int W,
                                     int view_begin, int view_end, int gather_format, void* stream);

/* ---- pass 1 that KEEPS the per-view group correlations + the streaming pass 2 ------------------------------------------------
 * cost_volume.py:74-101 with the [B,G,D,H,W] per-view correlation the reference materialises kept as [B,V-1,D,H,W,8] in `corr_format`
 * (MVS_CORR_F16: clamped to the fp16 range, mvs_f16_saturation_count; MVS_CORR_F32: exact) instead of warping twice.
 * mvs_warp_corr_entropy_keep_fwd = the entropy pass over ALL source views + `corr`; mvs_corr_aggregate_fwd =
 * sum_v vis_v * corr_v / (sum_v vis_v + 1e-6) -> the normalised volume [B,D,H,W,8] in `volume_format` (MVS_VOLUME_F16 / _SPLIT / _F32:
 * the regulariser's format is independent of the gather's).  Built where mvs_gather_keeps_correlations() returns 1 (the LDS-staged
 * gather's shapes; MVS_CORR_F32 additionally needs D > 4); MVS_ERR_UNSUPPORTED elsewhere - the two-gather pair above covers every
 * shape.  Whether the stream pays (16 / 32 B per voxel and view written and read against a second gather) is the caller's policy.   */
int mvs_gather_keeps_correlations(int layout, int C, int G, int D, int H, int W);
mvs_status mvs_warp_corr_entropy_keep_fwd(const void* features, int dtype, int layout, const float* homography /*[B,V-1,12]*/,
                                          const float* hyp, float* entropy, void* corr, int corr_format, int B, int V, int C, int G, int D,
                                          int H, int W, void* stream);
mvs_status mvs_corr_aggregate_fwd(const void* corr, int corr_format, const float* vis /*[B,V-1,H,W]*/, void* volume_cl, int volume_format,
                                  int B, int V, int D, int H, int W, void* stream);

/* ---- section 8f #4, producer side (round 5): the feature side's LAST 3x3 convolution emitting the hand-off layout ----------------
 * Replaces Conv2d(Cin, Cout, 3, padding=1[, bias]) [+ folded BatchNorm2d] [+ Swish] followed by torch.stack / mvs_pack_features:
 * models/FMT.py:195-197 (smooth_1/2/3: (32,32), (16,16), (8,8), no bias, act 0) and models/module.py:257-270 (FPNDecoder.out1/2/3:
 * (64,32), (64,16), (64,8), bias = folded BatchNorm shift, act 1 = Swish).  x [N,Cin,H,W] planar (in_dtype), image n at
 * x + n * in_batch_stride elements; w_packed = packing.pack_conv_weights_bf16x3(w[:, :, None], min(Cin, 32)) (split-bf16, three MFMA
 * terms: fp32-equivalent); bias [Cout] fp32 or NULL; tiled [.., Cout/8, H, W, 8] (out_dtype), image n at tiled + n * out_batch_stride
 * elements (so that view v of [B,V,C/8,H,W,8] can be written in place: out_batch_stride = V * Cout * H * W).  mvs_feature_conv_is_built
 * says which (Cin, Cout) pairs exist; others return MVS_ERR_UNSUPPORTED.                                                          */
int mvs_feature_conv_is_built(int Cin, int Cout);
mvs_status mvs_conv2d3x3_tiles_fwd(const void* x, int in_dtype, const void* w_packed, const float* bias, int act, void* tiled, int out_dtype,
                                   int N, int Cin, int Cout, int H, int W, long long in_batch_stride, long long out_batch_stride,
                                   void* stream);

/* ---- section 8f #4: feature hand-off -------------------------------------------------------------------
 * features [N,C,H,W] (dtype) -> tiled [N,C/8,H,W,8] (out_dtype); C % 8 == 0.  fp32 / bf16 / fp16 in, any of them out except
 * bf16 <-> fp16.  The cast to a 2-byte type rounds to nearest even, like the .to(bfloat16) the reference's autocast applies. */
mvs_status mvs_pack_features(const void* features, int dtype, void* tiled, int out_dtype, int N, int C, int H, int W, void* stream);

/* ---- a5: visibility CNN, cost_volume.py:36,93 + module.py:168-197 ------------------------------
 * entropy [N,H,W] -> vis [N,H,W] = sigmoid(conv1x1(CBR(16->8)(CBR(16->16)(CBR(1->16)(entropy))))).
 * Packed parameters are produced by the Python side (mvsformerplusplus_amd/packing.py):
 *   w1 [9][16] + b1[16] (BN folded), w2/w3 = MFMA-packed 3x3 weights (layout below), b2[16], b3[8]
 *   (padded to 16), w4[8], b4[1].  workspace >= mvs_vis_workspace_bytes(N,H,W).                  */
size_t mvs_vis_workspace_bytes(int N, int H, int W, int precision);
mvs_status mvs_vis_weight_fwd(const float* entropy, const float* w1, const float* b1, const void* w2, const float* b2,
                              const void* w3, const float* b3, const float* w4, const float* b4, float* vis,
                              void* workspace, size_t workspace_bytes, int N, int H, int W, int precision, void* stream);

/* the first (1->16 3x3 + BN + ReLU -> [N,H,W,16] channel-last) and last (8->1 1x1 + sigmoid) layer of the chain above
 * on their own; the two middle layers are mvs_conv3d_bn_relu_fwd with kd = 1 */
mvs_status mvs_vis_conv1_fwd(const float* entropy, const float* w1, const float* b1, float* out_cl16, int N, int H, int W, void* stream);
mvs_status mvs_vis_out_fwd(const float* x_cl8, const float* w4, const float* b4, float* vis, int N, int H, int W, void* stream);

/* ---- a4 + a6: recompute warp + correlation, weight by visibility, aggregate over views ----------
 * cost_volume.py:79-101.  vis [B,V-1,H,W].  volume_cl [B,D,H,W,G] channel-last.
 *   normalise = 1 : volume = sum_v ip_v*vis_v / (sum_v vis_v + 1e-6)              (single GPU)
 *   normalise = 0 : volume = partial sum over [view_begin, view_end), vis_sum [B,H,W] = partial
 *                   sum of vis (view-sharded multi-GPU: all-reduce both, then mvs_volume_normalise) */
mvs_status mvs_warp_corr_aggregate_fwd(const void* features, int dtype, int layout, const float* homography, const float* hyp,
                                       const float* vis, float* volume_cl, float* vis_sum, int normalise, int volume_format, int B,
                                       int V, int C, int G, int D, int H, int W, int view_begin, int view_end, void* stream);
/* ---- slab exchange of the view-sharded latency mode (no reference counterpart - the reference is
 * single-GPU; the sums follow cost_volume.py:97-101).  Message j = rows [row_begin[j], row_end[j]) of a PARTIAL fp32 volume
 * [B,D,H,W,G] followed by the same rows of the partial visibility sum [B,H,W], i.e. B*D*rows*W*G + B*rows*W floats (G: v10).
 * mvs_slab_pack: one launch writes the messages of all n_ranks destinations (send_host_ptrs[j] = device buffer, NULL = no message).
 * mvs_slab_reduce: slab_out = sum over ranks j = 0 .. n_ranks-1, in that order, of rank j's partial of MY rows [row_begin, row_end):
 * the own slice (j == my_rank) read in place from (volume_cl, vis_sum), the others from recv_host_ptrs[j] (NULL = rank j sent
 * nothing).  The pointer arrays are HOST arrays of device pointers (at most 16 ranks).                                           */
mvs_status mvs_slab_pack(const float* volume_cl, const float* vis_sum, float* const* send_host_ptrs, const int* row_begin, const int* row_end,
                         int n_ranks, int B, int D, int H, int W, int G, void* stream);
mvs_status mvs_slab_reduce(const float* volume_cl, const float* vis_sum, float* const* recv_host_ptrs, int n_ranks, int my_rank, float* slab_out,
                           int row_begin, int row_end, int B, int D, int H, int W, int G, void* stream);
/* volume_cl /= (vis_sum + 1e-6) in place; volume_format = MVS_VOLUME_SPLIT additionally converts it to the split format */
mvs_status mvs_volume_normalise(float* volume_cl, const float* vis_sum, int B, int D, int H, int W, int G, int volume_format, void* stream);
/* fp32 volume [B,D,H,W,8] (vis_sum != NULL: divided by vis_sum + 1e-6 first) -> fp16 [B,D,H,W,8] in a separate buffer, clamped to the
 * fp16 range: the cost volume of the MVS_PREC_F16X2 U-Net where the aggregate pass could not write it directly (view-sharded
 * multi-GPU partial sums; shapes outside the LDS-staged gather)                                                                */
/* 1 when the two gather passes take the LDS-staged kernels for this shape (the only ones that write MVS_VOLUME_SPLIT / _F16 directly) */
int mvs_gather_is_lds_staged(int layout, int C, int G, int D, int H, int W);
mvs_status mvs_volume_to_f16(const float* volume_cl, const float* vis_sum, void* out_f16, int B, int D, int H, int W, int G, void* stream);

/* ---- section 8f #2 (first slice): backward of mvs_warp_corr_aggregate_fwd(normalise = 1) ----------------------------
 * The gradient the reference's autograd produces for cost_volume.py:74-101: the sampling grid is built under torch.no_grad()
 * (warping.py:80) and the entropy from sim.detach() (cost_volume.py:90), so gradients reach the features and the visibility
 * maps only.  features planar [B,V,C,H,W] (fp32 / bf16 / fp16), volume_cl = the forward's output, vis_sum [B,H,W] = sum_v vis_v,
 * grad_volume_cl [B,D,H,W,G]; outputs: grad_features [B,V,C,H,W] fp32 (zeroed here, source views accumulated with atomics),
 * grad_vis [B,V-1,H,W].  Any C, G with C % G == 0.                                                                          */
mvs_status mvs_warp_corr_aggregate_bwd(const void* features, int dtype, const float* homography, const float* hyp, const float* vis,
                                       const float* vis_sum, const float* volume_cl, const float* grad_volume_cl,
                                       float* grad_features, float* grad_vis, int B, int V, int C, int G, int D, int H, int W,
                                       void* stream);

/* ---- a7: Conv3d + folded BatchNorm3d + ReLU, module.py:89-126 ----------------------------------
 * x_cl [B,D,H,W,Cin] -> y_cl [B,OD,OH,OW,Cout]; kernel (kd,3,3), kd in {1,3}, padding (kd/2,1,1),
 * stride (sd,sh,sw) in {1,2}.  Implicit GEMM on MFMA; `precision` = MVS_PREC_* selects the contraction and the
 * packed-weight format (packing.pack_conv_weights / pack_conv_weights_bf16x3, DESIGN.md "MFMA weight packing");
 * bias [max(Cout,16)] fp32.                                                                                */
mvs_status mvs_conv3d_bn_relu_fwd(const float* x_cl, const void* w_packed, const float* bias, float* y_cl, int B, int Cin,
                                  int Cout, int D, int H, int W, int kd, int sd, int sh, int sw, int relu, int precision,
                                  void* stream);

/* ---- a10: CostRegNet's 3x3x3 `prob` head (Conv3d(8, 1, 3, padding 1, bias=False), module.py:391,407) on the MFMA path:
 * x_cl [B,D,H,W,8] -> logits [B,D,H,W] planar.  w_packed = the [1,8,3,3,3] weight zero-padded to 16 output rows and packed like
 * a Conv3d(8,16) (packing.pack_conv_weights_bf16x3); bias [16] (zeros for the reference's bias-free layer).  MVS_PREC_BF16X3 only;
 * the exact-fp32 form of the same head is mvs_prob_regress_fwd(prob_ksize = 3).                                               */
mvs_status mvs_conv3d_logits_fwd(const float* x_cl, const void* w_packed, const float* bias, float* logits, int B, int D, int H,
                                 int W, int precision, void* stream);

/* ---- section 8f #2: training-mode regulariser (batch-statistics BatchNorm, weight gradients) -------------------------------
 * Channel-last fp32 [N voxels][C], C in {8,16,32,64}; `groups` independent statistics sets of N voxels each (tensor [groups][N][C],
 * statistics [groups][...]; the visibility CNN normalises each source view's batch on its own).  The forward convolutions and the DATA gradients of the training path are
 * mvs_conv3d_bn_relu_fwd (relu = 0, zero bias) / mvs_deconv3d_linear_fwd with un-folded, re-packed weights (training.py).
 *   mvs_bn_stats       sums[2C] (double) = per-channel [sum x | sum x^2]                       nn.BatchNorm3d, training=True
 *   mvs_bn_finalize    mean / biased var / 1/sqrt(var+eps) from sums and the voxel count (after an optional SyncBN all-reduce);
 *                      running_mean / running_var != NULL: nn.BatchNorm's momentum step (unbiased variance) in the same launch;
 *                      mvs_bn_running_update repeats that step alone
 *   mvs_bn_relu_apply  y = relu((z-mean)*invstd*gamma+beta) [+ skip]                            module.py:120-125, 402-405
 *   mvs_bn_relu_bwd    phase 0: sums[2C] = [d beta | d gamma] of dy through the ReLU mask; phase 1: dz (count = voxels of all
 *                      ranks, use_batch_stats = 0 for eval-mode BatchNorm inside a training graph)
 *   mvs_conv3d_wgrad   dW[CB][CA][kd*9] of Conv3d(k (kd,3,3), kd = 1 | 3, 'same' padding, stride) from input a_cl [B,D,H,W,CA] and output gradient
 *                      g_cl [B,OD,OH,OW,CB] on the fp32 MFMA path; a transposed convolution's weight gradient is the same call
 *                      with a = its output gradient and g = its input (result in ConvTranspose3d's [Cin][Cout][27] layout)    */
mvs_status mvs_deconv3d_linear_fwd(const float* x_cl, const void* w_packed, const float* bias, float* y_cl, int B, int Cin, int Cout,
                                   int D, int H, int W, int sd, int precision, void* stream);
mvs_status mvs_bn_stats(const float* x_cl, double* sums, long long N, int C, int groups, void* stream);
mvs_status mvs_bn_finalize(const double* sums, double count, float eps, float* mean, float* var, float* invstd, float* running_mean,
                           float* running_var, float momentum, int C, int groups, void* stream);
mvs_status mvs_bn_running_update(const float* mean, const float* var, double count, float momentum, float* running_mean,
                                 float* running_var, int C, int groups, void* stream);
mvs_status mvs_bn_relu_apply(const float* z_cl, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             const float* skip_cl, float* y_cl, long long N, int C, int relu, int groups, void* stream);
mvs_status mvs_bn_relu_bwd(const float* dy_cl, const float* z_cl, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, double* sums, double count, float* dz_cl, long long N, int C, int relu,
                           int use_batch_stats, int phase, int groups, void* stream);
/* One conv / transposed-conv + batch-statistics BatchNorm + ReLU [+ skip] block per call (the launches of the granular entry points
 * chained in C): forward = pack, linear convolution -> z, statistics, finalize (+ running-statistics step), normalise -> y;
 * backward = running-statistics step (the reference's checkpoint recomputation), reduce -> dgamma / dbeta, dz, weight gradient dw
 * ([Cout][Cin][kd*9], ConvTranspose: [Cin][Cout][27]), data gradient da (NULL: not needed).  w = the layer's own fp32 weight;
 * zero_bias: >= 64 zeros; wpack_ws: bf16 scratch of mvs_pack_*_weights_elems elements (max over the block's three packings);
 * sums_ws: double [groups][2C]; B, D, H, W = the block INPUT's batch and size.  SyncBatchNorm / eval-mode BatchNorm: use the
 * granular entry points (an all-reduce sits between statistics and finalize).                                                  */
mvs_status mvs_train_block_fwd(const float* a_in_cl, const float* w, int transposed, int Cin, int Cout, int kd, int sd, int sh, int sw,
                               int B, int D, int H, int W, const float* gamma, const float* beta, float eps, float* running_mean,
                               float* running_var, float momentum, const float* skip_cl, const float* zero_bias, void* wpack_ws,
                               double* sums_ws, float* z_cl, float* mean, float* var, float* invstd, float* y_cl, int groups,
                               void* stream);
mvs_status mvs_train_block_bwd(const float* dy_cl, const float* a_in_cl, const float* z_cl, const float* mean, const float* var,
                               const float* invstd, const float* w, int transposed, int Cin, int Cout, int kd, int sd, int sh, int sw,
                               int B, int D, int H, int W, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, const float* zero_bias, void* wpack_ws, double* sums_ws,
                               float* dz_cl, float* dw, float* dgamma, float* dbeta, float* da_cl, int groups, void* stream);

/* MFMA weight packing on the device (bit-identical to packing.pack_conv_weights_bf16x3 / pack_deconv_weights_bf16x3; used by the
 * training path, which re-packs every un-folded weight each iteration).  *_elems = number of bf16 elements of the packed tensor
 * (-1: unsupported shape).  w: Conv3d [cout][cin][ntap] (tflip = 1: read as [cin][cout] with reversed taps = the data-gradient form
 * of a stride-1 convolution) / ConvTranspose3d [cin][cout][27].                                                               */
long long mvs_pack_conv_weights_elems(int cout, int cin, int ntap, int ch);
mvs_status mvs_pack_conv_weights(const float* w, void* packed_bf16, int cout, int cin, int ntap, int ch, int tflip, void* stream);
long long mvs_pack_deconv_weights_elems(int cin, int cout, int sd);
mvs_status mvs_pack_deconv_weights(const float* w, void* packed_bf16, int cin, int cout, int sd, void* stream);
mvs_status mvs_conv3d_wgrad(const float* a_cl, const float* g_cl, float* dw, int B, int CA, int CB, int D, int H, int W, int kd,
                            int sd, int sh, int sw, void* stream);

/* ---- a7: ConvTranspose3d(k3, padding 1, stride (sd,2,2), output_padding (sd-1,1,1)) + BN + ReLU,
 * then + skip (module.py:129-165, 402-405, 467-481, 498-501).
 * x_cl [B,D,H,W,Cin] -> y_cl [B,D*sd,2H,2W,Cout]; skip_cl has y's shape (NULL = no skip).          */
mvs_status mvs_deconv3d_bn_relu_add_fwd(const float* x_cl, const void* w_packed, const float* bias, const float* skip_cl,
                                        float* y_cl, int B, int Cin, int Cout, int D, int H, int W, int sd, int precision,
                                        void* stream);

/* ---- a7-a9, layer shapes OUTSIDE the tuned tables: shape-generic exact-fp32 Conv3d / ConvTranspose3d -------------------------------
 * Replaces nn.Conv3d / nn.ConvTranspose3d (+ folded BatchNorm3d, ReLU, skip add) of module.py:89-165 for any channel counts, kernel
 * size, stride and padding (dilation 1, groups 1): what a regulariser built with base_ch != 8 (cost_volume.py:29-49: CostRegNet(G, G),
 * widths 2G / 4G / 8G), the 1x1x1 `inner` convolution of in_channels != base_channels (module.py:385-388, 481-484) and a `prob` head of
 * G != 8 channels run on.  No shipped config reaches it: an FMA kernel built for coverage and exactness, not for the roofline.
 *   x_cl [B,D,H,W,Cin] fp32 -> y_cl [B,OD,OH,OW,Cout] fp32;  w_tck [kd*kh*kw][Cin][Cout] fp32 (BN folded; a ConvTranspose3d weight
 *   [Cin,Cout,kd,kh,kw] is laid out the same way, NOT flipped: the kernel gathers i = (o + p - k) / s);  bias [Cout] or NULL;
 *   skip_cl [B,OD,OH,OW,Cout] or NULL, added after bias and ReLU (module.py:403-405).
 *   transposed = 0: O = (N + 2p - k) / s + 1 per axis;  transposed = 1: O = (N - 1) s - 2p + k + output_padding, 0 <= output_padding < s
 *   (the caller states OD, OH, OW; anything else is MVS_ERR_ARG).  Cout == 1 writes what is also a planar [B,OD,OH,OW] volume.          */
mvs_status mvs_conv3d_generic_fwd(const float* x_cl, const float* w_tck, const float* bias, const float* skip_cl, float* y_cl, int B,
                                  int Cin, int Cout, int D, int H, int W, int OD, int OH, int OW, int kd, int kh, int kw, int sd, int sh,
                                  int sw, int pd, int ph, int pw, int transposed, int relu, void* stream);
/* 1 when mvs_conv3d_bn_relu_fwd / mvs_deconv3d_bn_relu_add_fwd have a tuned MFMA kernel for the layer shape (kernel (kd,3,3), padding
 * (kd/2,1,1) / the k3 p1 (sd,2,2) transposed form), else 0: the host mirror routes the layer to mvs_conv3d_generic_fwd then */
int mvs_conv3d_is_tuned(int Cin, int Cout, int kd, int sd, int sh, int sw);
int mvs_deconv3d_is_tuned(int Cin, int Cout, int sd);

/* the last U-Net layer with the 1x1x1 `prob` head in its epilogue (Cout = 8): x_cl [B,D,H,W,Cin] -> logits [B,D*sd,2H,2W]
 * = prob(skip + relu(bn(deconv(x)))); MVS_PREC_BF16X3 only.  mvs_regnet_logits_fwd chains it after the other eight layers. */
mvs_status mvs_deconv3d_prob_fwd(const float* x_cl, const void* w_packed, const float* bias, const float* skip_cl, const float* prob_w,
                                 const float* prob_b, float* logits, int B, int Cin, int D, int H, int W, int sd, int precision,
                                 void* stream);

/* ---- a8/a9: whole regulariser U-Net (CostRegNet / CostRegNet3D), module.py:367-408 / 453-504 ----
 * volume_cl [B,D,H,W,8] -> feat_cl [B,D,H,W,8] = conv0 + relu(bn(deconv11(...))) (input of `prob`).
 * params: 9 packed weight pointers + 9 bias pointers in layer order conv1..conv6, conv7, conv9, conv11.*/
size_t mvs_regnet_workspace_bytes(int kind, int B, int D, int H, int W);
mvs_status mvs_regnet_fwd(int kind, const float* volume_cl, const void* const* w_packed, const float* const* bias,
                          float* feat_cl, void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int precision,
                          void* stream);
/* the same U-Net with a 1x1x1 `prob` head (CostRegNet3D, module.py:486,502: prob_w [8], prob_b [1]) applied in the epilogue
 * of the last ConvTranspose3d: volume_cl -> logits [B,D,H,W] = prob_volume_pre; the 8-channel full-resolution feature
 * volume is never written (MVS_PREC_BF16X3 only).  Follow with mvs_softmax_regress_fwd.                              */
mvs_status mvs_regnet_logits_fwd(int kind, const float* volume_cl, const void* const* w_packed, const float* const* bias,
                                 const float* prob_w, const float* prob_b, float* logits, void* workspace, size_t workspace_bytes,
                                 int B, int D, int H, int W, int precision, void* stream);

/* ---- a8/a9 `prob` + a10 + a11: logits, softmax, depth regression, confidence --------------------
 * feat_cl [B,D,H,W,8]; prob_w: [8] (+ prob_b[1]) for the 1x1x1 head (CostRegNet3D, module.py:486)
 * or [27][8] tap-major for the 3x3x3 head without bias (CostRegNet, module.py:391; prob_b = NULL).
 * hyp [B,D,H,W].  mode: MVS_HEAD_*.  conf_n: window of conf_regression for MVS_HEAD_REG (0 = max prob).
 * Outputs (any of prob_volume / prob_volume_pre may be NULL): depth [B,H,W], conf [B,H,W],
 * prob_volume [B,D,H,W], prob_volume_pre [B,D,H,W].                                                */
mvs_status mvs_prob_regress_fwd(const float* feat_cl, const float* prob_w, const float* prob_b, int prob_ksize,
                                const float* hyp, float tmp, int mode, int conf_n, float* depth, float* conf,
                                float* prob_volume, float* prob_volume_pre, int B, int D, int H, int W, void* stream);
/* same head on precomputed logits [B,D,H,W] (depth_regression / conf_regression callers) */
mvs_status mvs_softmax_regress_fwd(const float* logits, const float* hyp, float tmp, int mode, int conf_n, float* depth,
                                   float* conf, float* prob_volume, int B, int D, int H, int W, void* stream);
/* Round 5: a stage's head fused with the NEXT stage's inverse-depth schedule (mvs_softmax_regress_fwd + mvs_schedule_inverse_range_fwd with
 * shift = 0 in one launch; DINOv2_mvsformer_model.py:133-148 + cost_volume.py:105-131): besides depth / conf / prob_volume it writes
 * next_hyp [B,next_D,2H,2W] from this stage's depth and hypotheses (module.py:707-724, `ratio` = the next stage's depth_interals_ratio).
 * depth / conf / prob_volume are bit-identical to mvs_softmax_regress_fwd's; next_hyp equals the stand-alone schedule's up to FMA
 * contraction of the two translation units (<= 2e-6 of its range; bit-identical on the shipped build).                               */
mvs_status mvs_softmax_regress_schedule_fwd(const float* logits, const float* hyp, float tmp, int mode, int conf_n, float* depth, float* conf,
                                            float* prob_volume, float ratio, float* next_hyp, int next_D, int B, int D, int H, int W,
                                            void* stream);
/* Round 5: the LAST cascade stage's head with a16 fused (DINOv2_mvsformer_model.py:167-177): besides depth / conf / prob_volume it writes
 * conf_avg [B,H,W] = (sum_i nearest-upsampled prev_conf[i] + conf) / (n_prev + 1); prev_conf[i] is [B, H >> shift[i], W >> shift[i]]
 * (host arrays of n_prev <= 7 device pointers / shifts, earliest stage first: the summation order of mvs_confidence_average).    */
mvs_status mvs_softmax_regress_confavg_fwd(const float* logits, const float* hyp, float tmp, int mode, int conf_n, float* depth,
                                           float* conf, float* prob_volume, const float* const* prev_conf_host_ptrs,
                                           const int* prev_shifts_host, int n_prev, float* conf_avg, int B, int D, int H, int W,
                                           void* stream);

/* module.py:649-671 as free functions on a probability volume p [B,D,H,W]:
 * depth_regression: out = sum_d p*depth_values (depth_values [B,D,H,W]); conf_regression: window sum of n. */
mvs_status mvs_depth_regression_fwd(const float* p, const float* depth_values, float* out, int B, int D, int H, int W, void* stream);
mvs_status mvs_conf_regression_fwd(const float* p, int n, float* out, int B, int D, int H, int W, void* stream);

/* ---- a13-a15: hypothesis ranges, module.py:674-741 ----------------------------------------------*/
mvs_status mvs_init_range_fwd(const float* depth_values /*[B,N]*/, int N, int inverse, float* hyp /*[B,D,H,W]*/, int B,
                              int D, int H, int W, void* stream);
/* the per-pixel form of the two (module.py:683-688, 698-703): depth_values [B,H,W,N], every pixel's own first / last depth */
mvs_status mvs_init_range_pixel_fwd(const float* depth_values /*[B,H,W,N]*/, int N, int inverse, float* hyp /*[B,D,H,W]*/, int B,
                                    int D, int H, int W, void* stream);
/* prev_depth [B,H/2,W/2], prev_hyp [B,Dprev,H/2,W/2] -> hyp [B,D,H,W]; ratio = depth_interals_ratio; shift != 0: the reference's
 * `shift=True` branch (module.py:712-715), statement by statement                                                             */
mvs_status mvs_schedule_inverse_range_fwd(const float* prev_depth, const float* prev_hyp, int Dprev, float ratio, int shift,
                                          float* hyp, int B, int D, int H, int W, void* stream);
/* interval [B] = depth_interals_ratio * depth_interval, or (interval_per_pixel != 0) [B,H/2,W/2] (module.py:727-741) */
mvs_status mvs_schedule_range_fwd(const float* prev_depth, const float* interval, int interval_per_pixel, float* hyp, int B, int D,
                                  int H, int W, void* stream);

/* ---- a16: confidence fusion, DINOv2_mvsformer_model.py:167-177 -----------------------------------
 * out[b,y,x] = mean_s conf_s[b, y >> shift_s, x >> shift_s] (nearest upsample), n_stages <= 8.      */
mvs_status mvs_confidence_average(const float* const* conf_host_ptrs, const int* shifts_host, int n_stages, float* out,
                                  int B, int H, int W, void* stream);

/* ==== section 8f #1: stage-1 transformer regulariser of the shipped config =========================
 * PureTransformerCostReg module.py:602-646 (FlashAttnBlock :535-583, FFN :507-532, LayerNorm3D :586-599), softmax
 * attention models/dino/layers/attention.py:76-101,141-170, Frustoconical PE models/position_encoding.py:138-189.
 * Tokens are rows [B, n, 64] fp32, n = (D/rd)(H/rh)(W/rw), token index (td*H/rh + th)*W/rw + tw (attention is
 * invariant to the order; the reference's "(h w d)" order, module.py:573, is not reproduced).  All contractions
 * are MVS_PREC_BF16X3 (fp32-equivalent); other precisions return MVS_ERR_UNSUPPORTED.  Packed weights come from
 * packing.pack_linear_bf16x3 (layout in mvsformerplusplus_amd/packing.py).                                        */

/* get_position_3d(normalize=True), position_encoding.py:138-163.  K [B,3,3] = proj[:,0,1,:3,:3] of the stage,
 * hyp [B,D,H,W], depth_values [B*n] (only its min / max are used).  range [6] = {height_min, height_max, width_min,
 * width_max, depth_min, depth_max}: with compute_range != 0 the first four are measured over the whole volume
 * (stage 1) and written, otherwise they are read (later stages reuse stage 1's, DINOv2_mvsformer_model.py:152-160);
 * the last two are always written.  -> position3d [B,3,D,H,W] in 0..1.                                            */
size_t mvs_position3d_workspace_bytes(void);
mvs_status mvs_position3d_fwd(const float* K, const float* hyp, const float* depth_values, int n_depth_values, float* range,
                              int compute_range, float* workspace, size_t workspace_bytes, float* position3d, int B, int D,
                              int H, int W, void* stream);

/* get_position_3d(normalize=False), position_encoding.py:146-149: position3d [B,3,D,H,W] = K^-1 [x, y, 1] * depth, no ranges (v10) */
mvs_status mvs_position3d_raw_fwd(const float* K, const float* hyp, float* position3d, int B, int D, int H, int W, void* stream);
/* PositionEncoding3D(position3d, C, rescale) as a tensor of its own, position_encoding.py:164-189: position3d [B,3,N] (N = D*H*W) ->
 * pe [B,3C,N], channel ax*C + 2f = sin(pos_ax * rescale * div_f), + 1 = cos; div_term [C/2] (device) = the frequencies
 * exp(2f * (-ln 1e4 / C)) as the caller computed them; C even.  The hot path never materialises the encoding (mvs_tr_embed_fwd
 * evaluates it per token); this is the standalone form for callers of the function (v10)                                        */
mvs_status mvs_position_encoding3d_fwd(const float* position3d, const float* div_term, float* pe, int B, int C, float rescale, long long N,
                                       void* stream);

/* x + pe_proj(PositionEncoding3D(position3d, 8)) (module.py:631-635, position_encoding.py:166-189; skipped when
 * position3d == NULL), `down` = Conv3d(8, 64, kernel = stride = (rd,rh,rw)) + bias + LayerNorm3D(64, eps 1e-6).
 * volume_cl [B,D,H,W,8], pe_w = pe_proj.weight [8][24], pe_div_host = the 4 frequencies exp(2k * -ln(1e4)/8) (HOST
 * pointer), w_packed = pack_linear_bf16x3(down.0.weight as [64][patch_voxel*8 + c]) -> tokens [B,n,64].           */
mvs_status mvs_tr_embed_fwd(const float* volume_cl, const float* position3d, const float* pe_w, const float* pe_div_host,
                            const void* w_packed, const float* bias, const float* ln_w, const float* ln_b, float* tokens,
                            int B, int D, int H, int W, int rd, int rh, int rw, int precision, void* stream);

/* y = epilogue(x @ W^T): x [B,n,K], W [N,K] packed, y [B,n,N].
 *   MVS_TR_EPI_BIAS    y = x W^T (+ bias)                                                K = 64
 *   MVS_TR_EPI_GELU    y = gelu(x W^T + bias), exact erf form (FFN.linear1 + act)         K = 64
 *   MVS_TR_EPI_RES_LN  y = LayerNorm(residual + gamma[0] * (x W^T + bias)), N = 64        K = 64 | 256
 *                      (attn.proj / ffn.linear2 + layer scale + post-norm, module.py:575-576)                      */
mvs_status mvs_tr_linear_fwd(const float* x, const void* w_packed, const float* bias, int epilogue, const float* residual,
                             const float* gamma, const float* ln_w, const float* ln_b, float ln_eps, float* y, int B, int n,
                             int K, int N, int precision, void* stream);

/* attn.qkv (no bias) written as the operands of the attention kernel, q pre-scaled by softmax_scale * log2 e.  softmax_scale =
 * head_dim^-0.5 * log(n) / log(train_avg_length) for "entropy_invariance" (attention.py:158-161).  heads = 4, head_dim = 16.
 * `precision` = contraction of the projection itself (MVS_PREC_BF16X3); `operand_format` = what the attention kernel will read:
 *   MVS_PREC_BF16X3 (or _BF16P)  q, k as [B,heads,npad,32] bf16 = [hi16 | lo16], v transposed as [B,heads,2,16,npad] bf16, npad = n
 *                                rounded up to 64 (rounds 1-3: fp32-equivalent attention)
 *   MVS_PREC_ATTN16              ONE 16-bit term per operand like the reference's flash-attn (dino/layers/attention.py:141-170 runs q, k, v,
 *                                p in bf16): q, k fp16 (clamped to +-65504), v bf16 (the probabilities are bf16 in the kernel); q
 *                                [B,heads,npad,16]; k as score-MFMA operand tiles [B,heads,npad/32,4,16,2,4]; v as p.v-MFMA operand tiles
 *                                [B,heads,npad/32,4,16,8] in the key order the scores leave the matrix core in
 *                                (csrc/attention_f16_kernels.hip); npad = n rounded up to 256
 * Each buffer holds mvs_tr_attention_operand_bytes(B, n, heads) bytes (enough for either format).                              */
size_t mvs_tr_attention_operand_bytes(int B, int n, int heads);
mvs_status mvs_tr_qkv_fwd(const float* x, const void* w_packed, void* q, void* k, void* vt, float softmax_scale, int B, int n,
                          int heads, int precision, int operand_format, void* stream);
/* softmax(q k^T) v over all n tokens -> out [B,n,heads*16] (scaled_dot_product_attention, attention.py:96);
 * precision = the operand format of mvs_tr_qkv_fwd: MVS_PREC_BF16X3 (four-term scores, three-term p.v), MVS_PREC_BF16P (the same with
 * one-term probabilities) or MVS_PREC_ATTN16 (fp16 q / k, bf16 p / v, one MFMA term, fp32 softmax statistics and accumulation)              */
mvs_status mvs_tr_attention_fwd(const void* q, const void* k, const void* vt, float* out, int B, int n, int heads,
                                int precision, void* stream);
/* Backward of the attention core (training path; the reference differentiates scaled_dot_product_attention / flash-attn,
 * dino/layers/attention.py:141-170): qkv [B,n,3,heads,16] fp32 = the projection's plain output (q | k | v), o [B,n,heads*16] the
 * forward result, d_o its gradient -> d_qkv [B,n,3,heads,16] (dq | dk | dv).  fp32 throughout, two launches, no atomics.
 * lse_ws / dsum_ws: B*heads*n floats each (log-sum-exp and sum_c d_o*o per query row, produced by the first launch).            */
mvs_status mvs_tr_attention_bwd(const float* qkv, const float* o, const float* d_o, float* d_qkv, float* lse_ws, float* dsum_ws,
                                int B, int n, int heads, float softmax_scale, void* stream);

/* `up` = ConvTranspose3d(64, 8, kernel = stride = (rd,rh,rw)) + bias + LayerNorm3D(8, eps 1e-6), then `prob` =
 * Conv3d(8, 1, 1) + bias (module.py:621-626, 643-644): tokens [B,n,64] -> logits [B,D,H,W].
 * w_packed = pack_linear_bf16x3(up.0.weight as [patch_voxel*8 + co][ci]).                                          */
mvs_status mvs_tr_up_prob_fwd(const float* tokens, const void* w_packed, const float* up_bias, const float* ln_w,
                              const float* ln_b, const float* prob_w, const float* prob_b, float* logits, int B, int D, int H,
                              int W, int rd, int rh, int rw, int precision, void* stream);

/* ==== section 8f #3: depth-map filtering after inference ============================================
 * misc/fusion.py (reprojection-consistency filters) as driven by test.py:388-409 ("pcd") and test.py:455-483 ("dpcd").
 * Cameras: [N,2,4,4] as everywhere (0 = extrinsic world->camera, 1 = intrinsic in the top-left 3x3), first packed once per
 * camera into mvs_fusion_campack_floats() floats {K, K^-1, E, E^-1} (the reference inverts them per call, fusion.py:24,32).
 * Depth / confidence maps are planar fp32 [n,h,w] / [n,v,h,w]; pixel centres sit at +0.5 (fusion.py:9-10).              */
size_t mvs_fusion_campack_floats(void);
mvs_status mvs_fusion_prepare_cams(const float* cams /*[N,2,4,4]*/, int N, float* packed /*[N,campack]*/, void* stream);
/* dynamic = 0: get_reproj (fusion.py:80-97) + vis_filter (:100-109) + ave_fusion (:112-114); p0 = img_dist_thresh,
 *              p1 = depth_thresh, vthresh = view threshold; srcs_conf (nullable) zeroes source depths with conf <=
 *              conf_thresh (test.py:389-392); vis_masks [n,v,h,w].
 * dynamic = 1: get_reproj_dynamic (:116-153) + vis_filter_dynamic (:156-168) + test.py:463-476; p0 = dist_base,
 *              p1 = rel_diff_base; vis_masks [n,v,v-1,h,w]; v >= 2.
 * Either computes the reprojection from depths + cameras (xyd_in = NULL; written to xyd_out [n,v,3,h,w] / in_range_out
 * [n,v,h,w] when non-NULL) or starts from a given one (xyd_in, in_range_in).  With depth != NULL the filter runs:
 * depth [n,h,w] = averaged depth, geo_mask / mask [n,h,w] (mask = geo & (ref_conf > conf_thresh), ref_conf nullable),
 * points [n,3,h,w] = world coordinates of the averaged depth (test.py:406-409); any of vis_masks / geo_mask / mask /
 * points may be NULL.  v <= 16.                                                                                          */
mvs_status mvs_fusion_filter_fwd(int dynamic, const float* ref_depth, const float* ref_conf, const float* srcs_depth,
                                 const float* srcs_conf, const float* ref_cam_packed, const float* srcs_cam_packed,
                                 const float* xyd_in, const float* in_range_in, float conf_thresh, float p0, float p1, float vthresh,
                                 float* xyd_out, float* in_range_out, uint8_t* vis_masks, float* depth, uint8_t* geo_mask,
                                 uint8_t* mask, float* points, int n, int v, int h, int w, void* stream);
/* ave_fusion (fusion.py:112-114) on its own: masks [n,v,h,w] fp32 */
mvs_status mvs_fusion_ave_fwd(const float* ref_depth, const float* reproj_xyd, const float* masks, float* out, int n, int v, int h,
                              int w, void* stream);

/* ==== point cloud: the filtered views of a scene as one binary PLY body =====================
 * The per-view body after the filter in test.py filter_depth (:414-442) / dynamic_filter_depth (:485-517): keep the pixels of
 * the final mask in row-major order (points_np[i, k][mask_np[i, 0]], :419 / :491), take the reference image's colours
 * (:421-424 / :493-497), concatenate the views (:429 / :504) and pack the PLY vertex array (the tuple loop of :431-441 / :506-516).
 * One view per call: mask [h,w] u8 and points [3,h,w] fp32 as mvs_fusion_filter_fwd writes them, rgb [h,w,3] u8.  The kept
 * pixels land as packed 15-byte little-endian records {float x, y, z; uchar red, green, blue} in `records` (4-byte aligned,
 * capacity records) starting at record *counter; *counter advances by the view's count, which is also written to
 * view_counts[view_slot] (view_counts nullable).  Three launches on `stream`, no host synchronisation, bit-reproducible.
 * The caller keeps *counter + h*w <= capacity (records past the capacity are dropped, the counter still advances).
 * workspace: mvs_pointcloud_workspace_bytes(h, w) bytes, stream-ordered scratch.                                          */
size_t mvs_pointcloud_workspace_bytes(int h, int w);
mvs_status mvs_pointcloud_append(const uint8_t* mask, const float* points, const uint8_t* rgb, int h, int w, void* workspace,
                                 size_t workspace_bytes, unsigned* counter, unsigned* view_counts, int view_slot, uint8_t* records,
                                 long long capacity, void* stream);

/* ==== gipuma route: fusibile's cross-view consistency fusion as misc/gipuma.py drives it ===========
 * The probability filter (misc/gipuma.py:160-181), the camera conversion (:72-92: P = [K 0; 0 1] E, first three rows) and the
 * fusion fusibile performs on the converted folder (:184-205), restated from the project's contract.  N views of one size h x w,
 * device-resident: depths fp32 [N,h,w] (filtered), colours u32 [N,h,w] (r | g << 8 | b << 16), used u8 [N,h,w] (zeroed once).
 * mvs_gipuma_prepare_cams is HOST code (fp64): cams [N,2,4,4] fp32 as everywhere -> view_consts [N, view_floats] and
 * pair_consts [N, N, pair_floats] (fp32, host memory; the caller uploads them).  Fails on a singular P[:, :3].              */
size_t mvs_gipuma_view_floats(void);
size_t mvs_gipuma_pair_floats(void);
mvs_status mvs_gipuma_prepare_cams(const float* cams, int N, float* view_consts, float* pair_consts);
/* one view's slot: depth_out = keep ? depth : 0 (keep u8 [h,w] nullable = keep all), color_out = packed rgb [h,w,3] u8     */
mvs_status mvs_gipuma_prepare_view(const float* depth, const uint8_t* keep, const uint8_t* rgb, int h, int w, float* depth_out,
                                   uint32_t* color_out, void* stream);
/* one launch per reference view r, in processing order on ONE stream (the marks of launch r are read by the later launches):
 * mask [h,w] u8, points [3,h,w] fp32, rgb [h,w,3] u8 of view r, as mvs_pointcloud_append reads them (points / rgb are written
 * for kept pixels only); used[c][v][u] = 1 for every pixel an emitted vertex used (c != r).  depth_min / depth_max are applied
 * exactly as in fp64 to the fp32 map values; a vertex needs n >= num_consistent consistent views.  skipped (nullable,
 * diagnostic) receives the used[r] the launch read.                                                                        */
mvs_status mvs_gipuma_fuse_view(const float* depths, const uint32_t* colors, uint8_t* used, const float* view_consts,
                                const float* pair_consts, int N, int h, int w, int r, double depth_min, double depth_max,
                                float disp_thresh, double num_consistent, uint8_t* mask, float* points, uint8_t* rgb,
                                uint8_t* skipped, void* stream);

/* ==== colmap2mvsnet: view-selection scores and depth values of a COLMAP model =====================
 * fp64 throughout, device-resident.  mvs_colmap_depths: z[k] = erow[obs_img[k]] . [xyz[obs_pt[k]], 1] for n observations
 * (erow = row 2 of each image's [R|t; 0 1], [N, 4]; xyz [P, 3]).  mvs_colmap_scores: score [N, N] (zeroed here) for N <= 16384
 * images from a per-image CSR (img_ptr [N+1], img_pts sorted unique dense point indices, img_mult their multiplicities) and a
 * per-point CSR of ascending unique images (pt_ptr [P+1], pt_imgs); centres [N, 3] = -R^T t; den1 / den2 = 2 sigma1^2,
 * 2 sigma2^2.  max_pairs >= the number of co-visible pairs i < j sizes `pairs` (u32); flags u8 [N, N] scratch (zeroed here);
 * workspace of mvs_colmap_workspace_bytes(N) (0 = N out of range).  Deterministic: no atomics, fixed reduction order.     */
size_t mvs_colmap_workspace_bytes(int N);
mvs_status mvs_colmap_depths(const int* obs_img, const int* obs_pt, long long n, const double* xyz, const double* erow, double* z, void* stream);
mvs_status mvs_colmap_scores(const int* img_ptr, const int* img_pts, const int* img_mult, int N, const int* pt_ptr, const int* pt_imgs, int P,
                             const double* xyz, const double* centres, double theta0, double den1, double den2, long long max_pairs,
                             uint8_t* flags, unsigned* pairs, void* workspace, size_t workspace_bytes, double* score, void* stream);

/* ==== FPN feature encoder and decoder at full image resolution ========================================
 * models/module.py:47-86 (Conv2d: conv without bias + BatchNorm2d + leaky_relu 0.1), models/module.py:200-270 (FPNEncoder,
 * FPNDecoder) with feat_chs = [8, 16, 32, 64] (DINOv2_mvsformer_model.py:34-35, casmvs_model.py:33-34).  All tensors planar fp32,
 * contiguous [N, C, H, W].  Split-bf16 three-term MFMA contraction (fp32-equivalent); BatchNorm folded on the host.
 * mvs_fpn_conv_fwd: Conv2d(Cin, Cout, k, stride, padding k/2) + bias [Cout] (nullable) + act (0 none, 1 Swish, 2 LeakyReLU 0.1);
 *   x [N,Cin,H,W] -> y [N,Cout,(H-1)/stride+1,(W-1)/stride+1]; w_packed = packing.pack_conv_weights_bf16x3(w (Cin padded to a
 *   multiple of 8)[:, :, None], packing.fpn_chunk(Cin, stride)).  mvs_fpn_conv_is_built lists the (Cin, Cout, k, stride) that exist.
 * mvs_fpn_merge_fwd (module.py:262-266): intra [N,64,H,W] = up2(prev [N,64,H/2,W/2]) + b_inner + w_inner [64,Clat] . lateral
 *   [N,Clat,H,W]; up2 = bilinear x2, align_corners=True, source index dst * (in - 1) / (out - 1) in fp32.
 * mvs_fpn_merge_conv_fwd (module.py:267-268): y = act(conv3x3(intra) + bias) with intra as above computed inside the convolution's
 *   staging - the 64-channel full-resolution intra is never written.  mvs_fpn_merge_is_built(Clat, 0) = the merge alone,
 *   (Clat, Cout) = the fused last level.  H and W even.                                                                              */
int mvs_fpn_conv_is_built(int Cin, int Cout, int k, int stride);
int mvs_fpn_merge_is_built(int Clat, int Cout);
mvs_status mvs_fpn_conv_fwd(const float* x, const void* w_packed, const float* bias, int act, float* y, int N, int Cin, int Cout, int k, int stride,
                            int H, int W, void* stream);
mvs_status mvs_fpn_merge_fwd(const float* prev, const float* lateral, const float* w_inner, const float* b_inner, float* intra, int N, int Clat,
                             int H, int W, void* stream);
mvs_status mvs_fpn_merge_conv_fwd(const float* prev, const float* lateral, const float* w_inner, const float* b_inner, const void* w_packed,
                                  const float* bias, int act, float* y, int N, int Clat, int Cout, int H, int W, void* stream);

/* ---- FPNDecoder in train mode: out_k = Swish(BatchNorm2d(conv(intra_k) + b)) with batch statistics over
 * all N H W samples of a channel, and its backward.  The forward convolutions are mvs_fpn_conv_fwd / mvs_fpn_merge_conv_fwd on
 * un-folded weights with bias = NULL, act 0 (a bias in front of a batch-statistics BatchNorm cancels).  Sums are fp64, left as
 * per-workgroup partials in `workspace` and added in a fixed order: no atomics, bit-identical run to run.  *_workspace_bytes: 0 = out
 * of range or not built.
 * mvs_fpn_bn_swish_fwd: z [N,C,H,W], C <= 64 -> stats [3][C] = mean | biased variance | 1 / sqrt(var + eps) and y = swish(gamma xhat +
 *   beta); running_mean / running_var (both or neither) take one step of `momentum` with mean + conv_bias (nullable) and the unbiased
 *   variance, like nn.BatchNorm2d behind a convolution with that bias.
 * mvs_fpn_bn_swish_bwd: dy, z, stats -> d_beta = sum du, d_gamma = sum du xhat, du = dy (s + u s (1 - s)), u = gamma xhat + beta,
 *   s = sigmoid(u), and dz = gamma invstd (du - d_beta / M - xhat d_gamma / M), M = N H W.
 * mvs_fpn_train_conv_fwd: Conv2d(Cin, Cout, k, padding k/2) without bias or activation, the data gradients' instances of the
 *   convolution (mvs_fpn_train_conv_is_built); w_packed = packing.pack_fpn_conv_weights(w, 1) of the flipped, channel-transposed taps.
 * mvs_fpn_wgrad: dw [Cout][Cin + ones][k][k] = sum_pixels dy [N,Cout,H,W] (x) x [N,Cin,H,W] shifted by the tap (zero padding), exact fp32
 *   products (v_mfma_f32_16x16x4_f32).  ones = 1 appends an input channel that is 1 inside the image: dw[:, Cin] is the gradient of a bias
 *   behind the taps.  Built: (Cout, Cin, k, ones) = (32|16, 64, 3, 0), (64, 64, 1, 0), (64, 32|16, 1, 1), (8, 8, 3, 1).
 * mvs_fpn_merge_wgrad: the last level's dw [8][64][3][3] with x = up2(prev) + inner(lateral) (mvs_fpn_merge_fwd's map) re-evaluated in
 *   the kernel's staging and never written.
 * mvs_fpn_up2_adjoint: d_coarse [N,64,H/2,W/2] = U^T d_fine [N,64,H,W], U = mvs_fpn_merge_fwd's upsample; a gather with the forward's own
 *   coordinate function (the exact adjoint).  H and W even.                                                                          */
size_t mvs_fpn_bn_workspace_bytes(int N, int C, int H, int W);
mvs_status mvs_fpn_bn_swish_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var, float* stats, float* y, void* workspace, size_t workspace_bytes, int N, int C,
                                int H, int W, void* stream);
mvs_status mvs_fpn_bn_swish_bwd(const float* dy, const float* z, const float* stats, const float* gamma, const float* beta, float* dz, float* d_gamma,
                                float* d_beta, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, void* stream);
int mvs_fpn_train_conv_is_built(int Cin, int Cout, int k);
mvs_status mvs_fpn_train_conv_fwd(const float* x, const void* w_packed, float* y, int N, int Cin, int Cout, int k, int H, int W, void* stream);
size_t mvs_fpn_wgrad_workspace_bytes(int N, int Cin, int Cout, int k, int ones, int H, int W);
mvs_status mvs_fpn_wgrad(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int k, int ones,
                         int H, int W, void* stream);
size_t mvs_fpn_merge_wgrad_workspace_bytes(int N, int H, int W);
mvs_status mvs_fpn_merge_wgrad(const float* dy, const float* prev, const float* lateral, const float* w_inner, const float* b_inner, float* dw,
                               void* workspace, size_t workspace_bytes, int N, int H, int W, void* stream);
mvs_status mvs_fpn_up2_adjoint(const float* d_fine, float* d_coarse, int N, int H, int W, void* stream);

/* ---- FPNEncoder in train mode: eleven blocks leaky_relu(BatchNorm2d(conv(x)), 0.1) with batch statistics, and
 * their backward.  The forward convolutions, and the data gradients of the stride-1 blocks (Cin = Cout: flipped, channel-transposed taps),
 * are mvs_fpn_conv_fwd with bias = NULL, act 0.  No atomics: bit-identical run to run.
 * mvs_fpn_bn_leaky_fwd / _bwd: mvs_fpn_bn_swish_fwd / _bwd's arguments and workspace (mvs_fpn_bn_workspace_bytes; conv_bias may be NULL) with
 *   y = leaky_relu(u, 0.1), u = gamma xhat + beta, and du = dy (u > 0 ? 1 : 0.1) with u recomputed from z and stats.
 * mvs_fpn_enc_wgrad: dw [Cout][Cin][k][k] = sum_pixels dy [N,Cout,OH,OW] (x) x [N,Cin,H,W] at stride `stride`, padding k/2, OH = (H - 1) /
 *   stride + 1; exact fp32 products.  Built: (Cout, Cin, k, stride) = (8,3,7,1), (8,8,5,1), (16,8,5,2), (16,16,3,1), (32,16,5,2), (32,32,3,1),
 *   (64,32,3,2), (64,64,3,1).  mvs_fpn_enc_wgrad_workspace_bytes: 0 = not built or out of range.
 * mvs_fpn_enc_dgrad: dx [N,Cin,H,W] (H, W even) = the stride-2 transposed convolution of dz [N,Cout,H/2,W/2] with the layer's weight
 *   [Cout][Cin][k][k], padding k/2, as four parity classes of 3x3 convolutions; w_packed = packing.pack_fpn_enc_dgrad_weights(w)
 *   (mvs_fpn_enc_dgrad_weights_bytes bytes).  Built (mvs_fpn_enc_dgrad_is_built, stride 2 only): (Cin, Cout, k) = (8,16,5), (16,32,5),
 *   (32,64,3).                                                                                                                         */
mvs_status mvs_fpn_bn_leaky_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var, float* stats, float* y, void* workspace, size_t workspace_bytes, int N, int C,
                                int H, int W, void* stream);
mvs_status mvs_fpn_bn_leaky_bwd(const float* dy, const float* z, const float* stats, const float* gamma, const float* beta, float* dz, float* d_gamma,
                                float* d_beta, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, void* stream);
size_t mvs_fpn_enc_wgrad_workspace_bytes(int N, int Cin, int Cout, int k, int stride, int H, int W);
mvs_status mvs_fpn_enc_wgrad(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int k,
                             int stride, int H, int W, void* stream);
int mvs_fpn_enc_dgrad_is_built(int Cin, int Cout, int k, int stride);
size_t mvs_fpn_enc_dgrad_weights_bytes(int Cin, int Cout, int k);
mvs_status mvs_fpn_enc_dgrad(const float* dz, const void* w_packed, float* dx, int N, int Cin, int Cout, int k, int H, int W, void* stream);

/* ==== FMT_with_pathway: stage-1 linear attention + pathway ============================================
 * models/FMT.py:35-206 with the shipped FMT_config (Linear attention, d_model 64, 4 heads, ffn, pre-norm, LayerScale).  Token
 * tensors are the feature maps themselves: planar fp32 [N, 64, n], n = h w.  Split-bf16 three-term MFMA GEMMs (fp32-equivalent);
 * LayerNorm, elu, the normaliser, GELU (erf) and the residuals in fp32.  w_packed (mvs_fmt_weights_bytes) and vectors
 * (mvs_fmt_vectors_bytes) of one block come from packing.pack_fmt_block.
 * mvs_fmt_kv_fwd: key/value summary of kv = LN1(x [+ pe]) per view: k = elu(Wk kv) + 1, v = Wv kv, KV_h = sum_s k_s (x) v_s (exact
 *   fp32 products), ksum_h = sum_s k_s -> kv_operand [N] of mvs_fmt_kv_operand_bytes each (a packed split-bf16 GEMM operand).
 *   Per-workgroup partials in `workspace` (mvs_fmt_kv_workspace_bytes(N, n); 0 = out of range) are added in a fixed order: no
 *   atomics, bit-identical run to run.  pe (nullable) [64, n] is added to x first.
 * mvs_fmt_block_fwd: y = block(x [+ pe]) for N views; view i attends to kv_operand[i / kv_div] (self attention: its own, kv_div 1;
 *   cross attention: the reference view's of its batch element, kv_div = V - 1).  One launch; q, the attention output and the 256-wide
 *   hidden activation stay in registers.
 * mvs_fmt_path_fwd: y [N,C,H,W] = conv3x3(bilinear(w_reduce [C,2C] . prev [N,2C,h,w], size (H,W), align_corners=False) + lateral
 *   [N,C,H,W]), zero padding, no biases, C = 32 | 16 | 8, any h, w, H, W >= 1; the merged map is computed inside the convolution's
 *   staging and never written.  w_packed = packing.pack_fpn_conv_weights(w, 1).
 * mvs_fmt_merge_fwd + mvs_fmt_smooth_fwd: the same level unfused (the merged map written, then the convolution alone).            */
size_t mvs_fmt_weights_bytes(void);
size_t mvs_fmt_vectors_bytes(void);
size_t mvs_fmt_kv_operand_bytes(void);
size_t mvs_fmt_kv_workspace_bytes(int N, int n);
mvs_status mvs_fmt_kv_fwd(const float* x, const float* pe, const void* w_packed, const float* vectors, void* workspace, size_t workspace_bytes,
                          void* kv_operand, int N, int n, void* stream);
mvs_status mvs_fmt_block_fwd(const float* x, const float* pe, const void* kv_operand, const void* w_packed, const float* vectors, float* y, int N,
                             int n, int kv_div, void* stream);
mvs_status mvs_fmt_path_fwd(const float* prev, const float* lateral, const float* w_reduce, const void* w_packed, float* y, int N, int C, int h, int w,
                            int H, int W, void* stream);
mvs_status mvs_fmt_merge_fwd(const float* prev, const float* lateral, const float* w_reduce, float* merged, int N, int C, int h, int w, int H, int W,
                             void* stream);
mvs_status mvs_fmt_smooth_fwd(const float* x, const void* w_packed, float* y, int N, int C, int H, int W, void* stream);
/* Backward of one pathway level Y = S * M, M = U(W_r prev) + lateral.  d lateral = dM is mvs_fmt_smooth_fwd of
 * dY with S's taps flipped and its channel axes exchanged.  Weight gradients are per-workgroup fp32 partials in `workspace` (the
 * *_workspace_bytes queries; 0 = out of range or not built) added in a fixed order: no atomics, bit-identical run to run.
 * mvs_fmt_path_bwd: d_merged [N,C,H,W] -> d_prev [N,2C,h,w] = W_r^T U^T(dM) and d_w_reduce [C,2C] = sum U^T(dM) (x) prev; U^T gathers
 *   with the forward's own coordinate function (the exact adjoint; any h, w, H, W >= 1).
 * mvs_fmt_smooth_wgrad: d_w_smooth [C,C,3,3] = sum_pixels dY (x) M shifted by the tap, exact fp32 products; M is recomputed from
 *   prev, lateral and w_reduce in the kernel's staging and never written.                                                          */
size_t mvs_fmt_path_bwd_workspace_bytes(int N, int C, int h, int w);
mvs_status mvs_fmt_path_bwd(const float* d_merged, const float* prev, const float* w_reduce, float* d_prev, float* d_w_reduce, void* workspace,
                            size_t workspace_bytes, int N, int C, int h, int w, int H, int W, void* stream);
size_t mvs_fmt_smooth_wgrad_workspace_bytes(int N, int C, int H, int W);
mvs_status mvs_fmt_smooth_wgrad(const float* dy, const float* prev, const float* lateral, const float* w_reduce, float* d_w_smooth, void* workspace,
                                size_t workspace_bytes, int N, int C, int h, int w, int H, int W, void* stream);

/* ==== CrossVITDecoder: the ViT feature decoder at d_model 768 =========================================
 * models/module.py:273-364 with the shipped decoder_cfg (Linear attention, 12 heads of 64, ffn, pre-norm, LayerScale).  The residual
 * stream is token-major fp32 [M, 768], M = views x n tokens.  A GEMM's row operand is a PACKED-SPLIT tensor of
 * mvs_vitdec_packed_bytes(rows, channels) bytes: packed[row >> 4][k >> 5][hi|lo][lane = ((k >> 3) & 3) * 16 + (row & 15)][k & 7] bf16,
 * x ~= hi + lo, written by its producer.  Weights are packing.pack_linear_bf16x3; three-term products, fp32 accumulation.
 * mvs_vitdec_rows_fwd: per row [prev_value[0] * prev +] in [-> LayerNorm(mix_w, mix_b, eps 1e-6)] -> x (fp32, nullable), x_packed
 *   (nullable) and xn_packed = packed(LayerNorm(ln_w, ln_b, eps 1e-5)(x)) (nullable).  Row r = (b * in_views + j) * n + t is read at
 *   in + b * in_batch_stride + (in_v0 + j) * in_view_stride + t * in_row_stride (elements of in_dtype, 768 contiguous) and x_packed is
 *   written at row (b * out_V + out_v0 + j) * n + t.  prev_value lives in device memory.
 * mvs_vitdec_linear_fwd: y = epilogue(a W^T), K -> N = 768 -> 768 | 1536 | 3072 or 1536 | 3072 -> 768.  epilogue 0: fp32 [M, N], elu(.) + 1
 *   on columns < elu_cols; 1: fp32 residual + gamma * (. + bias); 2: packed-split GELU(. + bias).  A linear layer's data gradient
 *   dX = dY W is this call on pack_linear_bf16x3(W^T) (1536 -> 768: [k_proj; v_proj]).
 * mvs_vitdec_kv_fwd: kv [NV * n, 1536] fp32 (elu(k) + 1 | v) -> summary [NV][12][KV_h 64 x 64 | ksum_h 64] fp32 from exact fp32
 *   products; per-slab partials in `workspace` (mvs_vitdec_kv_workspace_bytes) added in a fixed order: no atomics.
 * mvs_vitdec_apply_fwd: a = (q . KV_h) / (q . ksum_h + 1e-6), q [NV * n, 768] fp32, view i uses summary[i / kv_div] -> packed-split.
 * mvs_vitdec_conv_fwd: layer 0 = proj (Conv2d 768 -> 256, 3x3, padding 1), 1 / 2 = upsampler0 / 1 (ConvTranspose2d 256 -> 128 / 128 -> 64,
 *   4x4, stride 2, padding 1), BatchNorm folded, SiLU; x packed-split tokens of the [NV, H, W] map; y packed-split tokens of the
 *   output map (planar 0) or planar fp32 [NV, Cout, Ho, Wo] (planar 1).  w_packed = packing.pack_vitdec_conv / pack_vitdec_deconv.   */
size_t mvs_vitdec_packed_bytes(long long rows, int channels);
size_t mvs_vitdec_summary_bytes(int NV);
size_t mvs_vitdec_kv_workspace_bytes(int NV, int n);
mvs_status mvs_vitdec_rows_fwd(const void* in, int in_dtype, long long in_batch_stride, long long in_view_stride, long long in_row_stride, int in_v0,
                               int in_views, const float* prev, const float* prev_value, const float* mix_w, const float* mix_b, float* x,
                               void* x_packed, int out_V, int out_v0, const float* ln_w, const float* ln_b, void* xn_packed, int NV, int n,
                               int channels, void* stream);
mvs_status mvs_vitdec_linear_fwd(const void* a_packed, const void* w_packed, const float* bias, const float* gamma, const float* residual, void* y,
                                 int M, int K, int N, int epilogue, int elu_cols, void* stream);
mvs_status mvs_vitdec_kv_fwd(const float* kv, void* workspace, size_t workspace_bytes, float* summary, int NV, int n, int channels, void* stream);
mvs_status mvs_vitdec_apply_fwd(const float* q, const float* summary, void* a_packed, int NV, int n, int kv_div, int channels, void* stream);
mvs_status mvs_vitdec_conv_fwd(const void* x_packed, const void* w_packed, const float* bias, void* y, int layer, int planar, int NV, int H, int W,
                               void* stream);

/* ---- training of the CrossVITDecoder's blocks ---------------------------------------------------------
 * mvs_vitdec_wgrad: the weight gradient of a linear layer over tokens: dy [M, N] and x [M, K] fp32, token-major and contiguous ->
 *   dw [N, K] = sum_m dy[m, n] x[m, k] fp32 and, when dbias is not null, dbias [N] = sum_m dy[m, n].  N and K multiples of 128
 *   (in use: N = 768 | 1536 | 3072, K = 768 | 3072), any M >= 1.  Three-term split-bf16 products, the operands split while they are
 *   staged, fp32 accumulation.  The tokens are cut into slabs of whole 32-token chunks (enough slabs for 512 workgroups over the
 *   (N / 128) (K / 128) tiles, never more than chunks); every workgroup leaves its partial tile in `workspace`
 *   (mvs_vitdec_wgrad_workspace_bytes = slabs * (N K + N) floats) and a second launch adds the slabs in slab order: no atomics, the
 *   same bits from run to run and on any stream; a launch of one slab writes dw directly.
 * mvs_vitdec_ln_bwd: LayerNorm backward over rows of 768 (one wave per row; mean and rstd recomputed from x): d_y, x [M, 768], w [768],
 *   eps -> d_x [M, 768] = the gradient into x [+ add [M, 768], nullable: the residual branch's gradient] and d_wb [2, 768] = d_w | d_b,
 *   from per-workgroup partials in `workspace` (mvs_vitdec_ln_bwd_workspace_bytes) added in a fixed order: no atomics.
 * mvs_vitdec_pack_fwd: fp32 [M, channels] (768 | 1536 | 3072) -> packed-split rows: a gradient as the row operand of its data-gradient
 *   GEMM.                                                                                                                          */
size_t mvs_vitdec_wgrad_workspace_bytes(long long M, int N, int K);
mvs_status mvs_vitdec_wgrad(const float* dy, const float* x, float* dw, float* dbias, void* workspace, size_t workspace_bytes, long long M, int N,
                            int K, void* stream);
size_t mvs_vitdec_ln_bwd_workspace_bytes(long long M, int channels);
mvs_status mvs_vitdec_ln_bwd(const float* d_y, const float* x, const float* w, float eps, const float* add, float* d_x, float* d_wb, void* workspace,
                             size_t workspace_bytes, long long M, int channels, void* stream);
mvs_status mvs_vitdec_pack_fwd(const float* x, void* x_packed, long long M, int channels, void* stream);

/* ---- training of the CrossVITDecoder's head -----------------------------------------------------------
 * layer 0 = proj (Conv2d 768 -> 256, 3x3, padding 1), 1 / 2 = upsampler0 / 1 (ConvTranspose2d 256 -> 128 / 128 -> 64, 4x4, stride 2,
 * padding 1), each followed by batch-statistics BatchNorm2d and SiLU.  Maps are token-major: row = (view * H + y) * W + x, fp32
 * [rows, C] or packed-split (mvs_vitdec_packed_bytes).  [NV, H, W] is always the layer's INPUT map; a transposed convolution's output
 * has 4 NV H W rows in fine-map order, view * 4 H W + (2 y + py) * 2 W + 2 x + px.  Three-term split-bf16 products, fp32 accumulation,
 * k ascending; no atomics: the same bits from run to run and on any stream.
 * mvs_vitdec_head_conv_fwd: the pre-activation z fp32 [output rows, Cout] = the convolution with raw weights and NO bias (it cancels in
 *   the batch statistics).  w_packed = packing.pack_vitdec_conv / pack_vitdec_deconv of the weight with an identity BatchNorm.
 * mvs_vitdec_head_dgrad: d_x fp32 [NV H W, Cin] from the packed-split d_z of the output map.  Layer 0: the 3x3 window on the flipped,
 *   channel-transposed taps, wt_packed = pack_linear_bf16x3 of [768, 9 x 256]; layers 1 / 2: the 4x4 stride-2 window of the fine map,
 *   input token (y, x) reads (2 y - 1 + ky, 2 x - 1 + kx), wt_packed = pack_linear_bf16x3 of [Cin, 16 Cout], column (4 ky + kx) Cout + co.
 * mvs_vitdec_head_wgrad: d_z fp32 rows of the output map, x fp32 [NV H W, Cin] -> dw fp32; layer 0: [256, 9 x 768], column
 *   (3 ky + kx) 768 + c; layers 1 / 2: [16 Cout, Cin], row (4 ky + kx) Cout + co.  Token slabs as mvs_vitdec_wgrad's, partials in
 *   `workspace` (mvs_vitdec_head_wgrad_workspace_bytes = slabs * rows * columns floats) added in slab order.
 * mvs_vitdec_head_bn_fwd: z fp32 [M, channels] (256 | 128 | 64) -> stats [3, channels] = mean | biased variance | invstd (fp64 sums,
 *   fixed order) and SiLU(gamma xhat + beta) as y fp32 [M, channels] and / or y_packed (both nullable), or as y_planar fp32
 *   [M / pixels_per_view, channels, pixels_per_view] alone.  running_mean / running_var (nullable) take one step of `momentum` with
 *   mean + conv_bias and the unbiased variance, on the device.
 * mvs_vitdec_head_bn_bwd: d_y (fp32 [M, channels], or planar with d_y_planar = 1), z, stats, gamma, beta -> d_z fp32 and / or
 *   d_z_packed (nullable, not both null), d_gb [2, channels] = d_gamma | d_beta.  workspace: mvs_vitdec_head_bn_workspace_bytes.      */
mvs_status mvs_vitdec_head_conv_fwd(const void* x_packed, const void* w_packed, float* z, int layer, int NV, int H, int W, void* stream);
mvs_status mvs_vitdec_head_dgrad(const void* dz_packed, const void* wt_packed, float* d_x, int layer, int NV, int H, int W, void* stream);
size_t mvs_vitdec_head_wgrad_workspace_bytes(int layer, int NV, int H, int W);
mvs_status mvs_vitdec_head_wgrad(const float* d_z, const float* x, float* dw, void* workspace, size_t workspace_bytes, int layer, int NV, int H,
                                 int W, void* stream);
size_t mvs_vitdec_head_bn_workspace_bytes(long long M, int channels);
mvs_status mvs_vitdec_head_bn_fwd(const float* z, const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                                  float* running_mean, float* running_var, float* stats, float* y, void* y_packed, float* y_planar,
                                  void* workspace, size_t workspace_bytes, long long M, int channels, int pixels_per_view, void* stream);
mvs_status mvs_vitdec_head_bn_bwd(const float* d_y, int d_y_planar, const float* z, const float* stats, const float* gamma, const float* beta,
                                  float* d_z, void* d_z_packed, float* d_gb, void* workspace, size_t workspace_bytes, long long M, int channels,
                                  int pixels_per_view, void* stream);

/* ==== DINOv2 ViT-B/14 backbone: forward_interval_features ==============================================
 * models/dino/dinov2.py vit_base(patch_size=14) with the shipped dino_cfg: 14 x 14 patch embedding + interpolated position embedding,
 * pre-norm blocks (LayerNorm eps 1e-6, qkv with bias, softmax attention over the n + 1 tokens of a view with 12 heads of 64, LayerScale,
 * fc1 - GELU (erf) - fc2).  The residual stream is fp32 [NV, npad, 768]: every view padded to npad = n + 1 rounded up to a multiple of
 * 32 rows (row 0 = class token, rows 1 .. n = patches row-major, the rest finite padding that is masked as keys).  Packed-split
 * operands and three-term products as in the decoder above; proj / fc1 / fc2 run on mvs_vitdec_linear_fwd with M = NV * npad.
 * mvs_vit_rows_fwd: mvs_vitdec_rows_fwd with the eps of the ln_w / ln_b LayerNorm as an argument (the ViT's norm1 / norm2: 1e-6).
 * mvs_vit_patches_fwd: image [NV, 3, 14 gh, 14 gw] (fp32 / bf16 / fp16, read in place with its four element strides) -> packed-split
 *   [NV gh gw, 640]: column c * 196 + ky * 14 + kx, columns 588 .. 639 zero.
 * mvs_vit_embed_fwd: x rows 1 .. n = patches W^T + bias + pos[1 + patch] (w_packed = packing.pack_vit_patch_embed, pos fp32 [n + 1, 768] =
 *   the interpolated position table), row 0 = cls_pos (cls_token + pos[0]), rows n + 1 .. npad - 1 = 0.  Two launches.
 * mvs_vit_qkv_fwd: xn W^T + bias (768 -> 2304) -> the attention operands, mvs_vit_qkv_bytes(NV, npad) bytes: per (view, head) q * q_scale
 *   | k as packed-split rows of 64 channels, then v transposed: vt[key >> 5][d >> 4][hi|lo][lane = g * 16 + (d & 15)][e] with
 *   key & 31 = 16 (e >> 2) + 4 g + (e & 3).  q_scale = softmax scale * log2(e).
 * mvs_vit_attention_fwd: softmax(q k^T) v per (view, head) over keys 0 .. ntok - 1 (online softmax in fp32, exp2; no atomics, no split
 *   over the keys: bit-identical run to run) -> packed-split [NV * npad, 768], the row operand of attn.proj.                        */
size_t mvs_vit_qkv_bytes(int NV, int npad);
mvs_status mvs_vit_rows_fwd(const void* in, int in_dtype, long long in_batch_stride, long long in_view_stride, long long in_row_stride, int in_v0,
                            int in_views, const float* prev, const float* prev_value, const float* mix_w, const float* mix_b, float* x,
                            void* x_packed, int out_V, int out_v0, const float* ln_w, const float* ln_b, float ln_eps, void* xn_packed, int NV, int n,
                            int channels, void* stream);
mvs_status mvs_vit_patches_fwd(const void* img, int dtype, long long batch_stride, long long channel_stride, long long row_stride,
                               long long col_stride, void* a_packed, int NV, int gh, int gw, int patch, int in_chans, void* stream);
mvs_status mvs_vit_embed_fwd(const void* a_packed, const void* w_packed, const float* bias, const float* pos, const float* cls_pos, float* x, int NV,
                             int n, int npad, int channels, void* stream);
mvs_status mvs_vit_qkv_fwd(const void* xn_packed, const void* w_packed, const float* bias, void* qkv, int NV, int npad, float q_scale, int channels,
                           void* stream);
mvs_status mvs_vit_attention_fwd(const void* qkv, void* a_packed, int NV, int ntok, int npad, int heads, int head_dim, void* stream);

/* ---- layout helpers for the nn.Module-level API (NCDHW <-> channel-last) -------------------------*/
mvs_status mvs_ncdhw_to_cl(const float* x, float* y_cl, int B, int C, int D, int H, int W, void* stream);
mvs_status mvs_cl_to_ncdhw(const float* x_cl, float* y, int B, int C, int D, int H, int W, void* stream);

/* ==== the network's glue (DINOv2_mvsformer_model.py:72-88) ===============================================
 * mvs_resize_bicubic_fwd: img fp32 [N,C,H,W] read in place with its four element strides -> out contiguous fp32 [N,C,h,w] =
 *   F.interpolate(img, (h, w), mode="bicubic", align_corners=False) without antialiasing: source coordinate (dst + 0.5) * (in / out) - 0.5,
 *   cubic convolution coefficients with A = -0.75, each of the 4 x 4 tap indices clamped to [0, in - 1].  Any scale, any size >= 1.
 * mvs_resize_bilinear_add_fwd: out = base + F.interpolate(x, (h, w), mode="bilinear", align_corners=False); base, out contiguous fp32
 *   [N,C,h,w], x fp32 [N,C,xh,xw] read in place with its strides; source coordinate max(0, (dst + 0.5) * (in / out) - 0.5), the upper
 *   neighbour clamped.  (xh, xw) == (h, w): out = base + x bit for bit.  out may be base.
 * The source coordinate is evaluated as an exact rational (floor + once-rounded fraction), not in fp32.  Sizes <= 32768, N * C <= 65535,
 * strides >= 0.  One launch each, no workspace.                                                                     */
mvs_status mvs_resize_bicubic_fwd(const float* img, long long batch_stride, long long channel_stride, long long row_stride, long long col_stride,
                                  float* out, int N, int C, int H, int W, int h, int w, void* stream);
mvs_status mvs_resize_bilinear_add_fwd(const float* base, const float* x, long long batch_stride, long long channel_stride, long long row_stride,
                                       long long col_stride, float* out, int N, int C, int h, int w, int xh, int xw, void* stream);

/* ==== a scene's depth inference: the two ends of the per-view loop (general_eval.py:112-131, test.py:266-294) ====
 * mvs_image_prepare_fwd: src uint8 RGB [h,w,3] (decoded image) -> planar fp32 [3,H,W] = table[c][resized] AND resized uint8 [H,W,3], where
 *   resized is the 8-bit linear resize of the source with pad_rows replicated rows above and below it (the "tt" edge pad, addressed and never
 *   materialised) to H x W in OpenCV's fixed-point arithmetic: per axis f = (float)((d + 0.5) * (in / out) - 0.5), s = floor(f), f -= s,
 *   clamped to [0, in - 1] with f = 0 at both ends, coefficients short(rint((1 - f) * 2048)) and short(rint(f * 2048)), horizontal
 *   S[s] * a0 + S[s + 1] * a1, vertical (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2; equal sizes give the identity.
 *   table fp32 [3,256]: the caller's ((u / 255) - mean[c]) / std[c] (ToTensor + Normalize).  planar and resized are plain pointers: a slot of
 *   a larger buffer is fine.  Sizes <= 32768, 0 <= pad_rows <= 64.
 * mvs_depth_outputs_pack_fwd: depth, conf (and reg_conf, or NULL) fp32 [H,W] -> staging, 5 H W bytes, 4-byte aligned: fp32 [H,W] the depth
 *   rows bottom-up (a PFM body), then uint8 [H,W] = uint8(c * 255) truncated and clamped to 0..255 with c = conf, or (conf * 3 + reg_conf) / 4
 *   as three separately rounded fp32 operations when reg_conf is given.
 * One launch each, no workspace.                                                                                     */
mvs_status mvs_image_prepare_fwd(const unsigned char* src, int h, int w, int pad_rows, const float* table, float* planar, unsigned char* resized,
                                 int H, int W, void* stream);
mvs_status mvs_depth_outputs_pack_fwd(const float* depth, const float* conf, const float* reg_conf, void* staging, int H, int W, void* stream);

/* ==== the multi-stage depth losses and the validation metrics (models/losses.py, utils.py:156-189) ================
 * All maps are dense planar fp32: logits / hyp [B,D,H,W], depth / gt / mask [B,H,W] (a pixel counts where mask > 0.5), interval [B].  Every
 * reduction leaves one partial per workgroup in the workspace and a one-workgroup launch adds them in a fixed order: no floating-point
 * atomics, bit-identical run to run.  loss fp32 [1] = weight * sum / N and count int32 [1] = N stay on the device; N = 0 gives a NaN loss
 * (a mean over nothing) and an all-zero gradient.  The backward entry points read the incoming gradient grad_loss [1] and N from device
 * memory and write their whole output (no memset, no host synchronisation).  B H W < 2^31.
 * mvs_ce_loss_fwd: per pixel one walk over the depth column (from plane D - 1 down when inverse: the reference's flips are index arithmetic):
 *   log-sum-exp of the logits, iv[j] = |d[j+1] - d[j]| / 2 with the last interval repeated, the bin = count of d[j] + iv[j] <= gt clamped to
 *   D - 1, out of range where gt < d[0] - iv[0] or gt > d[D-1] + iv[D-1].  index int32 [B,H,W] = the target plane in STORED order, -1 where
 *   the pixel is masked out or out of range; lse fp32 [B,H,W].  These 8 bytes per pixel are all the backward needs.  D >= 2.
 * mvs_ce_loss_bwd: grad_logits = (grad_loss * weight / N) * (exp(logit - lse) - [plane == index]) where index >= 0, else 0.
 * mvs_reg_loss_fwd / _bwd: smooth L1 (beta 1) of depth / interval[b] against gt / interval[b] (interval NULL: 1); with hyp != NULL every
 *   pixel's loss is clamped from above by (d_last - d_first) / interval[b], first and last in the walk order, and the gradient passes where
 *   loss <= range (torch.clamp_max).  The backward recomputes the pixel from the inputs: nothing is kept.
 * mvs_depth_metrics: est, gt [B,H,W] fp32, mask fp32 (> 0.5) or bytes (mask_bytes: != 0).  T <= MVS_METRICS_MAX_T thresholds and bands, formed
 *   on the device in fp64 and rounded to fp32: value = base * factor with base = interval ? (double)interval[per_sample ? b : 0] / divisor : 1
 *   and the host arrays thres / band_lo / band_hi [T] of factors; a NaN band_lo means "no band" (every valid pixel).  Per image: counts int32
 *   [B, 1 + 2 T] = valid, T counts of |est - gt| > thres, T counts of lo <= err <= hi; sums fp64 [B,T] of the errors inside the bands; means
 *   fp32 [B + 1, 2 T] = per image T ratios count / valid (no valid pixel: NaN) and T band means (an empty band: 0; no band and no valid
 *   pixel: NaN), row B = the mean over the images.  Two launches.                                                          */
#define MVS_METRICS_MAX_T 8
size_t mvs_loss_workspace_bytes(long long pixels);
mvs_status mvs_ce_loss_fwd(const float* logits, const float* hyp, const float* gt, const float* mask, int inverse, double weight, int* index, float* lse,
                           void* workspace, size_t workspace_bytes, float* loss, int* count, int B, int D, int H, int W, void* stream);
mvs_status mvs_ce_loss_bwd(const float* logits, const int* index, const float* lse, const float* grad_loss, const int* count, double weight,
                           float* grad_logits, int B, int D, int H, int W, void* stream);
mvs_status mvs_reg_loss_fwd(const float* depth, const float* gt, const float* mask, const float* interval, const float* hyp, int inverse, double weight,
                            void* workspace, size_t workspace_bytes, float* loss, int* count, int B, int D, int H, int W, void* stream);
mvs_status mvs_reg_loss_bwd(const float* depth, const float* gt, const float* mask, const float* interval, const float* hyp, int inverse,
                            const float* grad_loss, const int* count, double weight, float* grad_depth, int B, int D, int H, int W, void* stream);
size_t mvs_depth_metrics_workspace_bytes(int B, int H, int W, int T);
mvs_status mvs_depth_metrics(const float* est, const float* gt, const void* mask, int mask_bytes, const float* interval, double divisor, int per_sample,
                             const double* thres, const double* band_lo, const double* band_hi, int T, void* workspace, size_t workspace_bytes,
                             int* counts, double* sums, float* means, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVS_HIP_H */
