"""Training-mode path of one cascade stage.

What is native and what is not, stated plainly:

* the cost-volume construction - homography compose, warp + group-wise correlation + entropy (pass 1), the visibility-weighted
  aggregation (pass 2) AND ITS BACKWARD - runs on the library's HIP kernels: ``WarpCorrAggregate`` is a
  ``torch.autograd.Function`` whose forward is ``mvs_warp_corr_aggregate_fwd`` and whose backward is
  ``mvs_warp_corr_aggregate_bwd`` (gradients w.r.t. reference features, source features and visibility maps; the warped
  [B,C,D,H,W] volumes the reference keeps alive per view for ``grid_sample``'s backward are never materialised);
* the 3-D U-Net regulariser (CostRegNet / CostRegNet3D, nine Conv3d / ConvTranspose3d + BatchNorm3d + ReLU blocks and three skip
  adds) runs on the library's kernels in both directions (``RegNetTrain``): forward convolutions and DATA gradients on the
  split-bf16 MFMA kernels of the inference path with un-folded, re-packed weights (the data gradient of a stride-1 convolution is
  the convolution with flipped, transposed taps; of a strided convolution the transposed convolution; of a transposed convolution
  the strided convolution), WEIGHT gradients on an fp32-MFMA kernel (``mvs_conv3d_wgrad``), batch-statistics BatchNorm + ReLU +
  skip forward and backward on ``mvs_bn_*`` (sums in double, SyncBatchNorm's all-reduce of the sums included); on one rank each
  block is ONE C call per direction (``mvs_train_block_fwd`` / ``_bwd`` chain pack, convolution, statistics, finalize, normalise /
  reduce, apply, weight gradient, pack, data gradient on the stream).  Activations (pre-BatchNorm convolution outputs and
  block outputs) are kept while small and RECOMPUTED in the backward pass above 512 MB, or when ``reg.recompute_in_backward`` says
  so - the reference always runs its regularisers under ``torch.utils.checkpoint`` (module.py:393-396, 488-492);
* the visibility CNN's three Conv2d + BatchNorm2d + ReLU blocks (``VisTrain``: the same kernels on D = 1 volumes, BatchNorm per
  source view like the reference's per-view calls) and CostRegNet's 3x3x3 `prob` (``Prob3Train``) are native as well;
* still PyTorch-ROCm autograd, all of it element-wise or tiny: the visibility CNN's 1x1 Conv2d + sigmoid, CostRegNet3D's 1x1x1 `prob`,
  the softmax / argmax / regression head, the running-statistics momentum update.  There is no second backend in this module: a
  stage the native kernels do not cover (base_ch != 8) raises; a head configured with conv_precision "fp32" (exact contraction at
  inference) trains on the fp32-equivalent split-bf16 kernels and says so once.  The comparator that routes every conv /
  BatchNorm layer through PyTorch-ROCm autograd ops lives with the tests (``tests/train_torch_route.py``; on the MI355X image MIOpen
  picks naive kernels for these 3-D and 2-D convolutions: 400 ms per stage-4 step against 11.8 ms natively).

The reference differentiates neither the sampling grid (built under ``torch.no_grad()``, warping.py:80) nor the entropy
(``sim_vol.detach()``, cost_volume.py:90); this path follows it: no gradient reaches the depth hypotheses, the cameras or - via
the entropy - the features.  The transformer regulariser of the shipped stage 1 (``transformer_forward_torch``): each of its six
blocks is one autograd node (``TransformerBlockTrain``) whose forward is the inference path's five launches and whose backward is
hand-written - the attention core on ``mvs_tr_attention_bwd`` (fp32, no [n, n] tensor), the linears' gradients as plain GEMMs
(rocBLAS), LayerNorm / GELU / residual-scale gradients as tensor expressions, the FFN hidden layer and the pre-LayerNorm sums
recomputed; patch embedding / expansion with their LayerNorm3D and `prob` stay PyTorch-ROCm autograd ops.

The feature side receives the cascade's `d features` in ``fmt_forward_train``, the differentiable form of
``fmt.FMT_with_pathway.forward``: each linear-attention block is one node (``FmtBlockTrain``: forward = the inference launches on weights
packed on the device, backward hand-written like ``TransformerBlockTrain``'s with only the block's input kept), each pathway level one
node (``FmtPathLevelTrain``: forward = the fused inference launch; backward = the forward convolution with flipped taps for the
lateral, ``mvs_fmt_path_bwd`` - the interpolation's exact adjoint as a gather - for the coarse map and the 1x1 weights, and
``mvs_fmt_smooth_wgrad`` on fp32 MFMA for the 3x3 weights, the merged map recomputed in its staging; no atomics).  Its input gradients
go on into ``fpn_decoder_forward_train``, the train-mode FPNDecoder: planar batch-statistics BatchNorm + Swish,
weight gradients on fp32 MFMA, the upsample's adjoint as a gather, the last level fused so that its 64-channel full-resolution map is
never written in either direction.  The FPN encoder trains in ``fpn_encoder_forward_train`` (section 4.19) and the ViT decoder in
``vitdec_forward_train`` (section 4.20: block backward native, head on PyTorch ops or, with ``native_head``, on ``vitdec_head_train``,
section 4.21); the ViT backbone is frozen and has no training form.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, ops, packing


class WarpCorrAggregate(torch.autograd.Function):
    """volume_mean [B,G,D,H,W] = sum_v in_prod_v * vis_v / (sum_v vis_v + 1e-6)   (cost_volume.py:74-101), HIP forward and backward."""

    @staticmethod
    def forward(ctx, features, vis, homography, hyp, G, channel_last=False):
        feats, code = ops._feat(features.detach())
        vis_c = ops._f32c(vis.detach())
        vol_cl, _ = ops.warp_corr_aggregate(feats, code, homography, hyp, vis_c, G, normalise=True)
        ctx.save_for_backward(feats, vis_c, homography, hyp, vol_cl)
        ctx.code, ctx.G, ctx.in_dtype, ctx.channel_last = code, G, features.dtype, bool(channel_last)
        return vol_cl if channel_last else ops.cl_to_ncdhw(vol_cl)

    @staticmethod
    def backward(ctx, grad_volume):
        feats, vis, hom, hyp, vol_cl = ctx.saved_tensors
        gvol_cl = ops._f32c(grad_volume) if ctx.channel_last else ops.ncdhw_to_cl(ops._f32c(grad_volume))
        vis_sum = vis.sum(dim=1).contiguous()
        gfeat, gvis = ops.warp_corr_aggregate_bwd(feats, ctx.code, hom, hyp, vis, vis_sum, vol_cl, gvol_cl, ctx.G)
        return gfeat.to(ctx.in_dtype), gvis, None, None, None, None


# --------------------------------------------------------------------------------------------------
# native training form of the U-Net regulariser
# --------------------------------------------------------------------------------------------------
_PREC = _lib.PRECISIONS["bf16x3"]


def _block_parts(layer):
    """(conv module, BatchNorm module, is_transposed) of one Conv3d / Deconv3d wrapper or CostRegNet3D's Sequential block."""
    if isinstance(layer, nn.Sequential):
        return layer[0], layer[1], True
    return layer.conv, layer.bn, isinstance(layer.conv, nn.ConvTranspose3d)


def _stride3(conv):
    s = conv.stride
    return (s, s, s) if isinstance(s, int) else tuple(s)



def _conv_fwd(a_cl, w, stride, transposed, zero_bias, kd=3, tflip=False):
    """Linear (no bias / BatchNorm / ReLU) Conv3d(k (kd,3,3), 'same' padding, stride) or ConvTranspose3d(k3, stride (sd,2,2)) of a
    channel-last tensor on the split-bf16 MFMA kernels, from the un-folded weight tensor."""
    if transposed:
        return ops.deconv3d_linear(a_cl, ops.pack_deconv_weights_device(w, stride[0]), zero_bias, w.shape[1], stride[0], _PREC)
    if tflip:                                             # the convolution with w's taps reversed and its channel axes exchanged
        wp = ops.pack_conv_weights_device(w, packing.conv_chunk(w.shape[0], stride), tflip=True)
        return ops.conv3d_bn_relu(a_cl, wp, zero_bias, w.shape[1], kd, stride, False, _PREC)
    wp = ops.pack_conv_weights_device(w, packing.conv_chunk(w.shape[1], stride))
    return ops.conv3d_bn_relu(a_cl, wp, zero_bias, w.shape[0], kd, stride, False, _PREC)


def _conv_bwd(a_in, dz, w, stride, transposed, zero_bias, need_da=True):
    """(weight gradient, data gradient) of _conv_fwd.  Data gradients reuse the forward kernels: a transposed convolution's is the
    strided convolution with the same taps, a stride-1 convolution's the convolution with flipped, transposed taps, a strided
    convolution's the transposed convolution with the same taps."""
    if transposed:
        dw = ops.conv3d_wgrad(dz, a_in, stride)
        da = _conv_fwd(dz, w, stride, False, zero_bias) if need_da else None
        return dw, da
    dw = ops.conv3d_wgrad(a_in, dz, stride)
    if not need_da:
        return dw, None
    if stride == (1, 1, 1):
        return dw, _conv_fwd(dz, w, stride, False, zero_bias, tflip=True)
    if any(d % s for d, s in zip(a_in.shape[1:4], stride)):
        raise _lib.MvsHipError("training: strided convolutions need even input sizes (got %s)" % (tuple(a_in.shape[1:4]),))
    return dw, _conv_fwd(dz, w, stride, True, zero_bias)


def _embed_2d(w2d, cin_pad=None):
    """Conv2d weight [Cout, Cin, 3, 3] -> Conv3d weight [Cout, Cin (padded), 3, 3, 3] that acts on D = 1 volumes (only the centre
    depth tap is non-zero; the outer ones meet zero padding anyway)."""
    co, ci = w2d.shape[:2]
    w3 = torch.zeros(co, cin_pad or ci, 3, 3, 3, dtype=torch.float32, device=w2d.device)
    w3[:, :ci, 1] = w2d
    return w3


def _fast_bn(bn) -> bool:
    """The one-call block kernels cover batch-statistics BatchNorm with fp32 running statistics and a fixed momentum on one rank;
    SyncBatchNorm with an initialised process group, eval-mode BatchNorm and cumulative averaging take the granular path."""
    if not bn.training or bn.running_mean is None or bn.momentum is None:
        return False
    if isinstance(bn, nn.SyncBatchNorm) and torch.distributed.is_available() and torch.distributed.is_initialized():
        return False
    return bn.running_mean.dtype == torch.float32 and bn.running_mean.is_contiguous() and bn.running_var.is_contiguous()


class _BnState:
    """Forward statistics of one BatchNorm layer (batch statistics in train mode, running statistics otherwise) and the
    bookkeeping nn.BatchNorm3d / nn.SyncBatchNorm do: momentum update of the running statistics, all-reduce of the sums."""

    def __init__(self, bn, z_cl, groups: int = 1):
        """groups > 1: `groups` equal slices of z_cl along its leading axis are normalised independently (one nn.BatchNorm call each,
        in order, in the reference): statistics come back as [groups, C]."""
        self.groups = groups
        self.batch = bn.training or bn.running_mean is None
        self.sync = False                                  # SyncBatchNorm: the sums are all-reduced over bn.process_group (None = WORLD)
        self.group = None
        C = z_cl.shape[-1]
        n_local = z_cl.numel() // C // groups
        self.count = float(n_local)
        if self.batch:
            sums = ops.bn_stats(z_cl, groups)
            if isinstance(bn, nn.SyncBatchNorm) and torch.distributed.is_available() and torch.distributed.is_initialized():
                self.sync, self.group = True, bn.process_group
                cnt = torch.tensor([float(n_local)], dtype=torch.float64, device=z_cl.device)
                torch.distributed.all_reduce(sums, group=self.group)
                torch.distributed.all_reduce(cnt, group=self.group)
                self.count = float(cnt.item())
            self.bn = bn if (bn.training and bn.running_mean is not None) else None
            if self.bn is not None and bn.running_mean.dtype == torch.float32 and bn.running_mean.is_contiguous() and (groups == 1 or bn.momentum is not None):
                with torch.no_grad():
                    bn.num_batches_tracked += groups
                self.mean, self.var, self.invstd = ops.bn_finalize(sums, self.count, bn.eps, bn.running_mean, bn.running_var, self._momentum())
            else:
                self.mean, self.var, self.invstd = ops.bn_finalize(sums, self.count, bn.eps)
                self.update_running_stats()
        else:
            self.bn = None
            self.mean = bn.running_mean.detach().float().contiguous()
            self.invstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps).contiguous()
            if groups > 1:
                self.mean, self.invstd = self.mean.expand(groups, -1).contiguous(), self.invstd.expand(groups, -1).contiguous()

    def update_running_stats(self):
        """One momentum step of nn.BatchNorm's running statistics (unbiased variance).  Called once in the forward and once more
        in the backward: the reference runs its regulariser under torch.utils.checkpoint (module.py:393-396), whose recomputation
        in the backward pass is a second train-mode forward - its running statistics take two steps per iteration."""
        bn = self.bn
        if bn is None:
            return
        with torch.no_grad():
            if bn.running_mean.dtype == torch.float32 and bn.running_mean.is_contiguous() and (self.groups == 1 or bn.momentum is not None):
                bn.num_batches_tracked += self.groups
                ops.bn_running_update(self.mean, self.var, self.count, self._momentum(), bn.running_mean, bn.running_var)
                return
            means = self.mean.reshape(self.groups, -1)
            vars_ = self.var.reshape(self.groups, -1)
            for gi in range(self.groups):                    # one momentum step per group, in order (cumulative average: m = 1 / n)
                bn.num_batches_tracked += 1
                m = self._momentum()
                bn.running_mean.mul_(1.0 - m).add_(means[gi].to(bn.running_mean.dtype), alpha=m)
                bn.running_var.mul_(1.0 - m).add_((vars_[gi] * (self.count / max(self.count - 1.0, 1.0))).to(bn.running_var.dtype), alpha=m)

    def _momentum(self) -> float:
        bn = self.bn
        return float(bn.momentum) if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)


class RegNetTrain(torch.autograd.Function):
    """features_cl [B,D,H,W,8] = U-Net(volume_cl) up to (not including) `prob`, module.py:398-406 / 494-501, with gradients for the
    volume and all 27 parameters (nine weights, nine BatchNorm weights, nine BatchNorm biases) - see the module docstring."""

    NAMES = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11")
    SKIP = {6: 3, 7: 1, 8: -1}                       # block index -> index of the block whose output is added (-1: the input volume)

    # Activations: kept by default while they are small, RECOMPUTED in the backward pass above `RECOMPUTE_ABOVE_BYTES` - the
    # reference always runs its regularisers under torch.utils.checkpoint (module.py:393-396, 488-492: only the input volume survives
    # the forward, the backward re-runs forward_once).  `reg.recompute_in_backward = True / False` overrides the size rule.  In
    # recompute mode the forward saves the input volume, the parameters and each BatchNorm's batch statistics ([C] vectors); the
    # backward re-runs convolution + normalise with THOSE statistics (the kernels are deterministic: the regenerated activations are
    # bit-identical, so are the gradients) - one extra U-Net forward without the statistics passes.
    RECOMPUTE_ABOVE_BYTES = 512 << 20

    @staticmethod
    def kept_bytes(reg, shape) -> int:
        """Bytes of the activations the keep-everything mode holds between forward and backward: every block's pre-BatchNorm output z
        and every block's output y except the last (which is the result)."""
        B, D, H, W = shape[:4]
        dims, total = {0: (D, H, W)}, 0
        for i, name in enumerate(RegNetTrain.NAMES):
            conv, _, transposed = _block_parts(getattr(reg, name))
            d, h, w = dims[i]
            dims[i + 1] = ops._out_dims(transposed, 3, _stride3(conv), d, h, w)
            od, oh, ow = dims[i + 1]
            total += (2 if i + 1 < len(RegNetTrain.NAMES) else 1) * 4 * B * od * oh * ow * conv.out_channels
        return total

    @staticmethod
    def _wants_recompute(reg, shape) -> bool:
        flag = getattr(reg, "recompute_in_backward", None)
        return bool(flag) if flag is not None else RegNetTrain.kept_bytes(reg, shape) > RegNetTrain.RECOMPUTE_ABOVE_BYTES

    @staticmethod
    def forward(ctx, volume_cl, reg, *params):
        x = ops._f32c(volume_cl.detach())
        wsp = ops.TrainWorkspace(x.device)
        zero_bias = wsp.zero_bias
        recompute = RegNetTrain._wants_recompute(reg, x.shape)
        skip_sources = {k + 1 for k in RegNetTrain.SKIP.values()}              # activation indices a later block adds
        last_use = {k + 1: i for i, k in RegNetTrain.SKIP.items()}
        blocks, acts, saved = [], {0: x}, []
        n = len(RegNetTrain.NAMES)
        for i, name in enumerate(RegNetTrain.NAMES):
            conv, bn, transposed = _block_parts(getattr(reg, name))
            w = params[3 * i].detach().float()
            gamma, beta = params[3 * i + 1].detach().float().contiguous(), params[3 * i + 2].detach().float().contiguous()
            stride = _stride3(conv)
            a_in = acts[i]
            skip_idx = RegNetTrain.SKIP.get(i)
            skip = None if skip_idx is None else acts[skip_idx + 1]
            if _fast_bn(bn):
                with torch.no_grad():
                    bn.num_batches_tracked += 1
                z, stats, y = ops.train_block_fwd(wsp, a_in, w, transposed, 3, stride, gamma, beta, bn.eps, bn.running_mean, bn.running_var,
                                                  bn.momentum, skip)
                acts[i + 1] = y
                blocks.append((transposed, stride, True, 0.0, (False, None), bn))
                saved += ([stats, stats, w, gamma, beta] if recompute else [a_in, z, stats, stats, w, gamma, beta])
            else:
                z = _conv_fwd(a_in, w, stride, transposed, zero_bias)
                st = _BnState(bn, z)
                acts[i + 1] = ops.bn_relu_apply(z, st.mean, st.invstd, gamma, beta, skip, relu=True)
                blocks.append((transposed, stride, st.batch, st.count, (st.sync, st.group), st))
                saved += ([st.mean, st.invstd, w, gamma, beta] if recompute else [a_in, z, st.mean, st.invstd, w, gamma, beta])
            if recompute:                                # drop what no later block reads: the forward's live set stays a few tensors
                del z, a_in
                for k in [k for k in acts if k <= i and k != 0 and not (k in skip_sources and last_use[k] > i)]:
                    del acts[k]
        ctx.blocks, ctx.recompute = blocks, recompute
        ctx.save_for_backward(*(([x] if recompute else []) + saved))
        return acts[n]

    @staticmethod
    def _regenerate(S, blocks, zero_bias):
        """Recompute mode: the forward again from the saved input volume with the saved batch statistics -> the (a_in, z, ...) rows the
        backward reads.  Statistics rows: one-call blocks saved [3, 1, C] (mean, var, invstd), granular blocks mean and invstd."""
        acts, rows = {0: S[0]}, []
        for i, (transposed, stride, _, _, _, bn_state) in enumerate(blocks):
            s0, s1, w, gamma, beta = S[1 + 5 * i: 6 + 5 * i]
            mean, invstd = (s0, s1) if isinstance(bn_state, _BnState) else (s0[0].contiguous(), s0[2].contiguous())
            skip_idx = RegNetTrain.SKIP.get(i)
            skip = None if skip_idx is None else acts[skip_idx + 1]
            z = _conv_fwd(acts[i], w, stride, transposed, zero_bias)
            acts[i + 1] = ops.bn_relu_apply(z, mean, invstd, gamma, beta, skip, relu=True)
            rows += [acts[i], z, s0, s1, w, gamma, beta]
        return rows

    @staticmethod
    def backward(ctx, grad_out):
        S = ctx.saved_tensors
        n = len(ctx.blocks)
        grads = [None] * (3 * n)
        pending = {}                                     # activation index (0 = volume, i + 1 = output of block i) -> gradient so far
        pending[n] = ops._f32c(grad_out)
        wsp = ops.TrainWorkspace(grad_out.device)
        zero_bias = wsp.zero_bias
        if ctx.recompute:
            S = RegNetTrain._regenerate(S, ctx.blocks, zero_bias)
        for i in range(n - 1, -1, -1):
            transposed, stride, batch, count, group, bn_state = ctx.blocks[i]
            a_in, z, mean, invstd, w, gamma, beta = S[7 * i:7 * i + 7]
            g = pending.pop(i + 1)
            skip_idx = RegNetTrain.SKIP.get(i)
            if skip_idx is not None:                     # the skip source receives the block output's gradient unchanged
                k = skip_idx + 1
                pending[k] = g if k not in pending else pending[k] + g
            if not isinstance(bn_state, _BnState):       # one-call block: bn_state is the BatchNorm module, `mean` the [3, 1, C] statistics
                bn = bn_state
                with torch.no_grad():
                    bn.num_batches_tracked += 1          # the reference's checkpoint recomputation: a second momentum step (in the call)
                grads[3 * i], grads[3 * i + 1], grads[3 * i + 2], da = ops.train_block_bwd(
                    wsp, g, a_in, z, mean, w, transposed, 3, stride, gamma, beta, bn.running_mean, bn.running_var, bn.momentum)
                pending[i] = da if i not in pending else pending[i] + da
            else:
                bn_state.update_running_stats()          # the reference's checkpoint recomputation (see _BnState)
                sums = ops.bn_relu_bwd_reduce(g, z, mean, invstd, gamma, beta, relu=True)
                grads[3 * i + 2] = sums[: sums.numel() // 2].float()                 # d beta (this rank's voxels; DDP averages)
                grads[3 * i + 1] = sums[sums.numel() // 2:].float()                  # d gamma
                if group[0]:
                    sums = sums.clone()
                    torch.distributed.all_reduce(sums, group=group[1])
                dz = ops.bn_relu_bwd_apply(g, z, mean, invstd, gamma, beta, sums, count, relu=True, use_batch_stats=batch)
                grads[3 * i], da = _conv_bwd(a_in, dz, w, stride, transposed, zero_bias)
                pending[i] = da if i not in pending else pending[i] + da
            if ctx.recompute:
                S[7 * i] = S[7 * i + 1] = None           # this block's regenerated activations are done with
        return (pending[0], None) + tuple(grads)


def regnet_forward_native(reg, volume_cl: torch.Tensor) -> torch.Tensor:
    """CostRegNet / CostRegNet3D up to `prob` on the library's kernels, channel-last in and out."""
    if not isinstance(reg.inner, nn.Identity):
        raise NotImplementedError("in_channels != base_channels (1x1x1 `inner` conv): inference only (shape-generic kernel); no training kernels")
    params = []
    for name in RegNetTrain.NAMES:
        conv, bn, _ = _block_parts(getattr(reg, name))
        if bn is None or conv.bias is not None:
            raise NotImplementedError("the training path implements the bias-free conv + BatchNorm + ReLU blocks of the regularisers")
        params += [conv.weight, bn.weight, bn.bias]
    return RegNetTrain.apply(volume_cl, reg, *params)


class VisTrain(torch.autograd.Function):
    """The three Conv2d + BatchNorm2d + ReLU blocks of the visibility CNN (cost_volume.py:36, module.py:168-197) on the library's
    kernels: entropy [B, V-1, H, W] (no gradient: it comes from sim.detach()) -> features [V-1, B, H, W, 8] channel-last, with
    gradients for the nine parameters.  The 2-D layers run as k = (1|3,3,3) convolutions on D = 1 volumes; the reference calls the
    CNN once per source view on a batch of B maps, so the BatchNorm statistics (and running-stat updates) are per view here too."""

    @staticmethod
    def forward(ctx, entropy, vis_seq, *params):
        B, NV, H, W = entropy.shape
        dev = entropy.device
        zero_bias = torch.zeros(64, dtype=torch.float32, device=dev)
        x = torch.zeros(NV, B, H, W, 8, dtype=torch.float32, device=dev)         # view-major, 8 channels: the MFMA kernels' smallest Cin
        x[..., 0] = entropy.detach().float().permute(1, 0, 2, 3)
        a = x.view(NV * B, 1, H, W, 8)
        saved, blocks = [], []
        for i in range(3):
            w2d = params[3 * i].detach().float()
            gamma, beta = params[3 * i + 1].detach().float().contiguous(), params[3 * i + 2].detach().float().contiguous()
            w3 = _embed_2d(w2d, 8 if i == 0 else None)
            if w3.shape[0] == 8:                                                 # the 16 -> 8 layer: the kernels have its k = (1,3,3) form
                z = _conv_fwd(a, w3[:, :, 1:2].contiguous(), (1, 1, 1), False, zero_bias, kd=1)
            else:
                z = _conv_fwd(a, w3, (1, 1, 1), False, zero_bias)
            st = _BnState(vis_seq[i].bn, z, groups=NV)                            # one statistics set per source view
            mean, invstd = (st.mean, st.invstd) if NV > 1 else (st.mean.reshape(1, -1), st.invstd.reshape(1, -1))
            y = ops.bn_relu_apply(z, mean, invstd, gamma, beta, None, relu=True)
            blocks.append((st.batch, st.count, (st.sync, st.group)))
            saved += [mean, invstd]
            saved += [a, z, w3, gamma, beta]
            a = y
        ctx.blocks, ctx.B, ctx.NV = blocks, B, NV
        ctx.save_for_backward(*saved)
        return a.view(NV, B, H, W, 8)

    @staticmethod
    def backward(ctx, grad_out):
        S = ctx.saved_tensors
        B, NV = ctx.B, ctx.NV
        g = ops._f32c(grad_out).view(NV * B, 1, *grad_out.shape[2:])
        zero_bias = torch.zeros(64, dtype=torch.float32, device=g.device)
        grads = [None] * 9
        for i in (2, 1, 0):
            mean, invstd, a_in, z, w3, gamma, beta = S[7 * i:7 * i + 7]
            C = z.shape[-1]
            batch, count, group = ctx.blocks[i]
            sums = ops.bn_relu_bwd_reduce(g, z, mean, invstd, gamma, beta, relu=True)             # [NV, 2C]
            grads[3 * i + 2], grads[3 * i + 1] = sums[:, :C].sum(0).float(), sums[:, C:].sum(0).float()
            if group[0]:
                sums = sums.clone()
                torch.distributed.all_reduce(sums, group=group[1])
            dz = ops.bn_relu_bwd_apply(g, z, mean, invstd, gamma, beta, sums, count, relu=True, use_batch_stats=batch)
            # weight gradient on the k = (1,3,3) form of the kernel (the maps are D = 1 volumes); data gradient = the convolution with
            # flipped, transposed taps (nothing to propagate below the first layer: the entropy carries no gradient)
            dw2 = ops.conv3d_wgrad(a_in, dz, (1, 1, 1), kd=1)
            cin = 1 if i == 0 else w3.shape[1]
            grads[3 * i] = dw2[:, :cin, 0].contiguous()
            g = _conv_fwd(dz, w3, (1, 1, 1), False, zero_bias, tflip=True) if i > 0 else None
        return (None, None) + tuple(grads)


class Prob3Train(torch.autograd.Function):
    """CostRegNet's `prob` = Conv3d(8, 1, 3, padding 1, bias=False) (module.py:391,407): features_cl [B,D,H,W,8] -> logits [B,D,H,W].
    Forward on the MFMA head kernel; the gradients reuse the 8 <-> 16 channel kernels with the single logit channel zero-padded."""

    @staticmethod
    def forward(ctx, feat_cl, weight):
        f = ops._f32c(feat_cl.detach())
        w = weight.detach().float()
        w16 = torch.zeros(16, 8, 3, 3, 3, dtype=torch.float32, device=f.device)
        w16[0] = w[0]
        zero_bias = torch.zeros(64, dtype=torch.float32, device=f.device)
        ctx.save_for_backward(f, w)
        return ops.conv3d_logits(f, ops.pack_conv_weights_device(w16, 8), zero_bias, _PREC)

    @staticmethod
    def backward(ctx, grad_logits):
        f, w = ctx.saved_tensors
        g = ops._f32c(grad_logits)
        zero_bias = torch.zeros(64, dtype=torch.float32, device=g.device)
        g8 = torch.zeros(*g.shape, 8, dtype=torch.float32, device=g.device)
        g8[..., 0] = g
        dw = ops.conv3d_wgrad(f, g8, (1, 1, 1))[0:1].contiguous()                 # [1, 8, 3, 3, 3]
        wt = torch.zeros(16, 8, 3, 3, 3, dtype=torch.float32, device=g.device)   # rows = feature channels, column 0 = the logit channel
        wt[:8, 0] = w[0].flip(1, 2, 3)
        df = _conv_fwd(g8, wt, (1, 1, 1), False, zero_bias)[..., :8].contiguous()
        return df, dw


def vis_forward_native(vis_seq, entropy: torch.Tensor) -> torch.Tensor:
    """self.vis per source view (cost_volume.py:93) -> [B, V-1, H, W]; conv / BatchNorm / ReLU blocks native, the 1x1 conv + sigmoid
    as elementwise autograd ops."""
    params = []
    for i in range(3):
        params += [vis_seq[i].conv.weight, vis_seq[i].bn.weight, vis_seq[i].bn.bias]
    t = VisTrain.apply(entropy, vis_seq, *params)                                 # [V-1, B, H, W, 8]
    last = vis_seq[3]
    v = (t * last.weight.reshape(1, 1, 1, 1, -1)).sum(-1)
    if last.bias is not None:
        v = v + last.bias
    return torch.sigmoid(v).permute(1, 0, 2, 3)


def _position_encoding_3d(position3d: torch.Tensor, C: int, rescale: float = 4.0) -> torch.Tensor:
    """PositionEncoding3D (position_encoding.py:166-189): per axis C channels, sin on the even and cos on the odd ones of
    position * rescale * 10000^(-2i/C) -> [B, 3C, D, H, W].  No gradient: the positions come from the hypotheses."""
    import math
    B, _, D, H, W = position3d.shape
    freq = torch.exp(torch.arange(0, C, 2, device=position3d.device, dtype=torch.float32) * (-math.log(10000.0) / C)).view(1, 1, -1, 1)
    ang = position3d.reshape(B, 3, 1, D * H * W).float() * rescale * freq                           # [B, 3, C/2, N]
    pe = torch.stack([torch.sin(ang), torch.cos(ang)], dim=3)                                      # [B, 3, C/2, 2, N]: interleaved
    return pe.reshape(B, 3 * C, D, H, W)


def _layer_norm_channels(x: torch.Tensor, ln) -> torch.Tensor:
    """LayerNorm3D (module.py:586-599): normalise an NCDHW tensor over its channel axis."""
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    return ln.weight.view(1, -1, 1, 1, 1) * (xc * torch.rsqrt(xc.pow(2).mean(1, keepdim=True) + ln.eps)) + ln.bias.view(1, -1, 1, 1, 1)


class AttentionTrain(torch.autograd.Function):
    """a [B,n,64] = proj-less attention of one block: softmax(scale q k^T) v over all tokens, q | k | v = t W_qkv^T (no bias,
    attention.py:76-101, 141-170).  Forward = the inference kernels (mvs_tr_qkv_fwd + mvs_tr_attention_fwd: split-bf16 operands,
    flash attention on the MFMA k axis); backward = the library's attention backward (mvs_tr_attention_bwd: fp32, two launches, no
    atomics) between two plain GEMMs - q | k | v are re-projected from the saved tokens (nothing [n, n]-sized or per-key is kept
    between forward and backward), d_t = d_qkv W_qkv, d_W = d_qkv^T t."""

    @staticmethod
    def forward(ctx, t, w_qkv, heads, scale):
        tt = ops._f32c(t.detach())
        w = w_qkv.detach().float()
        a = ops.tr_attention(tt, packing.pack_linear_bf16x3(w), heads, scale, _lib.PREC_BF16X3)   # packed on the weight's device (torch ops)
        ctx.save_for_backward(tt, w, a)
        ctx.heads, ctx.scale = heads, scale
        return a

    @staticmethod
    def backward(ctx, d_a):
        t, w, a = ctx.saved_tensors
        B, n, C = t.shape
        qkv = (t.reshape(B * n, C) @ w.t()).reshape(B, n, 3 * C)                   # [.., (q | k | v), heads, 16]
        d_qkv = ops.tr_attention_bwd(qkv, a, ops._f32c(d_a), ctx.heads, ctx.scale)
        d2 = d_qkv.reshape(B * n, 3 * C)
        return (d2 @ w).reshape(B, n, C), d2.t() @ t.reshape(B * n, C), None, None


def _gelu_bwd(pre):
    """d gelu(pre) / d pre of the erf form: Phi(pre) + pre phi(pre)."""
    return 0.5 * (1.0 + torch.erf(pre * 0.7071067811865476)) + pre * torch.exp(-0.5 * pre * pre) * 0.3989422804014327


def _layer_norm_bwd(d_y, u, w, eps):
    """Backward of y = LayerNorm(u) over the last axis (weight w): -> (d_u, d_w, d_b)."""
    mu = u.mean(-1, keepdim=True)
    xc = u - mu
    rstd = torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    dxh = d_y * w
    d_u = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
    red = tuple(range(d_y.dim() - 1))
    return d_u, (d_y * xh).sum(red), d_y.sum(red)


class TransformerBlockTrain(torch.autograd.Function):
    """One post-norm block (module.py:535-583: t1 = LN1(t + g1 proj(attn(t))), t2 = LN2(t1 + g2 W2 gelu(W1 t1))) with a hand-written
    backward.  Forward = the five launches of the inference path (qkv + flash attention, proj + residual + LayerNorm, linear1 + GELU,
    linear2 + residual + LayerNorm on the split-bf16 kernels); kept for the backward: the block input, the attention output and t1 -
    the 4x wider FFN hidden layer and both pre-LayerNorm sums are recomputed.  Backward: the attention core on
    ``mvs_tr_attention_bwd``; the linears' data / weight gradients are plain GEMMs (rocBLAS through torch.mm), LayerNorm / GELU /
    residual-scale gradients element-wise tensor expressions - no autograd graph, no [n, n] tensor."""

    @staticmethod
    def forward(ctx, t, heads, scale, w_qkv, w_proj, b_proj, g1, n1w, n1b, eps1, w1, b1, w2, b2, g2, n2w, n2b, eps2):
        f = lambda p: p.detach().float().contiguous()
        pk = lambda w: packing.pack_linear_bf16x3(f(w))
        prec = _lib.PREC_BF16X3
        t0 = ops._f32c(t.detach())
        a = ops.tr_attention(t0, pk(w_qkv), heads, scale, prec)
        t1 = ops.tr_linear(a, pk(w_proj), f(b_proj), _lib.TR_EPI_RES_LN, 64, prec, residual=t0, gamma=f(g1).reshape(1), ln_w=f(n1w), ln_b=f(n1b), ln_eps=eps1)
        hdn = ops.tr_linear(t1, pk(w1), f(b1), _lib.TR_EPI_GELU, w1.shape[0], prec)
        t2 = ops.tr_linear(hdn, pk(w2), f(b2), _lib.TR_EPI_RES_LN, 64, prec, residual=t1, gamma=f(g2).reshape(1), ln_w=f(n2w), ln_b=f(n2b), ln_eps=eps2)
        ctx.save_for_backward(t0, a, t1, f(w_qkv), f(w_proj), f(b_proj), f(g1), f(n1w), f(w1), f(b1), f(w2), f(b2), f(g2), f(n2w))
        ctx.heads, ctx.scale, ctx.eps = heads, scale, (eps1, eps2)
        return t2

    @staticmethod
    def backward(ctx, d_t2):
        t0, a, t1, w_qkv, w_proj, b_proj, g1, n1w, w1, b1, w2, b2, g2, n2w = ctx.saved_tensors
        B, n, C = t0.shape
        flat = lambda x: x.reshape(B * n, -1)
        d_t2 = ops._f32c(d_t2)
        # ---- FFN half: recompute pre-GELU, hidden, the scaled branch and the pre-LayerNorm sum
        pre = flat(t1) @ w1.t() + b1
        hdn = F.gelu(pre)
        y2 = hdn @ w2.t() + b2
        d_u2, d_n2w, d_n2b = _layer_norm_bwd(flat(d_t2), flat(t1) + g2 * y2, n2w, ctx.eps[1])
        d_g2 = (d_u2 * y2).sum()
        d_y2 = g2 * d_u2
        d_w2, d_b2 = d_y2.t() @ hdn, d_y2.sum(0)
        d_pre = (d_y2 @ w2) * _gelu_bwd(pre)
        d_w1, d_b1 = d_pre.t() @ flat(t1), d_pre.sum(0)
        d_t1 = d_u2 + d_pre @ w1
        # ---- attention half
        yp = flat(a) @ w_proj.t() + b_proj
        d_u1, d_n1w, d_n1b = _layer_norm_bwd(d_t1, flat(t0) + g1 * yp, n1w, ctx.eps[0])
        d_g1 = (d_u1 * yp).sum()
        d_yp = g1 * d_u1
        d_wp, d_bp = d_yp.t() @ flat(a), d_yp.sum(0)
        d_a = (d_yp @ w_proj).reshape(B, n, C)
        qkv = (flat(t0) @ w_qkv.t()).reshape(B, n, 3 * C)
        d_qkv = flat(ops.tr_attention_bwd(qkv, a, d_a, ctx.heads, ctx.scale))
        d_t0 = (d_u1 + d_qkv @ w_qkv).reshape(B, n, C)
        d_wqkv = d_qkv.t() @ flat(t0)
        return (d_t0, None, None, d_wqkv, d_wp, d_bp, d_g1.reshape(g1.shape), d_n1w, d_n1b, None, d_w1, d_b1, d_w2, d_b2, d_g2.reshape(g2.shape),
                d_n2w, d_n2b, None)


def transformer_forward_torch(reg, x: torch.Tensor, position3d) -> torch.Tensor:
    """PureTransformerCostReg.forward (module.py:629-646, blocks :569-581, attention dino/layers/attention.py:76-101,141-170), the
    training form of the shipped stage 1: every transformer block runs forward on the inference path's kernels and backward through
    the hand-written ``TransformerBlockTrain`` (attention backward on the library's kernel, linears as plain GEMMs, LayerNorm / GELU
    gradients as tensor expressions); the two ends - position-encoding projection + patch embedding + LayerNorm3D, and patch
    expansion + LayerNorm3D + `prob` - are PyTorch-ROCm autograd ops on the module's own parameters."""
    import math
    if reg.training and (reg.drop or reg.attn_drop):
        raise NotImplementedError("dropout inside the transformer regulariser (drop / attn_drop != 0) is not used by the shipped config")
    if position3d is not None:
        x = x + reg.pe_proj(_position_encoding_3d(position3d, x.shape[1]))
    x = _layer_norm_channels(reg.down[0](x), reg.down[1])
    B, C, d, h, w = x.shape
    heads = reg.num_heads
    t = x.permute(0, 3, 4, 2, 1).reshape(B, h * w * d, C)                                          # tokens ordered (h w d), module.py:573
    N = t.shape[1]
    scale = (C // heads) ** -0.5
    if reg.softmax_scale == "entropy_invariance":
        scale *= math.log(N, reg.train_avg_length)
    for blk in reg.attention_layers:
        if C == 64 and heads == 4 and blk.attn.proj.bias is not None and blk.ffn.linear1.bias is not None and blk.ffn.linear2.bias is not None:
            t = TransformerBlockTrain.apply(t, heads, scale, blk.attn.qkv.weight, blk.attn.proj.weight, blk.attn.proj.bias, blk.gamma1,
                                            blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, blk.ffn.linear1.weight, blk.ffn.linear1.bias,
                                            blk.ffn.linear2.weight, blk.ffn.linear2.bias, blk.gamma2, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
            continue
        a = AttentionTrain.apply(t, blk.attn.qkv.weight, heads, scale)               # bias-free variants: attention core native, the rest autograd ops
        proj, l1, l2 = blk.attn.proj, blk.ffn.linear1, blk.ffn.linear2
        t = blk.norm1(t + blk.gamma1 * proj(a))
        t = blk.norm2(t + blk.gamma2 * l2(F.gelu(l1(t))))
    x = t.reshape(B, h, w, d, C).permute(0, 4, 3, 1, 2)
    return reg.prob(_layer_norm_channels(reg.up[0](x), reg.up[1]))


# --------------------------------------------------------------------------------------------------
# FMT_with_pathway (fmt.py): the feature-side module the cascade's `d features` flow into
# --------------------------------------------------------------------------------------------------
FMT_BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight", "attn.proj.weight",
                    "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                    "mlp.fc2.bias", "ls2.gamma")


def _tokens(x: torch.Tensor) -> torch.Tensor:
    """planar [N, 64, ...] -> token-major [N n, 64]"""
    return x.reshape(x.shape[0], 64, -1).transpose(1, 2).reshape(-1, 64)


def _elu1_bwd(d_out, out):
    """Backward of out = elu(pre) + 1: the derivative is 1 where out > 1 and exp(pre) = out elsewhere (out = 1 exactly: both give 1)."""
    return d_out * torch.where(out > 1, torch.ones_like(out), out)


def _linattn_fwd(qh, KV, ks):
    """Linear-attention core: qh [B, l, H, d], KV = sum_s k_s (x) v_s [B, H, d, m], ks = sum_s k_s [B, H, d] -> (Z, num, a = num Z)."""
    Z = 1.0 / (torch.einsum("blhd,bhd->blh", qh, ks) + 1e-6)
    num = torch.einsum("blhd,bhdm->blhm", qh, KV)
    return Z, num, num * Z.unsqueeze(-1)


def _linattn_bwd(d_a, qh, kh, vh, KV, ks, Z, num):
    """Adjoint of _linattn_fwd and of the summaries KV, ks of kh, vh [B, s, H, .]: (d_q, d_k, d_v) on heads."""
    d_num = d_a * Z.unsqueeze(-1)
    d_den = -(d_a * num).sum(-1) * Z * Z
    d_q = torch.einsum("blhm,bhdm->blhd", d_num, KV) + d_den.unsqueeze(-1) * ks.unsqueeze(1)
    d_KV = torch.einsum("blhd,blhm->bhdm", qh, d_num)
    d_ks = torch.einsum("blhd,blh->bhd", qh, d_den)
    d_k = torch.einsum("bhdm,bshm->bshd", d_KV, vh) + d_ks.unsqueeze(1)
    d_v = torch.einsum("bshd,bhdm->bshm", kh, d_KV)
    return d_q, d_k, d_v


class FmtBlockTrain(torch.autograd.Function):
    """One pre-norm CrossBlock with linear attention (fmt.py, tests/fmt_ref.py::block) over N views: x [N,64,h,w] (+ the position table
    on the first block) -> the same shape.  ref = None: self attention.  ref [N / kv_div, 64, h, w]: cross attention, view i reads the
    summary of ref[i // kv_div] through this block's own norm1.  Forward = the inference path's launches (fmt_kv + fmt_block) on weights
    packed on the device from the live parameters, so the outputs are the inference bits.  Kept for the backward: x and ref.  The
    backward recomputes everything else in fp32 and is hand-written: the linears' gradients are plain GEMMs, LayerNorm / elu / GELU /
    LayerScale / residual and the linear-attention core (KV_h = sum_s k_s (x) v_s, Z = 1 / (q . sum_s k_s + 1e-6), a = q KV Z) tensor
    expressions - no autograd graph.  A cross layer's gradient into ref is the sum over the kv_div views that share it."""

    @staticmethod
    def forward(ctx, x, ref, pe, kv_div, *params):
        P = [p.detach().float() for p in params]
        wp, vec = packing.pack_fmt_block(dict(zip(FMT_BLOCK_PARAMS, P)), device=None)
        x0 = ops._f32c(x.detach())
        kvt = None if ref is None else ops._f32c(ref.detach())
        kv = ops.fmt_kv(x0, wp, vec, pe) if kvt is None else ops.fmt_kv(kvt, wp, vec)
        y = ops.fmt_block(x0, kv, wp, vec, pe, kv_div=kv_div)
        ctx.save_for_backward(x0, kvt, pe, *P)
        ctx.kv_div = kv_div
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        x0p, refp, pe = ctx.saved_tensors[:3]
        n1w, n1b, wq, wk, wv, wp, bp, g1, n2w, n2b, w1, b1, w2, b2, g2 = ctx.saved_tensors[3:]
        N, kv_div, eps = x0p.shape[0], ctx.kv_div, 1e-5
        n = x0p[0, 0].numel()
        Nr = N // kv_div
        ln = lambda u, w, b: F.layer_norm(u, (64,), w, b, eps)
        heads = lambda t, views: t.reshape(Nr, views * n, 4, 16)
        x0 = _tokens(x0p if pe is None else x0p.reshape(N, 64, n) + pe)
        dy = _tokens(ops._f32c(d_y))
        # ---- recompute the forward: attention half (q from the block's tokens, k / v from its own or the reference view's)
        xn = ln(x0, n1w, n1b)
        reft = None if refp is None else _tokens(refp)
        kvn = xn if reft is None else ln(reft, n1w, n1b)
        qp, kp, v = xn @ wq.t(), kvn @ wk.t(), kvn @ wv.t()
        q, k = F.elu(qp) + 1, F.elu(kp) + 1
        qh, kh, vh = heads(q, kv_div), heads(k, 1), heads(v, 1)
        KV = torch.einsum("bshd,bshm->bhdm", kh, vh)
        ks = kh.sum(1)
        Z, num, a = _linattn_fwd(qh, KV, ks)
        a = a.reshape(-1, 64)
        yp = a @ wp.t() + bp
        x1 = x0 + g1 * yp
        # ---- FFN half, forward and backward
        u = ln(x1, n2w, n2b)
        pre = u @ w1.t() + b1
        hdn = F.gelu(pre)
        y2 = hdn @ w2.t() + b2
        d_g2, d_y2 = (dy * y2).sum(0), dy * g2
        d_w2, d_b2 = d_y2.t() @ hdn, d_y2.sum(0)
        d_pre = (d_y2 @ w2) * _gelu_bwd(pre)
        d_w1, d_b1 = d_pre.t() @ u, d_pre.sum(0)
        d_x1n, d_n2w, d_n2b = _layer_norm_bwd(d_pre @ w1, x1, n2w, eps)
        d_x1 = dy + d_x1n
        # ---- attention half
        d_g1, d_yp = (d_x1 * yp).sum(0), d_x1 * g1
        d_wp, d_bp = d_yp.t() @ a, d_yp.sum(0)
        d_q, d_k, d_v = _linattn_bwd(heads(d_yp @ wp, kv_div), qh, kh, vh, KV, ks, Z, num)
        d_v = d_v.reshape(-1, 64)
        d_qp, d_kp = _elu1_bwd(d_q.reshape(-1, 64), q), _elu1_bwd(d_k.reshape(-1, 64), k)
        d_wq, d_wk, d_wv = d_qp.t() @ xn, d_kp.t() @ kvn, d_v.t() @ kvn
        d_xn, d_kvn = d_qp @ wq, d_kp @ wk + d_v @ wv
        d_ref = None
        if reft is None:
            d_x0n, d_n1w, d_n1b = _layer_norm_bwd(d_xn + d_kvn, x0, n1w, eps)
        else:
            d_x0n, d_n1w, d_n1b = _layer_norm_bwd(d_xn, x0, n1w, eps)
            d_reft, d_n1w_kv, d_n1b_kv = _layer_norm_bwd(d_kvn, reft, n1w, eps)
            d_n1w, d_n1b = d_n1w + d_n1w_kv, d_n1b + d_n1b_kv
            d_ref = d_reft.reshape(Nr, n, 64).transpose(1, 2).reshape(refp.shape)
        d_x = (d_x1 + d_x0n).reshape(N, n, 64).transpose(1, 2).reshape(x0p.shape)
        return (d_x, d_ref, None, None, d_n1w, d_n1b, d_wq, d_wk, d_wv, d_wp, d_bp, d_g1, d_n2w, d_n2b, d_w1, d_b1, d_w2, d_b2, d_g2)


class FmtPathLevelTrain(torch.autograd.Function):
    """One pathway level Y = S * (U(W_r prev) + lat) for all views (fmt.py, tests/fmt_ref.py::level).  Forward = the fused inference
    launch (the merged map is never written); kept: prev and lat, which the neighbouring nodes hold anyway.  Backward: d lat = dM on
    the forward convolution with flipped, channel-transposed taps; d prev and d W_r on mvs_fmt_path_bwd (the interpolation's exact
    adjoint as a gather); d S on mvs_fmt_smooth_wgrad, which recomputes the merged map in its staging.  No atomics: bit-identical
    from run to run."""

    @staticmethod
    def forward(ctx, prev, lat, w_reduce, w_smooth):
        p, l = ops._f32c(prev.detach()), ops._f32c(lat.detach())
        wr = w_reduce.detach().float().reshape(w_reduce.shape[0], -1).contiguous()
        ws = w_smooth.detach().float()
        ctx.save_for_backward(p, l, wr, ws)
        ctx.wr_shape = w_reduce.shape
        return ops.fmt_path(p, l, wr, packing.pack_fpn_conv_weights(ws, 1))

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        p, l, wr, ws = ctx.saved_tensors
        d_y = ops._f32c(d_y)
        d_m = ops.fmt_smooth(d_y, packing.pack_fpn_conv_weights(ws.flip(2, 3).transpose(0, 1), 1))
        d_prev, d_wr = ops.fmt_path_bwd(d_m, p, wr)
        return d_prev, d_m, d_wr.reshape(ctx.wr_shape), ops.fmt_smooth_wgrad(d_y, p, l, wr)


def fmt_forward_train(module, features: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """FMT_with_pathway.forward with autograd: `module` is an fmt.FMT_with_pathway (train or eval mode; it has no BatchNorm and no
    dropout, so both compute the same), `features` its stage1..stage4 dictionary of [B, V, 64 | 32 | 16 | 8, ., .] tensors -> the
    same dictionary of fp32 [B, V, C, H, W] outputs, bit for bit the inference forward's.  One autograd node per launch group
    (``FmtBlockTrain`` per block and view group, ``FmtPathLevelTrain`` per level), joined by indexing and `cat`.  Gradients reach every
    input that requires grad, in that input's dtype (fp16 / bf16 inputs are widened once), and the module's 66 parameters.  No double
    backward."""
    ts, B, V = module._shapes(features)
    net = module.FMT
    names = net.layer_names
    f1 = ts[0].float()
    h, w = f1.shape[-2:]
    pe = net.position_encoding(h, w, f1.device)
    params = [[blk.get_parameter(k) for k in FMT_BLOCK_PARAMS] for blk in net.layers]
    # reference view: the self layers only; the tokens after each are the cross layers' keys / values
    x, refs, first = f1[:, 0], [], pe
    for i, name in enumerate(names):
        if name == "self":
            x = FmtBlockTrain.apply(x, None, first, 1, *params[i])
            first = None
            refs.append(x)
    views = [x.unsqueeze(1)]
    if V > 1:
        # every source view of the batch in one node per layer: view b * (V - 1) + j attends to reference view b
        x, first = f1[:, 1:].reshape(B * (V - 1), 64, h, w), pe
        for i, name in enumerate(names):
            if name == "self":
                x = FmtBlockTrain.apply(x, None, first, 1, *params[i])
            else:
                x = FmtBlockTrain.apply(x, refs[i] if len(refs) == len(names) else refs[i // 2], first, V - 1, *params[i])
            first = None
        views.append(x.reshape(B, V - 1, 64, h, w))
    out1 = torch.cat(views, 1)
    outs = {"stage1": out1}
    prev = out1.reshape(B * V, 64, h, w)
    for k in (1, 2, 3):
        lat = ts[k].float()
        prev = FmtPathLevelTrain.apply(prev, lat.reshape((B * V,) + tuple(lat.shape[2:])), getattr(module, "dim_reduction_%d" % k).weight,
                                       getattr(module, "smooth_%d" % k).weight)
        outs["stage%d" % (k + 1)] = prev.reshape((B, V) + tuple(prev.shape[1:]))
    return outs


# --------------------------------------------------------------------------------------------------
# FPNDecoder (features.py): where fmt_forward_train's input gradients go
# --------------------------------------------------------------------------------------------------
def _require_single_process(what):
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise NotImplementedError("%s: batch statistics are per process; SyncBatchNorm / multi-GPU training of the feature side is not built"
                                  % what)


def _bn_train_step(bn, what):
    """One train-mode BatchNorm2d call of module `what`: checks the running buffers, num_batches_tracked + 1 -> (mean, var, momentum)."""
    rm, rv = bn.running_mean, bn.running_var
    if rm is None:
        return None, None, 0.0
    if rm.dtype != torch.float32 or not rm.is_contiguous() or not rv.is_contiguous():
        raise NotImplementedError("%s training: BatchNorm running statistics must be contiguous fp32 buffers" % what)
    with torch.no_grad():
        bn.num_batches_tracked += 1
    return rm, rv, float(bn.momentum) if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)


def _fpn_bn_swish(z, bn, conv_bias, gamma, beta):
    """Train-mode BatchNorm2d + Swish of the pre-activation z = conv(x) WITHOUT its bias: batch statistics (the bias cancels in
    z - mean), one momentum step of the running statistics with mean + bias and the unbiased variance, num_batches_tracked + 1."""
    rm, rv, momentum = _bn_train_step(bn, "FPNDecoder")
    return ops.fpn_bn_swish_fwd(z, gamma, beta, bn.eps, conv_bias if rm is not None else None, rm, rv, momentum)


def _vec32(p):
    return p.detach().float().contiguous()


class FpnHeadTrain(torch.autograd.Function):
    """out_k = Swish(BatchNorm2d(Conv2d(64, C_k, 1 | 3)(x) + b)) in train mode for k = 0, 1, 2 (module.py:246-252).  Forward: the inference
    convolution on the un-folded weights, then the planar batch-statistics BatchNorm + Swish.  Kept: x (which the neighbouring merge node
    holds anyway), the pre-activation z (C_k channels) and the statistics.  Backward: mvs_fpn_bn_swish_bwd, the weight gradient on fp32
    MFMA, the data gradient on the forward convolution with flipped, channel-transposed taps.  The conv bias sits in front of a
    batch-statistics BatchNorm: its gradient is exactly zero and is returned as zeros."""

    @staticmethod
    def forward(ctx, x, bn, w, b, gamma, beta):
        x0, w32, g, bt = ops._f32c(x.detach()), w.detach().float(), _vec32(gamma), _vec32(beta)
        k = w32.shape[2]
        z = ops.fpn_conv(x0, packing.pack_fpn_conv_weights(w32, 1), None, w32.shape[0], k, 1, ops.FPN_ACT_NONE)
        y, stats = _fpn_bn_swish(z, bn, _vec32(b), g, bt)
        ctx.save_for_backward(x0, z, stats, w32, g, bt)
        ctx.b_like = (b.shape, b.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        x0, z, stats, w32, g, bt = ctx.saved_tensors
        d_z, d_g, d_b = ops.fpn_bn_swish_bwd(d_y, z, stats, g, bt)
        d_w = ops.fpn_wgrad(d_z, x0, w32.shape[2])
        d_x = ops.fpn_train_conv(d_z, w32.flip(2, 3).transpose(0, 1).contiguous()) if ctx.needs_input_grad[0] else None
        return d_x, None, d_w, torch.zeros(ctx.b_like[0], dtype=ctx.b_like[1], device=d_z.device), d_g, d_b


class FpnMergeTrain(torch.autograd.Function):
    """intra_k = up2(prev) + inner_k(lat) for k = 1, 2 (module.py:262-266): the inference launch forward; kept: lat.  Backward: d prev on
    mvs_fpn_up2_adjoint (the upsample's exact adjoint as a gather), d lat = W_inner^T d intra as a 1x1 convolution, d W_inner | d b_inner
    in one fp32-MFMA weight-gradient launch (the bias is its column of ones)."""

    @staticmethod
    def forward(ctx, prev, lat, wi, bi):
        l = ops._f32c(lat.detach())
        wi2 = wi.detach().float().reshape(wi.shape[0], -1).contiguous()
        ctx.save_for_backward(l, wi2)
        ctx.wi_shape = wi.shape
        return ops.fpn_merge(ops._f32c(prev.detach()), l, wi2, _vec32(bi))

    @staticmethod
    @once_differentiable
    def backward(ctx, d_intra):
        l, wi2 = ctx.saved_tensors
        d = ops._f32c(d_intra)
        clat = l.shape[1]
        d_prev = ops.fpn_up2_adjoint(d) if ctx.needs_input_grad[0] else None
        d_lat = ops.fpn_train_conv(d, wi2.t().reshape(clat, 64, 1, 1).contiguous()) if ctx.needs_input_grad[1] else None
        d_wb = ops.fpn_wgrad(d, l, 1, ones=True).reshape(64, clat + 1)
        return d_prev, d_lat, d_wb[:, :clat].reshape(ctx.wi_shape), d_wb[:, clat].contiguous()


class FpnLevel3Train(torch.autograd.Function):
    """out3 = Swish(BatchNorm2d(Conv2d(64, 8, 3)(up2(prev) + inner3(lat)) + b)) in train mode, merge and head in one node (module.py:267-268).
    Neither the 64-channel full-resolution intra3 nor its gradient ever exists as a whole tensor.  Forward: the fused inference launch
    (intra3 evaluated in the convolution's staging) -> z [N,8,H,W], then BatchNorm + Swish.  Backward, with dz from mvs_fpn_bn_swish_bwd:
      d W_out3   mvs_fpn_merge_wgrad, intra3 re-evaluated in its staging;
      d lat      = W_inner^T conv^T(dz): a 1x1 after a 3x3 composes exactly, borders included -> ONE 8 -> 8 3x3 convolution of dz;
      d W_inner, d b_inner = sum_p d intra3 (x) [lat | 1] = the contraction of W_out3 with the 8 x 9 x 3 x 3 correlation of dz with [lat | 1]
                 (one small weight-gradient launch; the contraction is a 64 x 9 x 72 product);
      d prev     = up2^T(conv^T(dz)), one view at a time: the view's d intra3 slab (conv^T, 8 -> 64) is gathered into d prev and reused."""

    @staticmethod
    def forward(ctx, prev, lat, bn, wi, bi, w, b, gamma, beta):
        p, l = ops._f32c(prev.detach()), ops._f32c(lat.detach())
        wi2, bi1 = wi.detach().float().reshape(64, 8).contiguous(), _vec32(bi)
        w32, g, bt = w.detach().float(), _vec32(gamma), _vec32(beta)
        z = ops.fpn_merge_conv(p, l, wi2, bi1, packing.pack_fpn_conv_weights(w32, 1), None, 8, ops.FPN_ACT_NONE)
        y, stats = _fpn_bn_swish(z, bn, _vec32(b), g, bt)
        ctx.save_for_backward(p, l, z, stats, wi2, bi1, w32, g, bt)
        ctx.like = (wi.shape, b.shape, b.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        p, l, z, stats, wi2, bi1, w32, g, bt = ctx.saved_tensors
        d_z, d_g, d_b = ops.fpn_bn_swish_bwd(d_y, z, stats, g, bt)
        d_w = ops.fpn_merge_wgrad(d_z, p, l, wi2, bi1)
        corr = ops.fpn_wgrad(d_z, l, 3, ones=True).double()                                # [8, 8 + 1, 3, 3]
        w64 = w32.double()
        d_wi = torch.einsum("cokl,cikl->oi", w64, corr[:, :8]).float().reshape(ctx.like[0])
        d_bi = torch.einsum("cokl,ckl->o", w64, corr[:, 8]).float()
        wd = w32.flip(2, 3).transpose(0, 1).contiguous()                                   # conv^T: dz (8) -> d intra3 (64)
        d_lat = None
        if ctx.needs_input_grad[1]:
            d_lat = ops.fpn_train_conv(d_z, torch.einsum("oi,ockl->ickl", wi2.double(), wd.double()).float().contiguous())
        d_prev = None
        if ctx.needs_input_grad[0]:
            d_prev = torch.empty_like(p)
            slab = torch.empty((1, 64) + tuple(l.shape[2:]), dtype=torch.float32, device=l.device)
            for n in range(l.shape[0]):
                ops.fpn_up2_adjoint(ops.fpn_train_conv(d_z[n:n + 1], wd, out=slab), out=d_prev[n:n + 1])
        return (d_prev, d_lat, None, d_wi, d_bi, d_w, torch.zeros(ctx.like[1], dtype=ctx.like[2], device=d_z.device), d_g, d_b)


def fpn_decoder_forward_train(module, conv01, conv11, conv21, conv31):
    """FPNDecoder.forward in train mode with autograd: `module` is a features.FPNDecoder (feat_chs [8, 16, 32, 64]), the inputs the
    encoder's [N, 8 | 16 | 32 | 64, ...] maps -> [out0, out1, out2, out3], fp32 contiguous [N, 64 | 32 | 16 | 8, ...].  nn.BatchNorm2d's
    train-mode semantics: every head normalises with the batch mean and biased variance of its channels over all N H W samples (the
    reference's training branch calls the decoder once on [B V, ...]), the running statistics take one momentum step (unbiased variance;
    running_mean includes the conv bias although the kernels drop it where it cancels) and num_batches_tracked grows by one.  One autograd
    node per head (``FpnHeadTrain``), per merge (``FpnMergeTrain``) and one for the fused last level (``FpnLevel3Train``).  Gradients
    reach every input that requires grad, in that input's dtype (fp16 / bf16 inputs are widened once), and all 22 parameters; the four
    ``out_k.0.bias`` sit in front of a batch-statistics BatchNorm, so their true gradient is exactly zero and an exact zero tensor is
    returned for them.  No double backward.  Single process only: with torch.distributed initialised on more than one rank this
    raises (SyncBatchNorm on the feature side is not built)."""
    _require_single_process("fpn_decoder_forward_train")
    module._check_inputs(conv01, conv11, conv21, conv31)
    c01, c11, c21, c31 = (t.float() for t in (conv01, conv11, conv21, conv31))
    head = lambda k, x: FpnHeadTrain.apply(x, getattr(module, "out%d" % k)[1], getattr(module, "out%d" % k)[0].weight,
                                           getattr(module, "out%d" % k)[0].bias, getattr(module, "out%d" % k)[1].weight,
                                           getattr(module, "out%d" % k)[1].bias)
    out0 = head(0, c31)
    intra1 = FpnMergeTrain.apply(c31, c21, module.inner1.weight, module.inner1.bias)
    out1 = head(1, intra1)
    intra2 = FpnMergeTrain.apply(intra1, c11, module.inner2.weight, module.inner2.bias)
    out2 = head(2, intra2)
    out3 = FpnLevel3Train.apply(intra2, c01, module.out3[1], module.inner3.weight, module.inner3.bias, module.out3[0].weight,
                                module.out3[0].bias, module.out3[1].weight, module.out3[1].bias)
    return [out0, out1, out2, out3]


# --------------------------------------------------------------------------------------------------
# FPNEncoder (features.py): where fpn_decoder_forward_train's input gradients go
# --------------------------------------------------------------------------------------------------
class FpnEncBlockTrain(torch.autograd.Function):
    """One encoder block leaky_relu(BatchNorm2d(Conv2d(no bias)(x)), 0.1) in train mode (module.py:47-86).  Forward: the inference
    convolution on the un-folded weights -> z, then the planar batch-statistics BatchNorm + LeakyReLU.  Kept: x, z, the statistics, the
    weight, gamma and beta.  Backward: mvs_fpn_bn_leaky_bwd (u recomputed from z and the statistics), the weight gradient on fp32 MFMA, and
    the data gradient - the forward convolution on flipped, channel-transposed taps at stride 1, four parity classes of 3x3 convolutions at
    stride 2 - unless the input needs none (conv00: the image)."""

    @staticmethod
    def forward(ctx, x, bn, w, gamma, beta, stride):
        x0, w32, g, bt = ops._f32c(x.detach()), w.detach().float().contiguous(), _vec32(gamma), _vec32(beta)
        k = w32.shape[2]
        z = ops.fpn_conv(x0, packing.pack_fpn_conv_weights(w32, stride), None, w32.shape[0], k, stride, ops.FPN_ACT_NONE)
        rm, rv, momentum = _bn_train_step(bn, "FPNEncoder")
        y, stats = ops.fpn_bn_leaky_fwd(z, g, bt, bn.eps, rm, rv, momentum)
        ctx.save_for_backward(x0, z, stats, w32, g, bt)
        ctx.stride = stride
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        x0, z, stats, w32, g, bt = ctx.saved_tensors
        d_z, d_g, d_b = ops.fpn_bn_leaky_bwd(d_y, z, stats, g, bt)
        d_w = ops.fpn_enc_wgrad(d_z, x0, w32.shape[2], ctx.stride)
        d_x = ops.fpn_enc_dgrad(d_z, w32, ctx.stride) if ctx.needs_input_grad[0] else None
        return d_x, None, d_w, d_g, d_b, None


def fpn_encoder_forward_train(module, x):
    """FPNEncoder.forward in train mode with autograd: `module` is a features.FPNEncoder (feat_chs [8, 16, 32, 64], norm_type "BN"), x the
    images [N, 3, H, W] with H and W multiples of 8 -> [conv01, conv11, conv21, conv31], fp32 contiguous.  nn.BatchNorm2d's train-mode
    semantics in each of the 11 blocks: the batch mean and biased variance per channel over all N H W samples of the call (the reference's
    training branch calls the encoder once on [B V, 3, H, W]), one momentum step of the running statistics with the unbiased variance,
    num_batches_tracked + 1.  One autograd node per block (``FpnEncBlockTrain``): an output consumed several times (conv01 by downsample1
    and by the decoder) has its gradients summed by autograd.  Gradients reach all 33 parameters.  The image's gradient is not built: an x
    that requires grad raises; bf16 / fp16 images are widened once.  No double backward.  Single process only: with torch.distributed
    initialised on more than one rank this raises (SyncBatchNorm on the feature side is not built)."""
    _require_single_process("fpn_encoder_forward_train")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("FPNEncoder takes images [N, 3, H, W]; got %s" % (tuple(x.shape),))
    H, W = x.shape[-2:]
    if H % 8 or W % 8:
        raise ValueError("the native FPNEncoder needs H and W multiples of 8; got %d x %d" % (H, W))
    if x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("fpn_encoder_forward_train: the image's gradient is not built (conv00's data gradient is never computed); "
                                  "pass an image that does not require grad")
    outs, t = {}, x.detach().float()
    for name, _, stride in module.LAYERS:
        blk = getattr(module, name)
        t = FpnEncBlockTrain.apply(t, blk.bn, blk.conv.weight, blk.bn.weight, blk.bn.bias, stride)
        outs[name] = t
    return [outs["conv01"], outs["conv11"], outs["conv21"], outs["conv31"]]


# --------------------------------------------------------------------------------------------------
# CrossVITDecoder (vit_decoder.py): the ViT feature decoder whose output is added to the FPN's conv31
# --------------------------------------------------------------------------------------------------
VITDEC_BLOCK_PARAMS = FMT_BLOCK_PARAMS          # a CrossBlock's 15 parameters, the same names at d_model 768


def _vitdec_block_launches(pb, x0, r0, kv_div, n):
    """CrossVITDecoder.block on tokens x0 [NVq n, 768] with the keys / values of r0 [NVkv n, 768] (None: self attention on norm1(x0))."""
    from .vit_decoder import CrossVITDecoder
    NVq = x0.shape[0] // n
    xn = ops.vitdec_rows(x0.view(1, NVq, n, 768), 0, NVq, ln=(pb["norm1.weight"], pb["norm1.bias"]), want_x=False)[2]
    if r0 is None:
        return CrossVITDecoder.block(pb, x0, xn, xn, NVq, NVq, n, 1)
    NVkv = r0.shape[0] // n
    keys = ops.vitdec_rows(r0.view(1, NVkv, n, 768), 0, NVkv, want_x=False, want_packed=True)[1]
    return CrossVITDecoder.block(pb, x0, xn, keys, NVq, NVkv, n, kv_div)


class VitdecBlockTrain(torch.autograd.Function):
    """One pre-norm CrossBlock of the ViT decoder (vit_decoder.py, tests/vit_decoder_ref.py::block) on tokens x fp32 [N, n, 768].
    ref = None: self attention, keys and values from norm1(x).  ref [N / kv_div, n, 768]: cross attention, view i reads the summary of
    ref[i // kv_div] UN-normalised (pre_norm_query).  Forward = CrossVITDecoder.block's own launches on weights packed on the device from
    the live parameters: the inference bits.  Kept for the backward: x and ref.  The backward packs W and W^T again, recomputes the
    forward (every GEMM on mvs_vitdec_linear_fwd, pre-activations from epilogue 0), and is hand-written: every linear layer's weight
    gradient on mvs_vitdec_wgrad, every data gradient on mvs_vitdec_linear_fwd with the transposed weight, both LayerNorms on
    mvs_vitdec_ln_bwd (the residual branch's gradient added in the same pass); elu + 1, GELU, LayerScale and the linear-attention core's
    adjoints are fp32 tensor expressions.  d_ref is summed over the kv_div views that share a reference.  No double backward."""

    @staticmethod
    def forward(ctx, x, ref, kv_div, *params):
        P = [p.detach() for p in params]
        pb = packing.pack_vitdec_block_train(dict(zip(VITDEC_BLOCK_PARAMS, P)), transposed=False)
        N, n = x.shape[:2]
        x0 = ops._f32c(x.detach()).reshape(N * n, 768)
        r0 = None if ref is None else ops._f32c(ref.detach()).reshape(-1, 768)
        y = _vitdec_block_launches(pb, x0, r0, kv_div, n)
        ctx.save_for_backward(x0, r0, *P)
        ctx.kv_div, ctx.n = kv_div, n
        return y.view(N, n, 768)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        x0, r0 = ctx.saved_tensors[:2]
        pb = packing.pack_vitdec_block_train(dict(zip(VITDEC_BLOCK_PARAMS, ctx.saved_tensors[2:])))
        n1w, n1b, bp, g1, n2w, n2b, b1, b2, g2 = (pb[k] for k in packing.VITDEC_VECTORS)
        n, kv_div, eps, F32 = ctx.n, ctx.kv_div, 1e-5, ops.VITDEC_EPI_F32
        M = x0.shape[0]
        NVq = M // n
        dy = ops._f32c(d_y).reshape(M, 768)
        ln = lambda t, w, b: F.layer_norm(t, (768,), w, b, eps)
        # ---- recompute the forward: attention half
        xn = ln(x0, n1w, n1b)
        xn_p = ops.vitdec_rows(x0.view(1, NVq, n, 768), 0, NVq, ln=(n1w, n1b), want_x=False)[2]
        kvn, kv_p = (xn, xn_p) if r0 is None else (r0, ops.vitdec_pack(r0))
        Mk = kvn.shape[0]
        Nr = Mk // n
        heads = lambda t, views: t.reshape(Nr, views * n, 12, 64)
        q = ops.vitdec_linear(xn_p, M, pb["q"], 768, 768, F32, elu_cols=768)
        kv = ops.vitdec_linear(kv_p, Mk, pb["kv"], 768, 1536, F32, elu_cols=768)
        k, v = kv[:, :768], kv[:, 768:]
        qh, kh, vh = heads(q, kv_div), heads(k, 1), heads(v, 1)
        summary = ops.vitdec_kv(kv, Nr, n)
        KV, ks = summary[:, :, :4096].reshape(Nr, 12, 64, 64), summary[:, :, 4096:]
        Z, num, a = _linattn_fwd(qh, KV, ks)
        a = a.reshape(M, 768)
        yp = ops.vitdec_linear(ops.vitdec_pack(a), M, pb["proj"], 768, 768, F32, bias=bp)
        x1 = x0 + g1 * yp
        # ---- FFN half, forward and backward
        u = ln(x1, n2w, n2b)
        u_p = ops.vitdec_rows(x1.view(1, NVq, n, 768), 0, NVq, ln=(n2w, n2b), want_x=False)[2]
        pre = ops.vitdec_linear(u_p, M, pb["fc1"], 768, 3072, F32, bias=b1)
        hdn = F.gelu(pre)
        y2 = ops.vitdec_linear(ops.vitdec_pack(hdn), M, pb["fc2"], 3072, 768, F32, bias=b2)
        d_g2, d_y2 = (dy * y2).sum(0), dy * g2
        d_w2, d_b2 = ops.vitdec_wgrad(d_y2, hdn, want_bias=True)
        d_pre = ops.vitdec_dgrad(d_y2, pb["fc2T"], 3072) * _gelu_bwd(pre)
        d_w1, d_b1 = ops.vitdec_wgrad(d_pre, u, want_bias=True)
        d_x1, d_n2w, d_n2b = ops.vitdec_ln_bwd(ops.vitdec_dgrad(d_pre, pb["fc1T"], 768), x1, n2w, eps, add=dy)
        # ---- attention half
        d_g1, d_yp = (d_x1 * yp).sum(0), d_x1 * g1
        d_wp, d_bp = ops.vitdec_wgrad(d_yp, a, want_bias=True)
        d_q, d_k, d_v = _linattn_bwd(heads(ops.vitdec_dgrad(d_yp, pb["projT"], 768), kv_div), qh, kh, vh, KV, ks, Z, num)
        d_qp = _elu1_bwd(d_q.reshape(M, 768), q)
        d_kpv = torch.cat([_elu1_bwd(d_k.reshape(Mk, 768), k), d_v.reshape(Mk, 768)], 1)
        d_wq = ops.vitdec_wgrad(d_qp, xn)
        d_wkv = ops.vitdec_wgrad(d_kpv, kvn.contiguous())
        # the data gradients into norm1: always needed for d_norm1 (and d_x) on the query side; on the key side only where the keys are
        # norm1(x) (self attention) or the reference needs a gradient (level 0's is the frozen backbone's output)
        d_xn, d_ref = ops.vitdec_dgrad(d_qp, pb["qT"], 768), None
        if r0 is None:
            d_xn = d_xn + ops.vitdec_dgrad(d_kpv, pb["kvT"], 768)
        elif ctx.needs_input_grad[1]:
            d_ref = ops.vitdec_dgrad(d_kpv, pb["kvT"], 768).view(Nr, n, 768)
        d_x, d_n1w, d_n1b = ops.vitdec_ln_bwd(d_xn, x0, n1w, eps, add=d_x1)
        return (d_x.view(NVq, n, 768), d_ref, None, d_n1w, d_n1b, d_wq, d_wkv[:768], d_wkv[768:], d_wp, d_bp, d_g1, d_n2w, d_n2b, d_w1, d_b1,
                d_w2, d_b2, d_g2)


class VitdecMixTrain(torch.autograd.Function):
    """The AAS step norm_layers[i - 1](prev_values[i - 1] * prev + x_i) (module.py:349-352): prev fp32 [N, n, 768], x_i the level's ViT
    feature [B, views, n, 768] (N = B views; fp32 / bf16 / fp16, read in place with its strides) -> [N, n, 768].  Forward = the row kernel.
    Backward: mvs_vitdec_ln_bwd on the recomputed mix for d_mix_w, d_mix_b and the mix's gradient, then d_prev = prev_value * that and
    d_prev_value = <that, prev>.  x_i (the frozen backbone's output) gets no gradient."""

    @staticmethod
    def forward(ctx, prev, x_i, prev_value, mix_w, mix_b):
        N, n = prev.shape[:2]
        p0 = ops._f32c(prev.detach()).reshape(N * n, 768)
        pv, w, b = prev_value.detach().float().reshape(1), _vec32(mix_w), _vec32(mix_b)
        y = ops.vitdec_rows(x_i, 0, x_i.shape[1], prev=p0, prev_value=pv, mix=(w, b))[0]
        ctx.save_for_backward(p0, x_i, pv, w)
        ctx.pv_shape = prev_value.shape
        return y.view(N, n, 768)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        p0, x_i, pv, w = ctx.saved_tensors
        s = pv * p0 + x_i.float().reshape(p0.shape)
        d_s, d_w, d_b = ops.vitdec_ln_bwd(ops._f32c(d_y).reshape(p0.shape), s, w, 1e-6)
        return (pv * d_s).view(d_y.shape), None, (d_s * p0).sum().reshape(ctx.pv_shape), d_w, d_b


def vitdec_forward_train(module, x, vit_shape):
    """CrossVITDecoder.forward in train mode with autograd: `module` is a vit_decoder.CrossVITDecoder, x the three [B, V, h w, 768] ViT
    interval features (fp32 / bf16 / fp16, read in place with their strides), vit_shape = [B, V, h, w, 768] -> fp32 [B V, 64, 4 h, 4 w].
    The reference views run the two self blocks, all B (V - 1) source views one node per cross level (``VitdecBlockTrain``), the AAS
    steps are ``VitdecMixTrain`` nodes; ref_feat_list[i] collects its gradient from the next self block, the cross block of level i and,
    for the last level, the output tokens - autograd sums them, as it sums the gradients of prev_values / norm_layers, which the
    reference path and the source path share.  The head (proj, upsampler0, upsampler1) runs on the module's own nn.Sequential layers in
    train mode: PyTorch ops with batch-statistics BatchNorm over all B V views, exactly what the reference runs; with
    ``module.native_head`` it runs on the library's kernels instead (``vitdec_head_train``).  The backbone is frozen (the reference runs it under torch.no_grad()): an input that requires grad raises.
    V = 1 runs no cross block, so their parameters get no gradient.  No double backward.  Single process only: with torch.distributed
    initialised on more than one rank this raises (the BatchNorm statistics are per process)."""
    _require_single_process("vitdec_forward_train")
    B, V, h, w = module._check_shapes(x, None, vit_shape)
    if torch.is_grad_enabled() and any(t.requires_grad for t in x):
        raise NotImplementedError("vitdec_forward_train: the gradient into the ViT features is not built (the DINOv2 backbone is frozen and "
                                  "runs under torch.no_grad()); pass inputs that do not require grad")
    n = h * w
    xs = [module._rows_input(t.detach()) for t in x]
    params = lambda blk: [blk.get_parameter(k) for k in VITDEC_BLOCK_PARAMS]
    mix = lambda i: (module.prev_values[i - 1], module.norm_layers[i - 1].weight, module.norm_layers[i - 1].bias)
    cur = xs[0][:, 0].float()
    refs = [cur]                                                      # ref_feat_list: the cross blocks' keys / values
    for i in range(1, len(module.cross_attn_blocks)):
        y = VitdecBlockTrain.apply(cur, None, 1, *params(module.self_attn_blocks[i - 1]))
        cur = VitdecMixTrain.apply(y, xs[i][:, :1], *mix(i))
        refs.append(cur)
    views = [cur.unsqueeze(1)]
    if V > 1:
        # every source view of the batch in one node per level: view b (V - 1) + j attends to reference view b
        S, y = V - 1, None
        for i, blk in enumerate(module.cross_attn_blocks):
            q = xs[0][:, 1:].float().reshape(B * S, n, 768) if i == 0 else VitdecMixTrain.apply(y, xs[i][:, 1:], *mix(i))
            y = VitdecBlockTrain.apply(q, refs[i], S, *params(blk))
        views.append(y.reshape(B, S, n, 768))
    tokens = torch.cat(views, 1)
    if getattr(module, "native_head", False):
        return vitdec_head_train(module, tokens.reshape(B * V * n, 768), B * V, h, w)     # token-major through the head: no permute
    return module.upsampler1(module.upsampler0(module.proj(tokens.reshape(B * V, h, w, 768).permute(0, 3, 1, 2))))


class VitdecHeadLayerTrain(torch.autograd.Function):
    """One layer of the CrossVITDecoder's head in train mode (module.py:316-321): SiLU(BatchNorm2d(conv(x) + b))
    with batch statistics, conv = proj (layer 0: Conv2d 768 -> 256, 3x3) or upsampler0 / 1 (layers 1 / 2: ConvTranspose2d 4x4 stride 2),
    on the token-major map x fp32 [NV H W, Cin] (x_packed = its packed-split form, or None: packed here).  Returns (y, y_packed): fp32
    [output rows, Cout] and its packed-split form, the next layer's operand; with `last`, (planar fp32 [NV, Cout, 2 H, 2 W], None).
    Weights are packed on the device from the live parameter at every call.  Kept: x, the pre-activation z, the statistics.  Backward:
    mvs_vitdec_head_bn_bwd (d_z as fp32 and packed-split in one pass), the window weight gradient, the window data gradient.  The conv
    bias sits in front of a batch-statistics BatchNorm: it enters the running mean only and its gradient is returned as exact zeros."""

    @staticmethod
    def forward(ctx, x, x_packed, bn, layer, NV, H, W, last, w, b, gamma, beta):
        name = packing.VITDEC_HEAD[layer]
        if not bn.training:
            raise NotImplementedError("vitdec_forward_train: %s's BatchNorm is in eval mode while the module trains; frozen-BatchNorm "
                                      "gradients are not built" % name)
        x0 = ops._f32c(x.detach())
        if layer == 0 and x0.shape[0] == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size [1, 256, 1, 1] (proj's BatchNorm)")
        g, bt = _vec32(gamma), _vec32(beta)
        xp = x_packed if x_packed is not None else ops.vitdec_pack(x0)
        wp = packing.pack_vitdec_head_train({name + ".0.weight": w}, transposed=False)[name]["w"]
        z = ops.vitdec_head_conv(xp, wp, layer, NV, H, W)
        rm, rv, momentum = _bn_train_step(bn, "CrossVITDecoder")
        y, yp, stats = ops.vitdec_head_bn_fwd(z, g, bt, bn.eps, _vec32(b) if rm is not None else None, rm, rv, momentum,
                                              want_packed=True, planar=(NV, 2 * H, 2 * W) if last else None)
        ctx.save_for_backward(x0, z, stats, w, g, bt)
        ctx.layer, ctx.map, ctx.b_like = layer, (NV, H, W), (b.shape, b.dtype)
        if yp is None:
            return y, None
        ctx.mark_non_differentiable(yp)
        return y, yp

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y, _):
        x0, z, stats, w, g, bt = ctx.saved_tensors
        name = packing.VITDEC_HEAD[ctx.layer]
        d_z, d_zp, d_g, d_b = ops.vitdec_head_bn_bwd(ops._f32c(d_y), z, stats, g, bt)
        d_w = ops.vitdec_head_wgrad(d_z, x0, ctx.layer, *ctx.map)
        d_x = None
        if ctx.needs_input_grad[0]:
            wt = packing.pack_vitdec_head_train({name + ".0.weight": w}, forward=False)[name]["wT"]
            d_x = ops.vitdec_head_dgrad(d_zp, wt, ctx.layer, *ctx.map)
        return d_x, None, None, None, None, None, None, None, d_w, torch.zeros(ctx.b_like[0], dtype=ctx.b_like[1], device=d_z.device), d_g, d_b


def vitdec_head_train(module, tokens, NV, h, w):
    """The head of the CrossVITDecoder in train mode on the library's kernels: tokens fp32 [NV h w, 768], token-major -> fp32
    [NV, 64, 4 h, 4 w]; one ``VitdecHeadLayerTrain`` node per layer, the map token-major from the blocks to the last BatchNorm pass."""
    for name in packing.VITDEC_HEAD:
        if not getattr(module, name)[1].training:                   # before any running statistic moves
            raise NotImplementedError("vitdec_forward_train: %s's BatchNorm is in eval mode while the module trains; frozen-BatchNorm "
                                      "gradients are not built" % name)
    t, tp = tokens, None
    for layer, (seq, H, W) in enumerate(((module.proj, h, w), (module.upsampler0, h, w), (module.upsampler1, 2 * h, 2 * w))):
        conv, bn = seq[0], seq[1]
        t, tp = VitdecHeadLayerTrain.apply(t, tp, bn, layer, NV, H, W, layer == 2, conv.weight, conv.bias, bn.weight, bn.bias)
    return t


_FP32_TRAIN_WARNED = False


def stage_forward_train(net, features, proj_matrices, depth_values, tmp, position3d=None) -> Dict[str, torch.Tensor]:
    """StageNet.forward with autograd (cost_volume.py:51-133).  See the module docstring for what runs where."""
    from .module import PureTransformerCostReg
    transformer = isinstance(net.cost_reg, PureTransformerCostReg)
    if isinstance(features, ops.PackedFeatures):
        raise NotImplementedError("the training path takes planar [B,V,C,H,W] features")
    if net.view_group is not None:
        raise NotImplementedError("view sharding is an inference-latency mode; train with DistributedDataParallel over batches (train.py:196-200)")
    B, V, C, H, W = features.shape
    G = net.in_channels
    if G > C:
        raise AssertionError("G must <= C!")                                                      # cost_volume.py:87
    with torch.no_grad():
        hyp = ops._f32c(depth_values)
        feats, code = ops._feat(features)
        hom = ops.compose_homography(proj_matrices)
        entropy = ops.warp_corr_entropy(feats, code, hom, hyp, G)                                 # [B,V-1,H,W], from sim.detach() in the reference
    # the reference runs the visibility CNN once per source view on a batch of B maps (cost_volume.py:93); BatchNorm statistics
    # are per call there, so the views are kept as separate calls here as well
    if G != 8:
        # inference runs such a stage on the shape-generic convolution kernel (module._RegNetBase.forward_cl_generic); the training
        # kernels (BatchNorm statistics, weight gradients, data gradients) exist for the tuned tables' widths only
        raise NotImplementedError("base_ch=%d: the HIP training kernels are built for 8 groups (all shipped configs); inference of this "
                                  "stage works (shape-generic kernel), fine-tuning it does not" % G)
    prec = getattr(net, "conv_precision", "bf16x3")
    if prec == "fp32":
        # a head configured for exact-fp32 INFERENCE can still be fine-tuned: the training kernels contract in split bf16
        # (three terms: 1e-6 from fp32) with fp32-MFMA weight gradients and fp32 activations - said once, not refused
        global _FP32_TRAIN_WARNED
        if not _FP32_TRAIN_WARNED:
            import warnings
            _FP32_TRAIN_WARNED = True
            warnings.warn("mvsformerplusplus_amd: conv_precision='fp32' selects the exact contraction at inference only; the training path runs "
                          "the fp32-equivalent split-bf16 kernels (forward / data gradients) and fp32-MFMA weight gradients.", RuntimeWarning, stacklevel=3)
    elif prec not in ("bf16x3",) + _lib.F16_FORMATS:       # the fp16 formats are inference storage formats: training keeps fp32 activations on the bf16x3 kernels
        raise NotImplementedError("conv_precision=%r: the native training kernels contract in split bf16 (forward and data gradients) "
                                  "and fp32 MFMA (weight gradients)" % net.conv_precision)
    vis = vis_forward_native(net.vis, entropy)                                                    # [B,V-1,H,W]
    if transformer:
        volume = WarpCorrAggregate.apply(features, vis, hom, hyp, G)                               # [B,G,D,H,W]
        prob_volume_pre = transformer_forward_torch(net.cost_reg, volume, position3d).squeeze(1)
    else:
        volume_cl = WarpCorrAggregate.apply(features, vis, hom, hyp, G, True)                      # [B,D,H,W,G]
        feat_cl = regnet_forward_native(net.cost_reg, volume_cl)                                   # [B,D,H,W,8]
        prob = net.cost_reg.prob
        if tuple(prob.kernel_size) == (1, 1, 1):
            prob_volume_pre = (feat_cl * prob.weight.reshape(1, 1, 1, 1, -1)).sum(-1)              # module.py:486,502
            if prob.bias is not None:
                prob_volume_pre = prob_volume_pre + prob.bias
        else:
            prob_volume_pre = Prob3Train.apply(feat_cl, prob.weight)                               # module.py:391,407
    return stage_head_train(net, prob_volume_pre, depth_values, tmp)


def stage_head_train(net, prob_volume_pre, depth_values, tmp) -> Dict[str, torch.Tensor]:
    """softmax / regression / confidence of a stage in autograd ops (cost_volume.py:105-131), from the logits [B,D,H,W]."""
    prob_volume = F.softmax(prob_volume_pre, dim=1)
    D = prob_volume_pre.shape[1]
    if net.depth_type == "ce":
        if net.training:
            idx = prob_volume.argmax(dim=1, keepdim=True)
            depth = torch.gather(depth_values, 1, idx).squeeze(1)                                 # cost_volume.py:109-112
        else:
            depth = (F.softmax(prob_volume_pre * tmp, dim=1) * depth_values).sum(1)
        conf = prob_volume.max(1)[0]
    else:
        depth = (prob_volume * depth_values).sum(1)
        n = 4 if D >= 32 else (3 if D == 16 else (2 if D == 8 else 0))                            # cost_volume.py:121-128
        conf = conf_regression_torch(prob_volume, n) if n else prob_volume.max(1)[0]
    return {"depth": depth, "prob_volume": prob_volume, "photometric_confidence": conf.detach(),
            "depth_values": depth_values, "prob_volume_pre": prob_volume_pre}


def conf_regression_torch(p: torch.Tensor, n: int) -> torch.Tensor:
    """Confidence of module.py:658-671: the probability mass of the n planes around floor(E[plane index]) - the window is
    [i - n//2, i + n//2] for odd n and [i - n//2 + 1, i + n//2] for even n, clipped to the volume.  Detached like the reference's."""
    D = p.shape[1]
    with torch.no_grad():
        q = p.detach()
        planes = torch.arange(D, device=p.device, dtype=torch.float32).view(1, D, 1, 1)
        idx = (q * planes).sum(1, keepdim=True).long().clamp(0, D - 1)
        lo = n // 2 if n % 2 == 1 else n // 2 - 1
        csum = F.pad(q.cumsum(1), (0, 0, 0, 0, 1, 0))                                             # csum[k] = sum of planes < k
        first = (idx - lo).clamp(0, D)
        last = (idx + n // 2 + 1).clamp(0, D)
        return (torch.gather(csum, 1, last) - torch.gather(csum, 1, first)).squeeze(1)
