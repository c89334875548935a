"""The FPN feature encoder and decoder on the device.

``FPNEncoder`` / ``FPNDecoder`` take the reference's constructor arguments and carry its submodule, parameter and buffer names
(``models/module.py:47-86, 200-270``), so a checkpoint's ``encoder.*`` / ``decoder.*`` entries load with ``strict=True``.  Their
forward runs every layer through ``csrc/fpn_kernels.hip``: split-bf16 three-term MFMA convolutions (fp32-equivalent) with the
BatchNorm folded on the host, the decoder's lateral merges as one kernel each, and the last level fused so that its 64-channel
full-resolution map is never written.

Outputs are fp32 planar ``[N, C, H, W]``.  Under the reference's bf16 autocast (``test.py:250``) its own modules return bf16; these
return the fp32-equivalent values (inputs in bf16 are widened once).  ``FPNEncoder`` / ``FPNDecoder`` are inference only: ``train()``
mode or an input that requires grad raises.  ``patch_fpn(model)`` swaps a model's ``encoder`` / ``decoder`` for these and leaves
everything else alone.  ``TrainableFPNDecoder`` (``patch_fpn(model, trainable_decoder=True)``) adds the decoder's train mode (DESIGN.md
section 4.18) and ``TrainableFPNEncoder`` (``trainable_encoder=True``) the encoder's (section 4.19).
"""
from __future__ import annotations

from typing import List, Sequence

import torch
import torch.nn as nn

from . import ops, packing
from .module import _PackedCache

SUPPORTED_FEAT_CHS = [8, 16, 32, 64]       # both shipped configs (DINOv2_mvsformer_model.py:34-35, casmvs_model.py:33-34)

_TRAIN_MSG = ("%s is the inference form (folded running BatchNorm statistics, no autograd): call .eval() and run it under torch.no_grad(), "
              "or keep the reference's models/module.py FPNEncoder / FPNDecoder for training")


class Swish(nn.Module):
    """x * sigmoid(x) (module.py Swish); no parameters."""

    def forward(self, x):
        return x * torch.sigmoid(x)


class Conv2d(nn.Module):
    """The reference's ``Conv2d`` block with norm_type="BN": ``conv`` (no bias) + ``bn`` + leaky_relu(0.1).  Parameter container only:
    the encoder runs it natively."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bn_momentum=0.1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_channels, momentum=bn_momentum)
        self.kernel_size, self.stride = kernel_size, stride


def _check_feat_chs(feat_chs):
    if list(feat_chs) != SUPPORTED_FEAT_CHS:
        raise NotImplementedError("the native FPN is built for feat_chs = %s (both shipped configs); got %s" % (SUPPORTED_FEAT_CHS, list(feat_chs)))


def _check_inference(mod: nn.Module, *xs):
    if mod.training or (torch.is_grad_enabled() and any(x.requires_grad for x in xs)):
        raise RuntimeError(_TRAIN_MSG % type(mod).__name__)


def _folded(conv: nn.Conv2d, bn: nn.BatchNorm2d, stride: int, device):
    """(packed weights, fp32 bias) of conv [+ bias] -> BatchNorm (eval), folded in fp64 like TiledFeatureHead._params."""
    w = conv.weight.detach().cpu().double()
    scale = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
    shift = bn.bias.detach().cpu().double() - bn.running_mean.detach().cpu().double() * scale
    if conv.bias is not None:                  # a conv bias in front of the BatchNorm goes through the same scale
        shift = shift + conv.bias.detach().cpu().double() * scale
    w = (w * scale.reshape(-1, 1, 1, 1)).float()
    return packing.pack_fpn_conv_weights(w, stride).to(device), shift.float().to(device)


class FPNEncoder(nn.Module):
    """models/module.py FPNEncoder (norm_type="BN"): forward(x [N,3,H,W], H and W multiples of 8) -> [conv01, conv11, conv21, conv31]
    (8 / 16 / 32 / 64 channels at 1, 1/2, 1/4, 1/8 resolution), fp32."""

    LAYERS = (("conv00", 7, 1), ("conv01", 5, 1), ("downsample1", 5, 2), ("conv10", 3, 1), ("conv11", 3, 1), ("downsample2", 5, 2),
              ("conv20", 3, 1), ("conv21", 3, 1), ("downsample3", 3, 2), ("conv30", 3, 1), ("conv31", 3, 1))

    def __init__(self, feat_chs: Sequence[int], norm_type: str = "BN"):
        super().__init__()
        _check_feat_chs(feat_chs)
        if norm_type != "BN":
            raise NotImplementedError("the native FPNEncoder folds BatchNorm (norm_type='BN'); the InstanceNorm encoder stays the reference's")
        c0, c1, c2, c3 = feat_chs
        self.conv00 = Conv2d(3, c0, 7, 1, padding=3)
        self.conv01 = Conv2d(c0, c0, 5, 1, padding=2)
        self.downsample1 = Conv2d(c0, c1, 5, stride=2, padding=2)
        self.conv10 = Conv2d(c1, c1, 3, 1, padding=1)
        self.conv11 = Conv2d(c1, c1, 3, 1, padding=1)
        self.downsample2 = Conv2d(c1, c2, 5, stride=2, padding=2)
        self.conv20 = Conv2d(c2, c2, 3, 1, padding=1)
        self.conv21 = Conv2d(c2, c2, 3, 1, padding=1)
        self.downsample3 = Conv2d(c2, c3, 3, stride=2, padding=1)
        self.conv30 = Conv2d(c3, c3, 3, 1, padding=1)
        self.conv31 = Conv2d(c3, c3, 3, 1, padding=1)
        self._cache = _PackedCache()

    def _params(self, device):
        def build(dev):
            return {name: _folded(getattr(self, name).conv, getattr(self, name).bn, s, dev) for name, _, s in self.LAYERS}
        return self._cache.get(self, build)

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        _check_inference(self, x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("FPNEncoder takes images [N, 3, H, W]; got %s" % (tuple(x.shape),))
        H, W = x.shape[-2:]
        if H % 8 or W % 8:
            raise ValueError("the native FPNEncoder needs H and W multiples of 8 (the decoder's x2 upsample-add; general_eval.py:120 scales "
                             "images to multiples of 64); got %d x %d" % (H, W))
        with torch.no_grad():
            p = self._params(x.device)
            outs, t = {}, x
            for name, k, s in self.LAYERS:
                wp, b = p[name]
                t = ops.fpn_conv(t, wp, b, getattr(self, name).conv.out_channels, k, s, ops.FPN_ACT_LEAKY)
                outs[name] = t
            return [outs["conv01"], outs["conv11"], outs["conv21"], outs["conv31"]]


class FPNDecoder(nn.Module):
    """models/module.py FPNDecoder: forward(conv01, conv11, conv21, conv31) -> [out0, out1, out2, out3] (64 / 32 / 16 / 8 channels at
    1/8, 1/4, 1/2, 1 resolution), fp32.  intra_1, intra_2 are written once each (64 channels); intra_3 is computed inside out3's
    convolution and never stored."""

    def __init__(self, feat_chs: Sequence[int]):
        super().__init__()
        _check_feat_chs(feat_chs)
        final_ch = feat_chs[-1]
        self.out0 = nn.Sequential(nn.Conv2d(final_ch, feat_chs[3], kernel_size=1), nn.BatchNorm2d(feat_chs[3]), Swish())
        self.inner1 = nn.Conv2d(feat_chs[2], final_ch, 1)
        self.out1 = nn.Sequential(nn.Conv2d(final_ch, feat_chs[2], kernel_size=3, padding=1), nn.BatchNorm2d(feat_chs[2]), Swish())
        self.inner2 = nn.Conv2d(feat_chs[1], final_ch, 1)
        self.out2 = nn.Sequential(nn.Conv2d(final_ch, feat_chs[1], kernel_size=3, padding=1), nn.BatchNorm2d(feat_chs[1]), Swish())
        self.inner3 = nn.Conv2d(feat_chs[0], final_ch, 1)
        self.out3 = nn.Sequential(nn.Conv2d(final_ch, feat_chs[0], kernel_size=3, padding=1), nn.BatchNorm2d(feat_chs[0]), Swish())
        self._cache = _PackedCache()

    def _params(self, device):
        def build(dev):
            p = {"out%d" % k: _folded(getattr(self, "out%d" % k)[0], getattr(self, "out%d" % k)[1], 1, dev) for k in range(4)}
            for k in (1, 2, 3):
                inner = getattr(self, "inner%d" % k)
                p["inner%d" % k] = (inner.weight.detach().float().reshape(inner.out_channels, -1).contiguous().to(dev),
                                    inner.bias.detach().float().contiguous().to(dev))
            return p
        return self._cache.get(self, build)

    @staticmethod
    def _check_inputs(conv01, conv11, conv21, conv31):
        N, _, h, w = conv31.shape
        want = [(N, 8, 8 * h, 8 * w), (N, 16, 4 * h, 4 * w), (N, 32, 2 * h, 2 * w), (N, 64, h, w)]
        got = [tuple(t.shape) for t in (conv01, conv11, conv21, conv31)]
        if got != want:
            raise ValueError("FPNDecoder takes the encoder's [conv01, conv11, conv21, conv31] (8 / 16 / 32 / 64 channels, each level twice "
                             "the next one's size); got %s" % got)

    def forward(self, conv01: torch.Tensor, conv11: torch.Tensor, conv21: torch.Tensor, conv31: torch.Tensor) -> List[torch.Tensor]:
        _check_inference(self, conv01, conv11, conv21, conv31)
        self._check_inputs(conv01, conv11, conv21, conv31)
        with torch.no_grad():
            p = self._params(conv31.device)
            out0 = ops.fpn_conv(conv31, *p["out0"], 64, 1, 1, ops.FPN_ACT_SWISH)
            intra1 = ops.fpn_merge(conv31, conv21, *p["inner1"])
            out1 = ops.fpn_conv(intra1, *p["out1"], 32, 3, 1, ops.FPN_ACT_SWISH)
            intra2 = ops.fpn_merge(intra1, conv11, *p["inner2"])
            del intra1
            out2 = ops.fpn_conv(intra2, *p["out2"], 16, 3, 1, ops.FPN_ACT_SWISH)
            out3 = ops.fpn_merge_conv(intra2, conv01, *p["inner3"], *p["out3"], 8, ops.FPN_ACT_SWISH)
            return [out0, out1, out2, out3]


class TrainableFPNDecoder(FPNDecoder):
    """FPNDecoder with a train mode: the same constructor and state-dict keys.  In train mode its forward is
    ``training.fpn_decoder_forward_train`` (batch-statistics BatchNorm, running statistics updated, gradients for the inputs and all 22
    parameters).  In eval mode under no_grad it is FPNDecoder.forward, bit for bit.  Eval mode with inputs that require grad - fine-tuning
    through frozen BatchNorm statistics - is not built and raises."""

    def forward(self, conv01: torch.Tensor, conv11: torch.Tensor, conv21: torch.Tensor, conv31: torch.Tensor) -> List[torch.Tensor]:
        if self.training:
            from .training import fpn_decoder_forward_train
            return fpn_decoder_forward_train(self, conv01, conv11, conv21, conv31)
        if torch.is_grad_enabled() and any(x.requires_grad for x in (conv01, conv11, conv21, conv31)):
            raise RuntimeError("TrainableFPNDecoder in eval() mode has no autograd: gradients through frozen (running-statistics) BatchNorm are "
                               "not built; call .train() for batch-statistics training, or run eval() under torch.no_grad()")
        return super().forward(conv01, conv11, conv21, conv31)


class TrainableFPNEncoder(FPNEncoder):
    """FPNEncoder with a train mode: the same constructor and state-dict keys.  In train mode its forward is
    ``training.fpn_encoder_forward_train`` (batch-statistics BatchNorm + LeakyReLU in all 11 blocks, running statistics updated, gradients
    for all 33 parameters; the image gets none, and an image that requires grad raises).  In eval mode under no_grad it is
    FPNEncoder.forward, bit for bit.  Eval mode with grad enabled on an input that requires grad - gradients through frozen BatchNorm
    statistics - is not built and raises."""

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        if self.training:
            from .training import fpn_encoder_forward_train
            return fpn_encoder_forward_train(self, x)
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("TrainableFPNEncoder in eval() mode has no autograd: gradients through frozen (running-statistics) BatchNorm are "
                               "not built; call .train() for batch-statistics training, or run eval() under torch.no_grad()")
        return super().forward(x)


def _feat_chs_of(enc: nn.Module) -> List[int]:
    return [enc.conv00.conv.out_channels, enc.downsample1.conv.out_channels, enc.downsample2.conv.out_channels,
            enc.downsample3.conv.out_channels]


def patch_fpn(model: nn.Module, trainable_decoder: bool = False, trainable_encoder: bool = False) -> nn.Module:
    """Swap ``model.encoder`` / ``model.decoder`` (the reference's FPNEncoder / FPNDecoder) for the native modules: parameters carried
    over by ``load_state_dict(strict=True)``, device and train / eval mode preserved.  The ViT, CrossVITDecoder, FMT, the
    ``conv31 + vit_feat`` add and the fusions are left as they are.  Returns ``model``: ``model = patch_fpn(patch_model(model))``.
    With neither flag both inference forms are installed.  trainable_decoder=True installs ``TrainableFPNDecoder`` as the decoder,
    trainable_encoder=True ``TrainableFPNEncoder`` as the encoder (DESIGN.md sections 4.18, 4.19); with one flag alone the other module
    is left untouched, the very same object."""
    enc, dec = model.encoder, model.decoder
    if not isinstance(enc.conv00.bn, nn.BatchNorm2d):
        raise NotImplementedError("patch_fpn: the encoder's norm is %s; the native FPNEncoder folds BatchNorm2d (norm_type='BN')" % type(enc.conv00.bn).__name__)
    feat_chs = _feat_chs_of(enc)
    if trainable_decoder or trainable_encoder:
        swaps = ((("encoder", enc, TrainableFPNEncoder(feat_chs)),) if trainable_encoder else ()) + \
            ((("decoder", dec, TrainableFPNDecoder(feat_chs)),) if trainable_decoder else ())
    else:
        swaps = (("encoder", enc, FPNEncoder(feat_chs)), ("decoder", dec, FPNDecoder(feat_chs)))
    for name, old, new in swaps:
        new.load_state_dict(old.state_dict(), strict=True)
        ref = next(old.parameters())
        new = new.to(ref.device).train(old.training)
        setattr(model, name, new)
    return model
