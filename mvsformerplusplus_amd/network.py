"""The whole network's eval forward on the device: ``models/networks/DINOv2_mvsformer_model.py`` DINOv2MVSNet
with every module native and the glue between them as two kernels of ``csrc/resize_kernels.hip``.

``DINOv2MVSNet(args)`` takes the reference's ``arch.args`` and owns ``encoder``, ``decoder``, ``vit``, ``decoder_vit``, ``FMT_module`` and
``fusions`` under the reference's names, so a reference model's state dict and a released checkpoint (``load_checkpoint``) load with
``strict=True``.  ``forward(imgs [1,V,3,H,W], proj_matrices, depth_values, tmp)`` returns the reference's output dictionary:

    resize_bicubic -> ViT -> CrossVITDecoder          the images at (H rescale // 14 * 14, W rescale // 14 * 14)
    FPNEncoder on all V views at once -> resize_bilinear_add (conv31 + vit_feat) -> FPNDecoder on all V views at once
    FMT_with_pathway -> the cascade                   CascadeDepthHead.forward: this class IS a CascadeDepthHead with a backbone in front

The reference's eval path runs the FPN once per view and stacks; here the views are the batch axis of one pass and the per-stage feature
maps are views of its outputs.  Everything runs on the caller's current stream; after the first call on a shape (packed weights, position
tables, the cascade's ``"auto"`` policy read of a new ``depth_values`` tensor) the forward issues no host synchronisation of its own and
can be captured by ``torch.cuda.graph``.  Inference only, one batch element (the reference's eval path indexes ``vit_feat[vi]`` and is
only right for B = 1): anything else raises.  ``patch_network(reference_model)`` builds the native network from a reference instance.
"""
from __future__ import annotations

import copy
import os
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib, ops
from .cascade import CascadeDepthHead
from .features import FPNDecoder, FPNEncoder
from .fmt import FMT_with_pathway
from .vit import PATCH, vit_base
from .vit_decoder import CrossVITDecoder

PREFIXES = ("encoder", "decoder", "vit", "decoder_vit", "FMT_module", "fusions")

_TRAIN_MSG = ("the native DINOv2MVSNet is the inference form (no autograd through the backbone): call .eval() and run it under "
              "torch.no_grad() on inputs that do not require grad; for training keep the reference's DINOv2MVSNet and swap its modules "
              "with mvsformerplusplus_amd.patch_all(model)")


def checkpoint_state_dict(checkpoint) -> Dict[str, torch.Tensor]:
    """The network's state dict out of a released checkpoint (a path or the loaded dictionary), the way the reference's test.py:213-220
    reads it: ``checkpoint["state_dict"]`` with a leading ``module.`` stripped and every ``pe_dict`` entry left out."""
    if isinstance(checkpoint, (str, os.PathLike)):
        checkpoint = torch.load(str(checkpoint), map_location="cpu")
    if not isinstance(checkpoint, dict) or "state_dict" not in checkpoint:
        raise ValueError("a released checkpoint is a dictionary with a 'state_dict' entry; got %s"
                         % (sorted(checkpoint)[:8] if isinstance(checkpoint, dict) else type(checkpoint).__name__))
    out = {}
    for key, val in checkpoint["state_dict"].items():
        if "pe_dict" in key:
            continue
        out[key[7:] if key.startswith("module.") else key] = val
    return out


class DINOv2MVSNet(CascadeDepthHead):
    """models/networks/DINOv2_mvsformer_model.py DINOv2MVSNet, eval forward.  ``args``: the reference's ``arch.args``.
    ``load_pretrained_vit=False`` skips reading ``args["vit_path"]`` (the weights come from somewhere else anyway)."""

    def __init__(self, args: dict, load_pretrained_vit: bool = True):
        super().__init__(args)
        fusions = self._modules.pop("fusions")               # registered last, as the reference does: the state dict keeps its key order
        self.rescale = float(args["rescale"])
        self.encoder = FPNEncoder(feat_chs=args["feat_chs"])
        self.decoder = FPNDecoder(feat_chs=args["feat_chs"])
        self.vit = vit_base(img_size=518, patch_size=14, init_values=1.0, block_chunks=0, ffn_layer="mlp", **args.get("dino_cfg", {}))
        self.decoder_vit = CrossVITDecoder(args)
        self.FMT_module = FMT_with_pathway(**args.get("FMT_config"))
        vit_path = args.get("vit_path")
        if load_pretrained_vit and vit_path and os.path.exists(vit_path):             # the pretrained backbone; a checkpoint of the whole network overrides it
            sd = torch.load(vit_path, map_location="cpu")
            self.vit.load_state_dict(sd.get("model", sd), strict=False)
        self.fusions = fusions

    def load_checkpoint(self, checkpoint) -> "DINOv2MVSNet":
        """Load a released checkpoint (path or loaded dictionary) with ``strict=True``; see ``checkpoint_state_dict``."""
        self.load_state_dict(checkpoint_state_dict(checkpoint), strict=True)
        return self

    def vit_size(self, H: int, W: int):
        """The ViT's input size for H x W images (DINOv2_mvsformer_model.py:72)."""
        return int(H * self.rescale // PATCH * PATCH), int(W * self.rescale // PATCH * PATCH)

    def _check(self, imgs, others: Sequence[torch.Tensor] = ()):
        if self.training or (torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (imgs,) + tuple(others))):
            raise RuntimeError(_TRAIN_MSG)
        if not torch.is_tensor(imgs) or imgs.dim() != 5 or imgs.shape[2] != 3 or min(imgs.shape) < 1:
            raise ValueError("DINOv2MVSNet takes imgs [1, V, 3, H, W]; got %s" % (tuple(imgs.shape) if torch.is_tensor(imgs) else type(imgs),))
        B, V, _, H, W = imgs.shape
        if B != 1:
            raise NotImplementedError("the native DINOv2MVSNet runs one batch element per call (the reference's eval path adds vit_feat[vi] to "
                                      "every batch element's view vi and is only right for B = 1); got B = %d" % B)
        for t in (imgs,) + tuple(others):
            if torch.is_tensor(t) and (t.device != imgs.device or (_lib._REQUIRE_DEVICE and not t.is_cuda)):
                raise _lib.MvsHipError("DINOv2MVSNet needs every input on one ROCm device (imgs on %s, another input on %s); there is no CPU "
                                       "path" % (imgs.device, t.device))
        if H % 8 or W % 8:
            raise ValueError("DINOv2MVSNet needs H and W multiples of 8 (the FPN's three x2 levels; general_eval.py:120 scales images to "
                             "multiples of 64); got %d x %d" % (H, W))
        vit_h, vit_w = self.vit_size(H, W)
        if vit_h < PATCH or vit_w < PATCH:
            raise ValueError("%d x %d images at rescale %g leave the ViT less than one 14 x 14 patch (%d x %d)" % (H, W, self.rescale, vit_h, vit_w))
        return V, H, W, vit_h, vit_w

    def vit_levels(self, views: torch.Tensor):
        """views fp32 [N, 3, H, W] (the network's normalised images) -> the ViT's interval levels, a list of OWNED fp32 [N, n, 768] tensors (the
        bicubic resize to ``vit_size`` and ``forward_interval_features``, copied out of the ViT's padded buffers).  A view's levels do not
        depend on which views share the call (tests/test_scene.py proves it bit for bit), so a scene driver computes them once per image
        and hands them back through ``forward(..., vit_levels=...)`` for every sample the image takes part in."""
        if not torch.is_tensor(views) or views.dim() != 4:
            raise ValueError("vit_levels takes views [N, 3, H, W]; got %s" % (tuple(views.shape) if torch.is_tensor(views) else type(views),))
        _, H, W, vit_h, vit_w = self._check(views.unsqueeze(0))
        with torch.no_grad():
            vit_imgs = ops.resize_bicubic(views if views.dtype == torch.float32 else views.float(), vit_h, vit_w)
            return [t.clone(memory_format=torch.contiguous_format) for t in self.vit.forward_interval_features(vit_imgs)]

    def _check_levels(self, vit_levels, imgs, V, vit_h, vit_w):
        n = (vit_h // PATCH) * (vit_w // PATCH)
        levels = list(vit_levels)
        for t in levels:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (1, V, n, self.vit.embed_dim) or t.device != imgs.device:
                raise ValueError("vit_levels must be the ViT's interval levels of these views, fp32 [1, %d, %d, %d] on %s each; got %s"
                                 % (V, n, self.vit.embed_dim, imgs.device, (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t)))
        return levels

    def feature_maps(self, imgs: torch.Tensor, capture: Optional[dict] = None, vit_levels=None) -> Dict[str, torch.Tensor]:
        """imgs [1, V, 3, H, W] -> the four FMT outputs {"stageK": fp32 [1, V, C, H / 2^(4-K), W / 2^(4-K)]} that feed the cascade.
        ``capture``: a dict that receives "vit_imgs" (the bicubic output) and "conv31" (after the add) - tests and measurements.
        ``vit_levels``: the views' ViT levels, [1, V, n, 768] each (``vit_levels`` per view, stacked): the resize and the ViT are skipped."""
        V, H, W, vit_h, vit_w = self._check(imgs)
        with torch.no_grad():
            if imgs.dtype != torch.float32:
                imgs = imgs.float()
            views = imgs[0]                                                                   # [V, 3, H, W]: a view, whatever the strides
            if vit_levels is None:
                vit_imgs = ops.resize_bicubic(views, vit_h, vit_w)
                levels = [t.unsqueeze(0) for t in self.vit.forward_interval_features(vit_imgs)]   # [1, V, n, 768] views of the ViT's buffers
            else:
                vit_imgs, levels = None, self._check_levels(vit_levels, imgs, V, vit_h, vit_w)
            vit_feat = self.decoder_vit(levels, Fmats=None, vit_shape=[1, V, vit_h // PATCH, vit_w // PATCH, self.vit.embed_dim])
            conv01, conv11, conv21, conv31 = self.encoder(views)
            conv31 = ops.resize_bilinear_add(conv31, vit_feat)
            feats = self.decoder(conv01, conv11, conv21, conv31)
            if capture is not None:
                capture["vit_imgs"], capture["conv31"] = vit_imgs, conv31
            return self.FMT_module({"stage%d" % (k + 1): f.unsqueeze(0) for k, f in enumerate(feats)})

    def forward(self, imgs: torch.Tensor, proj_matrices: Dict[str, torch.Tensor], depth_values: torch.Tensor,
                tmp: Sequence[float] = (5.0, 5.0, 5.0, 1.0), vit_levels=None) -> Dict[str, torch.Tensor]:
        self._check(imgs, tuple(proj_matrices.values()) + (depth_values,))
        feats = self.feature_maps(imgs) if vit_levels is None else self.feature_maps(imgs, vit_levels=vit_levels)
        return CascadeDepthHead.forward(self, feats, proj_matrices, depth_values, tmp)

    def capture(self, *args, **kwargs):
        raise NotImplementedError("DINOv2MVSNet: capture the forward with torch.cuda.graph after one warm call (CascadeDepthHead.capture takes "
                                  "feature maps, not images)")


def patch_network(reference_model: nn.Module) -> DINOv2MVSNet:
    """The native network built from a reference ``DINOv2MVSNet`` instance: its ``args``, its weights (``strict=True``), its device, eval
    mode.  The reference model is left as it is."""
    args = getattr(reference_model, "args", None)
    if not isinstance(args, dict) or any(not hasattr(reference_model, name) for name in PREFIXES):
        raise TypeError("patch_network takes the reference's DINOv2MVSNet (args, %s); got %s" % (", ".join(PREFIXES), type(reference_model).__name__))
    net = DINOv2MVSNet(copy.deepcopy(args), load_pretrained_vit=False)          # the weights come from the instance
    net.load_state_dict(reference_model.state_dict(), strict=True)
    return net.to(next(reference_model.parameters()).device).eval()
