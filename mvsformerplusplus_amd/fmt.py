"""FMT_with_pathway on the device: the stage-1 linear-attention transformer and the three-level pathway that
sit between the FPN and the cascade in the shipped network (``models/FMT.py:140-206``, ``DINOv2_mvsformer_model.py:84-117``).

``FMT_with_pathway(base_channel=8, **FMT_config)`` takes the reference's constructor arguments and carries its 66 state-dict keys, so a
checkpoint's ``FMT_module.*`` entries load with ``strict=True``.  Its forward runs on ``csrc/fmt_kernels.hip``: per block one
key/value-summary launch pair and one block launch (all source views of a batch together; a cross layer's summary is computed once
per reference view), then one fused launch per pathway level for all views.  Outputs are fp32 planar ``[B, V, C, H, W]``; bf16 inputs
are widened once.  Inference only: ``train()`` mode or an input that requires grad raises.  Capturable by ``torch.cuda.graph`` after one
warm call at the same map size (packed weights and the position table are built and uploaded on first use).  ``patch_fmt(model)`` swaps a model's
``FMT_module`` and leaves everything else alone.

``TrainableFMT_with_pathway`` is the same module with autograd: in eval mode on inputs that need no gradient it
runs the inference path above, otherwise ``training.fmt_forward_train`` - the same forward launches with a hand-written backward per
block and three HIP launches per pathway level.  ``patch_fmt(model, trainable=True)`` installs it.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn as nn

from . import ops, packing
from .module import _PackedCache

_TRAIN_MSG = ("%s is the inference form (no autograd): call .eval() and run it under torch.no_grad(), or keep the reference's "
              "models/FMT.py FMT_with_pathway for training")
STAGE_CHANNELS = (64, 32, 16, 8)
PE_CACHE_ENTRIES = 8          # position tables kept per module (7 MB each at 1152 x 1536)


def _unsupported(what):
    raise NotImplementedError("the native FMT_with_pathway is built for the shipped FMT_config (attention_type='Linear', d_model=64, nhead=4, "
                              "ffn_type='ffn', init_values set, base_channel=8, post_norm=False, pre_norm_query=False, self_cross_types=None, "
                              "layer_names of 'self' / 'cross' with a 'self' before the first 'cross'); got %s" % what)


class _LayerScale(nn.Module):
    def __init__(self, dim, init_values):
        super().__init__()
        self.gamma = nn.Parameter(float(init_values) * torch.ones(dim))


class _Attention(nn.Module):
    """Parameter container with CrossLinearAttention's names: q_proj / k_proj / v_proj without bias, proj with."""

    def __init__(self, dim):
        super().__init__()
        self.q_proj = nn.Linear(dim, dim, bias=False)
        self.k_proj = nn.Linear(dim, dim, bias=False)
        self.v_proj = nn.Linear(dim, dim, bias=False)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    """Parameter container with CrossBlock's names (pre-norm, LayerScale, mlp_ratio 4); FMT_with_pathway runs it natively."""

    def __init__(self, dim, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _Attention(dim)
        self.ls1 = _LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, 4 * dim)
        self.ls2 = _LayerScale(dim, init_values)


class FMT(nn.Module):
    """models/FMT.py FMT: the blocks' parameters and the position encoding table; driven by FMT_with_pathway.forward."""

    def __init__(self, attention_type="FLASH2", d_model=64, nhead=4, layer_names=("self", "cross"), **kwargs):
        super().__init__()
        if attention_type != "Linear":
            _unsupported("attention_type=%r" % (attention_type,))
        if d_model != 64 or nhead != 4:
            _unsupported("d_model=%r, nhead=%r" % (d_model, nhead))
        if kwargs.get("ffn_type", "ffn") != "ffn":
            _unsupported("ffn_type=%r" % (kwargs.get("ffn_type"),))
        if kwargs.get("init_values") is None:
            _unsupported("init_values=None (no LayerScale)")
        # the reference's CrossBlock defaults (block.py:332-333): post_norm False, pre_norm_query TRUE - a config that omits
        # pre_norm_query builds blocks that do not normalise a cross layer's keys / values, which this module does not implement
        if kwargs.get("post_norm", False):
            _unsupported("post_norm=%r" % (kwargs["post_norm"],))
        if kwargs.get("pre_norm_query", True):
            _unsupported("pre_norm_query=%r (the reference's default when the key is absent is True)" % (kwargs.get("pre_norm_query", True),))
        if kwargs.get("self_cross_types") is not None:
            _unsupported("self_cross_types=%r" % (kwargs["self_cross_types"],))
        names = list(layer_names)
        if not names or any(n not in ("self", "cross") for n in names) or names[0] != "self":
            _unsupported("layer_names=%r" % (names,))
        n_self = names.count("self")
        if any(n == "cross" and i // 2 >= n_self for i, n in enumerate(names)):
            _unsupported("layer_names=%r (a cross layer at position i reads the reference view's self layer i // 2)" % (names,))
        # softmax_scale, train_avg_length, attn_backend: accepted and unused (the Linear attention class ignores them)
        self.d_model, self.nhead, self.layer_names, self.attention_type = d_model, nhead, names, attention_type
        self.layers = nn.ModuleList([_Block(d_model, kwargs["init_values"]) for _ in names])
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self._pe = {}                      # at most pe_entries tables, oldest dropped first
        self.pe_entries = PE_CACHE_ENTRIES

    def position_encoding(self, H: int, W: int, device) -> torch.Tensor:
        """PositionEncodingSineNorm(64, max_shape=(128, 128)) as a [64, H*W] table, built on the host as the reference builds it (so
        that no device sin / cos differs from torch's) and cached per (H, W, device) - the last `pe_entries` sizes; the first
        call at a size builds and uploads the table, so a graph capture needs one warm call at that size first."""
        key = (H, W, str(device))
        if key not in self._pe:
            while len(self._pe) >= self.pe_entries:
                del self._pe[next(iter(self._pe))]
            d = self.d_model
            pe = torch.zeros((d, H, W))
            y = torch.ones((H, W)).cumsum(0).float().unsqueeze(0) * 128 / H
            x = torch.ones((H, W)).cumsum(1).float().unsqueeze(0) * 128 / W
            div = torch.exp(torch.arange(0, d // 2, 2).float() * (-math.log(10000.0) / (d // 2)))[:, None, None]
            pe[0::4] = torch.sin(x * div)
            pe[1::4] = torch.cos(x * div)
            pe[2::4] = torch.sin(y * div)
            pe[3::4] = torch.cos(y * div)
            self._pe[key] = pe.reshape(d, H * W).contiguous().to(device)
        return self._pe[key]


class FMT_with_pathway(nn.Module):
    """models/FMT.py FMT_with_pathway: forward({'stage1': [B,V,64,h,w], 'stage2': [B,V,32,.,.], 'stage3': [B,V,16,.,.], 'stage4':
    [B,V,8,.,.]}) -> the same dict of fp32 [B,V,C,H,W] tensors."""

    def __init__(self, base_channel=8, **kwargs):
        super().__init__()
        if base_channel != 8:
            _unsupported("base_channel=%r" % (base_channel,))
        self.FMT = FMT(**kwargs)
        for k in (1, 2, 3):
            c = base_channel * 2 ** (3 - k)
            setattr(self, "dim_reduction_%d" % k, nn.Conv2d(2 * c, c, 1, bias=False))
        for k in (1, 2, 3):
            c = base_channel * 2 ** (3 - k)
            setattr(self, "smooth_%d" % k, nn.Conv2d(c, c, 3, padding=1, bias=False))
        self._cache = _PackedCache()

    def _params(self, device):
        def build(dev):
            p = {}
            for i, blk in enumerate(self.FMT.layers):
                w, v = packing.pack_fmt_block(dict(blk.state_dict()))
                p["block%d" % i] = (w.to(dev), v.to(dev))
            for k in (1, 2, 3):
                red, smooth = getattr(self, "dim_reduction_%d" % k), getattr(self, "smooth_%d" % k)
                p["level%d" % k] = (red.weight.detach().float().reshape(red.out_channels, -1).contiguous().to(dev),
                                    packing.pack_fpn_conv_weights(smooth.weight.detach().float().cpu(), 1).to(dev))
            return p
        return self._cache.get(self, build)

    def _check(self, features: Dict[str, torch.Tensor]):
        ts = [features["stage%d" % s] for s in (1, 2, 3, 4)]
        if self.training or (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
            raise RuntimeError(_TRAIN_MSG % type(self).__name__)
        return self._shapes(features)

    def _shapes(self, features: Dict[str, torch.Tensor]):
        ts = [features["stage%d" % s] for s in (1, 2, 3, 4)]
        B, V = ts[0].shape[:2]
        for t, c in zip(ts, STAGE_CHANNELS):
            if t.dim() != 5 or tuple(t.shape[:3]) != (B, V, c) or t.shape[3] < 1 or t.shape[4] < 1:
                raise ValueError("FMT_with_pathway takes stage1..stage4 = [B, V, 64 / 32 / 16 / 8, H, W] with the same B and V; got %s"
                                 % [tuple(u.shape) for u in ts])
        return ts, B, V

    def forward(self, features: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        ts, B, V = self._check(features)
        with torch.no_grad():
            dev = ts[0].device
            p = self._params(dev)
            f1 = ops._planar32(ts[0])
            h, w = f1.shape[-2:]
            pe = self.FMT.position_encoding(h, w, dev)
            names = self.FMT.layer_names
            out1 = torch.empty(B, V, 64, h, w, dtype=torch.float32, device=dev)
            # reference view: the self layers only; the tokens after each are the cross layers' keys / values
            x, refs, first = f1[:, 0].contiguous(), [], pe
            for i, name in enumerate(names):
                if name == "self":
                    wp, vec = p["block%d" % i]
                    x = ops.fmt_block(x, ops.fmt_kv(x, wp, vec, first), wp, vec, first)
                    first = None
                    refs.append(x)
            out1[:, 0] = x
            if V > 1:
                # every source view of the batch in one launch per layer: view b * (V - 1) + j attends to reference view b
                x, first = f1[:, 1:].reshape(B * (V - 1), 64, h, w), pe
                for i, name in enumerate(names):
                    wp, vec = p["block%d" % i]
                    if name == "self":
                        x = ops.fmt_block(x, ops.fmt_kv(x, wp, vec, first), wp, vec, first)
                    else:
                        ref = refs[i] if len(refs) == len(names) else refs[i // 2]
                        x = ops.fmt_block(x, ops.fmt_kv(ref, wp, vec), wp, vec, first, kv_div=V - 1)     # once per reference view
                    first = None
                out1[:, 1:] = x.reshape(B, V - 1, 64, h, w)
            outs = {"stage1": out1}
            prev = out1.reshape(B * V, 64, h, w)
            for k in (1, 2, 3):
                lat = ops._planar32(ts[k])
                prev = ops.fmt_path(prev, lat.reshape((B * V,) + tuple(lat.shape[2:])), *p["level%d" % k])
                outs["stage%d" % (k + 1)] = prev.reshape((B, V) + tuple(prev.shape[1:]))
            return outs


TRAIN_PE_CACHE_ENTRIES = 32    # the shipped multi-scale training list has 25 sizes: 8 tables would be rebuilt on most steps


class TrainableFMT_with_pathway(FMT_with_pathway):
    """FMT_with_pathway with autograd: the same constructor, state-dict keys and configuration refusals.  In eval mode on inputs that
    need no gradient its forward is the inference path; otherwise it is ``training.fmt_forward_train`` (same outputs, bit for bit)."""

    def __init__(self, base_channel=8, **kwargs):
        super().__init__(base_channel, **kwargs)
        self.FMT.pe_entries = TRAIN_PE_CACHE_ENTRIES

    def forward(self, features: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        ts = [features["stage%d" % s] for s in (1, 2, 3, 4)]
        if not self.training and not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
            return super().forward(features)
        from .training import fmt_forward_train
        return fmt_forward_train(self, features)


def patch_fmt(model: nn.Module, trainable: bool = False) -> nn.Module:
    """Swap ``model.FMT_module`` (the reference's FMT_with_pathway) for the native module: parameters carried over by
    ``load_state_dict(strict=True)``, device and train / eval mode preserved.  Everything else is left as it is.  Returns ``model``:
    ``model = patch_fmt(patch_fpn(patch_model(model)))``.  trainable=True installs ``TrainableFMT_with_pathway`` instead of the
    inference form."""
    old = model.FMT_module
    inner = old.FMT
    cfg = dict(attention_type=getattr(inner, "attention_type", "Linear"), d_model=getattr(inner, "d_model", 64), nhead=getattr(inner, "nhead", 4),
               layer_names=list(getattr(inner, "layer_names", ["self", "cross"] * (len(inner.layers) // 2))), init_values=1.0,
               # what the old module's blocks do (CrossBlock attributes, with its defaults): not visible in the state dict
               post_norm=any(getattr(blk, "post_norm", False) for blk in inner.layers),
               pre_norm_query=any(getattr(blk, "pre_norm_query", True) for blk in inner.layers))
    sd = old.state_dict()
    if "FMT.layers.0.mlp.fc1.weight" not in sd or "FMT.layers.0.ls1.gamma" not in sd or "FMT.layers.0.attn.q_proj.weight" not in sd:
        _unsupported("a module without mlp.fc1 / ls1.gamma / attn.q_proj parameters (ffn_type, init_values or the attention class differ)")
    new = (TrainableFMT_with_pathway if trainable else FMT_with_pathway)(base_channel=old.smooth_3.out_channels, **cfg)
    new.load_state_dict(sd, strict=True)
    ref = next(old.parameters())
    model.FMT_module = new.to(ref.device).train(old.training)
    return model
