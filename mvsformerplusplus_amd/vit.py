"""The frozen DINOv2 ViT-B/14 backbone on the device: ``models/dino/dinov2.py`` ``vit_base(patch_size=14, ...)`` as
the shipped network builds and calls it - ``forward_interval_features(imgs)`` on ``[B V, 3, H', W']`` images with H', W' multiples of 14.

``DinoVisionTransformer(**kwargs)`` / ``vit_base(**kwargs)`` take the reference's constructor arguments and carry its 175 state-dict keys,
so a checkpoint's ``vit.*`` entries (and ``dinov2_vitb14_pretrain.pth``) load with ``strict=True``.  The forward runs on
``csrc/vitdec_kernels.hip`` (patch gather, GEMMs with the embedding / qkv / residual / GELU epilogues, LayerNorm rows) and
``csrc/vit_attention_kernels.hip`` (softmax attention at head dimension 64): one linear chain of 3 + 7 depth + 1 launches on the current
stream, no host synchronisation, capturable by ``torch.cuda.graph`` after one warm call (packed weights and the interpolated position
table are built on first use and cached per parameter version and patch grid).  Every view's tokens are padded to a multiple of 32 rows
in the working buffers; the outputs are fp32 ``[B V, n, 768]`` VIEWS of those buffers (view stride ``npad * 768``) - ``CrossVITDecoder``
reads them in place.  Inference only: an input that requires grad raises; ``train()`` mode is accepted (no dropout, no drop path - the
network calls the frozen ViT under ``no_grad`` in training too).  ``patch_vit(model)`` swaps a model's ``vit``; ``patch_all(model)`` is the
five patches composed.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops, packing
from .fmt import _LayerScale, _Mlp
from .module import _PackedCache

EMBED_DIM, HEADS, HEAD_DIM, PATCH = 768, 12, 64, 14
_LOG2E = 1.4426950408889634


def _unsupported(key, value):
    raise NotImplementedError("the native DinoVisionTransformer is built for the shipped ViT-B/14 (embed_dim=768, num_heads=12, patch_size=14, "
                              "in_chans=3, mlp_ratio=4, ffn_layer='mlp', init_values set, block_chunks=0, qkv_bias / proj_bias / ffn_bias True, "
                              "drop_path_rate=0, no masks); got %s=%r" % (key, value))


class _Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim, bias=True)


class _Block(nn.Module):
    """Parameter container with the reference Block's names (pre-norm, LayerScale, mlp_ratio 4)."""

    def __init__(self, dim, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim)
        self.ls1 = _LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, 4 * dim)
        self.ls2 = _LayerScale(dim, init_values)


class _PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, PATCH, stride=PATCH)


class DinoVisionTransformer(nn.Module):
    """models/dino/dinov2.py DinoVisionTransformer: forward_interval_features([B V, 3, H', W']) -> list of fp32 [B V, n, 768]."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True,
                 ffn_bias=True, proj_bias=True, drop_path_rate=0.0, drop_path_uniform=False, init_values=None, embed_layer=None, act_layer=None,
                 block_fn=None, ffn_layer="mlp", block_chunks=1, cross_layer_num=None, cross_attention_type="FLASH2", **kwargs):
        super().__init__()
        for key, value, ok in (("embed_dim", embed_dim, embed_dim == EMBED_DIM), ("num_heads", num_heads, num_heads == HEADS),
                               ("patch_size", patch_size, patch_size == PATCH), ("in_chans", in_chans, in_chans == 3),
                               ("mlp_ratio", mlp_ratio, float(mlp_ratio) == 4.0), ("ffn_layer", ffn_layer, ffn_layer == "mlp"),
                               ("init_values", init_values, bool(init_values)), ("block_chunks", block_chunks, not block_chunks > 0),
                               ("qkv_bias", qkv_bias, bool(qkv_bias)), ("proj_bias", proj_bias, bool(proj_bias)),
                               ("ffn_bias", ffn_bias, bool(ffn_bias)), ("drop_path_rate", drop_path_rate, not drop_path_rate > 0)):
            if not ok:
                _unsupported(key, value)
        for key, value in (("embed_layer", embed_layer), ("act_layer", act_layer), ("block_fn", block_fn)):
            if value is not None:
                _unsupported(key, value)
        side = (img_size if isinstance(img_size, int) else img_size[0]) // patch_size
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 1
        self.n_blocks = int(depth)
        self.num_heads = num_heads
        self.patch_size = patch_size
        self.cross_layer_num = cross_layer_num
        self.cross_attention_type = cross_attention_type
        self.chunked_blocks = False
        self.cross_interval_layers = kwargs.get("cross_interval_layers", None)
        self.dino_layer_idxs = kwargs.get("dino_layer_idxs", None)
        self.softmax_scale = kwargs.get("softmax_scale", None)
        self.train_avg_length = kwargs.get("train_avg_length", None)
        # use_flash2_dino: accepted either way, the arithmetic is the same
        if self.softmax_scale not in (None, "entropy_invariance"):
            _unsupported("softmax_scale", self.softmax_scale)
        if self.softmax_scale is not None and not (self.train_avg_length and self.train_avg_length > 1):
            _unsupported("train_avg_length", self.train_avg_length)
        if self.dino_layer_idxs is None and not (self.cross_interval_layers and self.n_blocks % self.cross_interval_layers == 0):
            _unsupported("cross_interval_layers", self.cross_interval_layers)
        self.patch_embed = _PatchEmbed(embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, side * side + 1, embed_dim))
        self.blocks = nn.ModuleList([_Block(embed_dim, init_values) for _ in range(self.n_blocks)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.head = nn.Identity()
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        for prm in self.parameters():
            prm.requires_grad = False
        self._cache = _PackedCache()

    @property
    def device(self):
        return self.cls_token.device

    # ---- cached parameter preprocessing ----
    def _params(self, device):
        def build(dev):
            w, b = packing.pack_vit_patch_embed(self.patch_embed.proj.weight, self.patch_embed.proj.bias)
            return {"patch": (w.to(dev), b.to(dev)),
                    "blocks": [{k: v.to(dev) for k, v in packing.pack_vit_block(dict(blk.state_dict())).items()} for blk in self.blocks],
                    "norm": (self.norm.weight.detach().float().contiguous().to(dev), self.norm.bias.detach().float().contiguous().to(dev))}
        return self._cache.get(self, build)

    def _positions(self, device, gh, gw):
        """(pos fp32 [n + 1, 768], cls_pos = cls_token + pos[0]) of a gh x gw grid: once per grid and parameter version."""
        def build(dev):
            pos = packing.vit_position_table(self.pos_embed, gh, gw)
            cls_pos = (self.cls_token.detach().float().cpu().reshape(-1) + pos[0]).contiguous()
            return pos.to(dev), cls_pos.to(dev)
        return self._cache.get(self, build, tag=("pos", gh, gw))

    def softmax_scale_for(self, ntok):
        """attention.py: head_dim ** -0.5, times log(ntok) / log(train_avg_length) under "entropy_invariance"."""
        scale = HEAD_DIM ** -0.5
        if self.softmax_scale == "entropy_invariance":
            scale *= math.log(ntok, self.train_avg_length)
        return scale

    def _emits(self, i):
        if i == self.n_blocks - 1:
            return False
        if self.dino_layer_idxs is not None:
            return i in self.dino_layer_idxs
        return (i + 1) % (self.n_blocks // self.cross_interval_layers) == 0

    @staticmethod
    def block(pb, x, NV, ntok, npad, q_scale):
        """One pre-norm block on the residual stream x fp32 [NV npad, 768] -> a fresh buffer of the same shape (7 launches)."""
        M = NV * npad
        xn = ops.vit_rows(x, ln=(pb["norm1.weight"], pb["norm1.bias"]))[1]
        qkv = ops.vit_qkv(xn, pb["qkv"], pb["attn.qkv.bias"], NV, npad, q_scale)
        a = ops.vit_attention(qkv, NV, ntok, npad)
        x1 = ops.vitdec_linear(a, M, pb["proj"], 768, 768, ops.VITDEC_EPI_RESID, bias=pb["attn.proj.bias"], gamma=pb["ls1.gamma"], residual=x)
        xn2 = ops.vit_rows(x1, ln=(pb["norm2.weight"], pb["norm2.bias"]))[1]
        hid = ops.vitdec_linear(xn2, M, pb["fc1"], 768, 3072, ops.VITDEC_EPI_GELU_SPLIT, bias=pb["mlp.fc1.bias"])
        return ops.vitdec_linear(hid, M, pb["fc2"], 3072, 768, ops.VITDEC_EPI_RESID, bias=pb["mlp.fc2.bias"], gamma=pb["ls2.gamma"], residual=x1)

    def prepare_tokens(self, x):
        """The tokens after the patch embedding, the class token and the position embedding: (fp32 [NV npad, 768], NV, n, npad)."""
        NV, _, H, W = x.shape
        gh, gw = H // PATCH, W // PATCH
        p = self._params(x.device)
        pos, cls_pos = self._positions(x.device, gh, gw)
        return ops.vit_embed(ops.vit_patches(x), p["patch"][0], p["patch"][1], pos, cls_pos, NV, gh * gw), NV, gh * gw, ops.vit_npad(gh * gw + 1)

    def forward_interval_features(self, x, masks=None):
        if masks is not None:
            _unsupported("masks", type(masks).__name__)
        if isinstance(x, (list, tuple)):
            _unsupported("x", "a list of images (forward_features_list)")
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % PATCH or x.shape[3] % PATCH or min(x.shape) < 1:
            raise ValueError("forward_interval_features takes images [B V, 3, H, W] with H and W multiples of 14; got %s"
                             % (tuple(x.shape) if torch.is_tensor(x) else type(x),))
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("DinoVisionTransformer is the inference form (no autograd) of the frozen ViT: run it under torch.no_grad() on an "
                               "input that does not require grad, or keep the reference's models/dino for fine-tuning")
        with torch.no_grad():
            if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                x = x.float()
            xs, NV, n, npad = self.prepare_tokens(x)
            p = self._params(x.device)
            q_scale = self.softmax_scale_for(n + 1) * _LOG2E
            feats = []
            for i, pb in enumerate(p["blocks"]):
                xs = self.block(pb, xs, NV, n + 1, npad, q_scale)              # a buffer of its own: an emitted level is never overwritten
                if self._emits(i):
                    feats.append(xs.view(NV, npad, EMBED_DIM)[:, 1:n + 1])
            y = ops.vit_rows(xs, norm=p["norm"])[0]
            feats.append(y.view(NV, npad, EMBED_DIM)[:, 1:n + 1])
            return feats

    def _other(self, *args, **kwargs):
        raise NotImplementedError("the native DinoVisionTransformer implements forward_interval_features (the only entry the network calls); "
                                  "keep the reference's models/dino for the other forward methods")

    forward = forward_features = forward_features_list = forward_features_with_idxs = forward_features_with_attn = get_intermediate_layers = _other


def vit_base(patch_size=14, **kwargs):
    """models/dino/dinov2.py vit_base: embed_dim 768, depth 12 (or kwargs["depth"]), 12 heads, mlp_ratio 4."""
    kwargs.setdefault("depth", 12)
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=768, num_heads=12, mlp_ratio=4, **kwargs)


def patch_vit(model: nn.Module) -> nn.Module:
    """Swap ``model.vit`` (the reference's DinoVisionTransformer) for the native module: parameters carried over by
    ``load_state_dict(strict=True)``, device and train / eval mode preserved; cross_interval_layers, dino_layer_idxs, softmax_scale and
    train_avg_length are read from the old module (the state dict does not show them).  Everything else is left as it is.  Returns ``model``."""
    old = model.vit
    sd = old.state_dict()
    for key in ("blocks.0.attn.qkv.bias", "blocks.0.ls1.gamma", "blocks.0.mlp.fc1.weight", "blocks.0.attn.proj.bias", "blocks.0.mlp.fc2.bias"):
        if key not in sd:
            raise NotImplementedError("the native DinoVisionTransformer needs the parameter %s (block_chunks, qkv_bias / proj_bias / ffn_bias, "
                                      "init_values or ffn_layer differ from the shipped dino_cfg)" % key)
    blocks = list(getattr(old, "blocks", []))
    for blk in blocks:
        for name in ("drop_path1", "drop_path2"):
            if float(getattr(getattr(blk, name, None), "drop_prob", 0.0) or 0.0) > 0:
                _unsupported("drop_path_rate", getattr(blk, name).drop_prob)
    attn = getattr(blocks[0], "attn", None) if blocks else None
    w = sd["patch_embed.proj.weight"]
    patch = w.shape[-1]
    side = int(math.sqrt(sd["pos_embed"].shape[1] - 1))
    new = DinoVisionTransformer(img_size=side * patch, patch_size=patch, in_chans=w.shape[1], embed_dim=w.shape[0], depth=len(blocks),
                                num_heads=getattr(old, "num_heads", HEADS), mlp_ratio=sd["blocks.0.mlp.fc1.weight"].shape[0] / w.shape[0],
                                init_values=1.0, ffn_layer="mlp", block_chunks=0,
                                cross_interval_layers=getattr(old, "cross_interval_layers", None),
                                dino_layer_idxs=getattr(old, "dino_layer_idxs", None), softmax_scale=getattr(attn, "softmax_scale", None),
                                train_avg_length=getattr(attn, "train_avg_length", None))
    new.load_state_dict(sd, strict=True)
    for prm in new.parameters():
        prm.requires_grad = False
    model.vit = new.to(sd["cls_token"].device).train(old.training)
    return model


def patch_all(model: nn.Module) -> nn.Module:
    """The five patches composed: patch_vit(patch_vit_decoder(patch_fmt(patch_fpn(patch_model(model)))))."""
    from .cascade import patch_model
    from .features import patch_fpn
    from .fmt import patch_fmt
    from .vit_decoder import patch_vit_decoder
    return patch_vit(patch_vit_decoder(patch_fmt(patch_fpn(patch_model(model)))))
