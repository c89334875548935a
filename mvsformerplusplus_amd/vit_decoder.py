"""CrossVITDecoder on the device: the ViT feature decoder of the shipped network (``models/module.py:273-364``)
that turns the three DINOv2 interval features into the map added to the FPN's ``conv31``.

``CrossVITDecoder(args)`` takes the reference's constructor argument (the ``arch.args`` dict) and carries its 102 state-dict keys, so a
checkpoint's ``decoder_vit.*`` entries load with ``strict=True``.  Its forward runs on ``csrc/vitdec_kernels.hip``: two self-attention
blocks on the reference views of the batch, three cross-attention blocks on all source views of the batch in one set of launches (a
cross block's key/value summary is computed once per reference view), then ``proj`` and the two transposed convolutions as implicit
GEMMs.  The output is fp32 contiguous ``[B * V, 64, 4 h, 4 w]``.  The inputs (fp32 / bf16 / fp16) are read IN PLACE with their batch,
view and row strides - the reference hands over ``x[:, 1:]`` views of the ViT's output, which are not contiguous - and widened as they
are read: nothing is copied.  ``CrossVITDecoder`` is the inference form: ``train()`` mode or an input that requires grad raises;
``TrainableCrossVITDecoder`` (``patch_vit_decoder(model, trainable=True)``) trains.  ``prev_values`` are read on the
device; there is no host synchronisation, every launch goes to the current stream, and the forward is one linear chain of launches,
capturable by ``torch.cuda.graph`` after one warm call (packed weights are built and uploaded on first use).
``patch_vit_decoder(model)`` swaps a model's ``decoder_vit`` and leaves everything else alone.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops, packing
from .fmt import _Block
from .module import _PackedCache

_TRAIN_MSG = ("%s is the inference form (no autograd): call .eval() and run it under torch.no_grad(), or keep the reference's "
              "models/module.py CrossVITDecoder for training")
D_MODEL, NHEAD, OUT_CH, LEVELS = 768, 12, 64, 3


def _unsupported(key, value):
    raise NotImplementedError("the native CrossVITDecoder is built for the shipped decoder_cfg (attention_type='Linear', d_model=768, nhead=12, "
                              "ffn_type='ffn', init_values set, post_norm=False, pre_norm_query=True, no_combine_norm=False, "
                              "self_cross_types=None, cross_interval_layers=3, vit_ch=768, out_ch=64); got %s=%r" % (key, value))


def _check_cfg(args):
    dino = args["dino_cfg"]
    cfg = dino["decoder_cfg"]
    if cfg.get("attention_type") != "Linear":
        _unsupported("attention_type", cfg.get("attention_type"))
    types = cfg.get("self_cross_types", None)
    if types is not None and any(t != "Linear" for t in types):
        _unsupported("self_cross_types", types)
    if cfg.get("d_model") != D_MODEL:
        _unsupported("d_model", cfg.get("d_model"))
    if cfg.get("nhead") != NHEAD:
        _unsupported("nhead", cfg.get("nhead"))
    if args.get("vit_ch") != D_MODEL:
        _unsupported("vit_ch", args.get("vit_ch"))
    if args.get("out_ch") != OUT_CH:
        _unsupported("out_ch", args.get("out_ch"))
    if cfg.get("ffn_type", "ffn") != "ffn":
        _unsupported("ffn_type", cfg.get("ffn_type"))
    if cfg.get("init_values") is None:
        _unsupported("init_values", None)
    # the reference's CrossBlock defaults (block.py:332-333): post_norm False, pre_norm_query True
    if cfg.get("post_norm", False):
        _unsupported("post_norm", cfg.get("post_norm"))
    if not cfg.get("pre_norm_query", True):
        _unsupported("pre_norm_query", cfg.get("pre_norm_query"))
    if cfg.get("no_combine_norm", False):
        _unsupported("no_combine_norm", cfg.get("no_combine_norm"))
    if dino.get("cross_interval_layers") != LEVELS:
        _unsupported("cross_interval_layers", dino.get("cross_interval_layers"))
    # softmax_scale, train_avg_length: accepted and unused (the Linear attention class ignores them)
    return dino, cfg


class CrossVITDecoder(nn.Module):
    """models/module.py CrossVITDecoder: forward([x0, x1, x2] of [B, V, h w, 768], Fmats=None, vit_shape=[B, V, h, w, 768]) -> fp32
    [B V, 64, 4 h, 4 w]."""

    def __init__(self, args):
        super().__init__()
        self.dino_cfg, self.decoder_cfg = _check_cfg(args)
        cfg = self.decoder_cfg
        self.self_cross_types = cfg.get("self_cross_types", None)
        self.no_combine_norm = False
        self.self_attn_blocks = nn.ModuleList([_Block(D_MODEL, cfg["init_values"]) for _ in range(LEVELS - 1)])
        self.cross_attn_blocks = nn.ModuleList([_Block(D_MODEL, cfg["init_values"]) for _ in range(LEVELS)])
        self.norm_layers = nn.ModuleList([nn.LayerNorm(D_MODEL, eps=1e-6) for _ in range(LEVELS - 1)])
        self.prev_values = nn.ParameterList([nn.Parameter(torch.tensor(float(cfg["prev_values"]))) for _ in range(LEVELS - 1)])
        ch = OUT_CH
        self.proj = nn.Sequential(nn.Conv2d(D_MODEL, ch * 4, 3, stride=1, padding=1), nn.BatchNorm2d(ch * 4), nn.SiLU())
        self.upsampler0 = nn.Sequential(nn.ConvTranspose2d(ch * 4, ch * 2, 4, stride=2, padding=1), nn.BatchNorm2d(ch * 2), nn.SiLU())
        self.upsampler1 = nn.Sequential(nn.ConvTranspose2d(ch * 2, ch, 4, stride=2, padding=1), nn.BatchNorm2d(ch), nn.SiLU())
        self._cache = _PackedCache()

    def _params(self, device):
        def build(dev):
            p = {}
            for kind, blocks in (("self", self.self_attn_blocks), ("cross", self.cross_attn_blocks)):
                for i, blk in enumerate(blocks):
                    p["%s%d" % (kind, i)] = {k: v.to(dev) for k, v in packing.pack_vitdec_block(dict(blk.state_dict())).items()}
            for i in range(LEVELS - 1):
                nl = self.norm_layers[i]
                p["mix%d" % i] = (nl.weight.detach().float().contiguous().to(dev), nl.bias.detach().float().contiguous().to(dev))
                p["pv%d" % i] = self.prev_values[i].detach().float().reshape(1).contiguous().to(dev)          # read by the kernel
            for name, pack in (("proj", packing.pack_vitdec_conv), ("upsampler0", packing.pack_vitdec_deconv),
                               ("upsampler1", packing.pack_vitdec_deconv)):
                conv, bn = getattr(self, name)[0], getattr(self, name)[1]
                stats = {"weight": bn.weight.detach(), "bias": bn.bias.detach(), "running_mean": bn.running_mean, "running_var": bn.running_var,
                         "eps": bn.eps}
                w, b = pack(conv.weight, conv.bias, stats)
                p[name] = (w.to(dev), b.to(dev))
            return p
        return self._cache.get(self, build)

    def _check_shapes(self, x, Fmats, vit_shape):
        if Fmats is not None:
            raise ValueError("CrossVITDecoder.forward: Fmats must be None (the reference ignores it)")
        if vit_shape is None or len(vit_shape) != 5:
            raise ValueError("CrossVITDecoder.forward needs vit_shape = [B, V, h, w, 768]")
        B, V, h, w, C = (int(s) for s in vit_shape)
        if not isinstance(x, (list, tuple)) or len(x) != LEVELS or C != D_MODEL or min(B, V, h, w) < 1 or \
                any((not torch.is_tensor(t)) or tuple(t.shape) != (B, V, h * w, C) for t in x):
            raise ValueError("CrossVITDecoder.forward takes x = three [B, V, h w, 768] tensors and vit_shape = [B, V, h, w, 768]; got %s, %s"
                             % ([tuple(t.shape) if torch.is_tensor(t) else type(t) for t in x] if isinstance(x, (list, tuple)) else type(x),
                                list(vit_shape)))
        return B, V, h, w

    def _check(self, x, Fmats, vit_shape):
        B, V, h, w = self._check_shapes(x, Fmats, vit_shape)
        if self.training or (torch.is_grad_enabled() and any(t.requires_grad for t in x)):
            raise RuntimeError(_TRAIN_MSG % type(self).__name__)
        return B, V, h, w

    @staticmethod
    def _rows_input(t):
        """The tensor the row kernel reads in place: any strides with contiguous channels; other dtypes / layouts are converted."""
        if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            t = t.float()
        ok = t.stride(3) == 1 and t.stride(2) >= 768 and t.stride(0) >= 0 and t.stride(1) >= 0
        return t if ok else t.contiguous()            # expanded / overlapping views and strided channels are materialised

    @staticmethod
    def block(pb, x, xn, kv_packed, NVq, NVkv, n, kv_div):
        """One pre-norm CrossBlock with linear attention on the residual stream x fp32 [NVq n, 768]; xn = packed LayerNorm1(x);
        kv_packed = the packed keys / values of NVkv views (xn itself for self attention, the reference view's un-normalised features
        for cross attention: pre_norm_query); query view i attends to key view i // kv_div."""
        M = NVq * n
        q = ops.vitdec_linear(xn, M, pb["q"], 768, 768, ops.VITDEC_EPI_F32, elu_cols=768)
        kv = ops.vitdec_linear(kv_packed, NVkv * n, pb["kv"], 768, 1536, ops.VITDEC_EPI_F32, elu_cols=768)
        a = ops.vitdec_apply(q, ops.vitdec_kv(kv, NVkv, n), NVq, n, kv_div)
        x1 = ops.vitdec_linear(a, M, pb["proj"], 768, 768, ops.VITDEC_EPI_RESID, bias=pb["attn.proj.bias"], gamma=pb["ls1.gamma"], residual=x)
        xn2 = ops.vitdec_rows(x1.view(NVq, 1, n, 768), 0, 1, ln=(pb["norm2.weight"], pb["norm2.bias"]), want_x=False)[2]
        hid = ops.vitdec_linear(xn2, M, pb["fc1"], 768, 3072, ops.VITDEC_EPI_GELU_SPLIT, bias=pb["mlp.fc1.bias"])
        return ops.vitdec_linear(hid, M, pb["fc2"], 3072, 768, ops.VITDEC_EPI_RESID, bias=pb["mlp.fc2.bias"], gamma=pb["ls2.gamma"], residual=x1)

    def forward(self, x, Fmats=None, vit_shape=None):
        B, V, h, w = self._check(x, Fmats, vit_shape)
        n = h * w
        with torch.no_grad():
            xs = [self._rows_input(t) for t in x]
            dev = xs[0].device
            p = self._params(dev)
            ln1 = lambda pb: (pb["norm1.weight"], pb["norm1.bias"])
            tokens = torch.empty(ops.lib().mvs_vitdec_packed_bytes(B * V * n, 768), dtype=torch.uint8, device=dev)
            # ---- reference views of the batch: self attention, AAS mix + norm between the levels ----
            cur, keys, cur_n = ops.vitdec_rows(xs[0], 0, 1, ln=ln1(p["self0"]), want_packed=V > 1)
            refs = [keys]                                             # ref_feat_list, packed: the cross blocks' keys / values
            for i in range(1, LEVELS):
                y = self.block(p["self%d" % (i - 1)], cur, cur_n, cur_n, B, B, n, 1)
                last = i == LEVELS - 1
                mix = dict(prev=y, prev_value=p["pv%d" % (i - 1)], mix=p["mix%d" % (i - 1)])
                if last:
                    ops.vitdec_rows(xs[i], 0, 1, want_x=False, packed_into=tokens, out_V=V, out_v0=0, **mix)
                    if V > 1 and B == 1:
                        # one batch element: the reference view's rows are the first n rows of `tokens` (a GEMM masks the rows past n)
                        refs.append(tokens[:ops.lib().mvs_vitdec_packed_bytes(n, 768)])
                    elif V > 1:
                        # several: their rows are V n apart in `tokens`, the keys want them one after the other: the same pass once more
                        refs.append(ops.vitdec_rows(xs[i], 0, 1, want_x=False, want_packed=True, **mix)[1])
                else:
                    cur, keys, cur_n = ops.vitdec_rows(xs[i], 0, 1, ln=ln1(p["self%d" % i]), want_packed=V > 1, **mix)
                    refs.append(keys)
            # ---- every source view of the batch in one set of launches per level: view b (V - 1) + j attends to reference view b ----
            if V > 1:
                S = V - 1
                y = None
                for i in range(LEVELS):
                    pb = p["cross%d" % i]
                    if i == 0:
                        cur, _, cur_n = ops.vitdec_rows(xs[0], 1, S, ln=ln1(pb))
                    else:
                        cur, _, cur_n = ops.vitdec_rows(xs[i], 1, S, ln=ln1(pb), prev=y, prev_value=p["pv%d" % (i - 1)], mix=p["mix%d" % (i - 1)])
                    y = self.block(pb, cur, cur_n, refs[i], B * S, B, n, S)             # the summary once per reference view
                ops.vitdec_rows(y.view(B, S, n, 768), 0, S, want_x=False, packed_into=tokens, out_V=V, out_v0=1)
            # ---- [B V, h, w, 768] tokens -> proj -> upsampler0 -> upsampler1 ----
            t = ops.vitdec_conv(tokens, *p["proj"], ops.VITDEC_PROJ, B * V, h, w)
            t = ops.vitdec_conv(t, *p["upsampler0"], ops.VITDEC_UP0, B * V, h, w)
            return ops.vitdec_conv(t, *p["upsampler1"], ops.VITDEC_UP1, B * V, 2 * h, 2 * w, planar=True)


class TrainableCrossVITDecoder(CrossVITDecoder):
    """CrossVITDecoder with autograd: the same constructor, state-dict keys and configuration refusals.  In
    eval() mode its forward is the inference path; in train() mode it is ``training.vitdec_forward_train``: the five blocks and the AAS
    steps forward and backward on the library's kernels, weights packed on the device from the live parameters at every call, the head
    (proj, upsampler0, upsampler1) on its own PyTorch layers with batch-statistics BatchNorm or, with ``native_head=True``, on the
    library's kernels as well (token-major through the head, no atomics, the same bits from run to run; a head
    BatchNorm in eval mode raises, as does a single value per channel).  The ViT features get no gradient (the backbone is frozen): an
    input that requires grad raises."""

    def __init__(self, args, native_head=False):
        super().__init__(args)
        self.native_head = bool(native_head)

    def forward(self, x, Fmats=None, vit_shape=None):
        if not self.training:
            return super().forward(x, Fmats, vit_shape)
        from .training import vitdec_forward_train
        if Fmats is not None:
            raise ValueError("CrossVITDecoder.forward: Fmats must be None (the reference ignores it)")
        return vitdec_forward_train(self, x, vit_shape)                     # checks the shapes itself


def patch_vit_decoder(model: nn.Module, trainable: bool = False, native_head: bool = False) -> nn.Module:
    """Swap ``model.decoder_vit`` (the reference's CrossVITDecoder) for the native module: parameters and buffers carried over by
    ``load_state_dict(strict=True)``, device and train / eval mode preserved.  What the old module's blocks do (post_norm, pre_norm_query)
    and its no_combine_norm flag are read from the old module, because the state dict does not show them.  Everything else is left as
    it is.  Returns ``model``: ``model = patch_vit_decoder(patch_fmt(patch_fpn(patch_model(model))))``.  trainable=True installs
    ``TrainableCrossVITDecoder`` instead of the inference form; native_head=True (with trainable=True) makes its train-mode head run on the
    library's kernels."""
    if native_head and not trainable:
        raise ValueError("patch_vit_decoder: native_head=True selects the train-mode head of TrainableCrossVITDecoder; pass trainable=True")
    old = model.decoder_vit
    blocks = list(getattr(old, "self_attn_blocks", [])) + list(getattr(old, "cross_attn_blocks", []))
    sd = old.state_dict()
    for key in ("self_attn_blocks.0.mlp.fc1.weight", "self_attn_blocks.0.ls1.gamma", "self_attn_blocks.0.attn.q_proj.weight", "norm_layers.0.weight"):
        if key not in sd:
            raise NotImplementedError("the native CrossVITDecoder needs the parameter %s (ffn_type, init_values, the attention class or "
                                      "no_combine_norm differ from the shipped decoder_cfg)" % key)
    old_cfg = dict(getattr(old, "decoder_cfg", {}) or {})
    dino = dict(getattr(old, "dino_cfg", {}) or {})
    cfg = dict(old_cfg, attention_type=old_cfg.get("attention_type", "Linear"), d_model=sd["norm_layers.0.weight"].numel(),
               nhead=old_cfg.get("nhead", NHEAD), init_values=old_cfg.get("init_values", 1.0), prev_values=old_cfg.get("prev_values", 0.5),
               # CrossBlock attributes with its defaults, and the decoder's own flag: not visible in the state dict
               post_norm=any(getattr(blk, "post_norm", False) for blk in blocks),
               pre_norm_query=all(getattr(blk, "pre_norm_query", True) for blk in blocks),
               no_combine_norm=bool(getattr(old, "no_combine_norm", False)),
               self_cross_types=getattr(old, "self_cross_types", None))
    args = {"dino_cfg": dict(dino, decoder_cfg=cfg, cross_interval_layers=len(getattr(old, "cross_attn_blocks", []))),
            "out_ch": sd["upsampler1.0.weight"].shape[1], "vit_ch": sd["proj.0.weight"].shape[1]}
    new = TrainableCrossVITDecoder(args, native_head=native_head) if trainable else CrossVITDecoder(args)
    new.load_state_dict(sd, strict=True)
    ref = next(old.parameters())
    model.decoder_vit = new.to(ref.device).train(old.training)
    return model
