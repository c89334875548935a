"""TEST ORACLE: a from-scratch torch-functional restatement of the reference's DINOv2 ViT-B/14 as the network calls it
(models/dino/dinov2.py forward_interval_features with block.py / attention.py / mlp.py / layer_scale.py / patch_embed.py: 14 x 14 patch
embedding, class token, interpolated position embedding, pre-norm blocks with LayerNorm eps 1e-6, qkv with bias, softmax attention over
the n + 1 tokens of a view with 12 heads of 64, LayerScale, fc1 - GELU (erf) - fc2, the interval outputs and the final norm), computed in
fp64 by default.  Pinned to fixture F28 on the CPU (tests/test_vit.py); it is the oracle at sizes the fixture lacks, and in fp32 / under
bf16 autocast the PyTorch baseline of scripts/bench_vit.py.  Parameters come as a state dict with the reference's key names; tensors may
live on any device.  `split_operands=True` rounds every GEMM and attention operand (q, k, v and the probabilities) to the two-term bf16
form (hi + lo, both round-to-nearest-even: 2^-17 relative per operand) before the product: the error model of the native arithmetic's
FORMAT."""
import math

import torch
import torch.nn.functional as F

HEADS, D, PATCH = 12, 768, 14


def _p(sd, key, like):
    if like.is_cuda and torch.is_autocast_enabled():
        return sd[key]
    return sd[key].to(device=like.device, dtype=like.dtype)


def two_term(t):
    """hi + lo with hi = bf16(t), lo = bf16(t - hi), returned in t's dtype."""
    f = t.float()
    hi = f.to(torch.bfloat16).float()
    lo = (f - hi).to(torch.bfloat16).float()
    return (hi.double() + lo.double()).to(t.dtype)


class _Ops:
    def __init__(self, sd, split_operands=False):
        self.sd, self.split = sd, split_operands

    def r(self, t):
        return two_term(t) if self.split else t

    def linear(self, t, name):
        return F.linear(self.r(t), self.r(_p(self.sd, name + ".weight", t)), _p(self.sd, name + ".bias", t))

    def ln(self, t, name):
        return F.layer_norm(t, (D,), _p(self.sd, name + ".weight", t), _p(self.sd, name + ".bias", t), 1e-6)


def position_table(pos_embed, gh, gw):
    """Position rows [gh gw + 1, 768] of a gh x gw patch grid (fp32, as the reference computes them whatever the run's dtype): bicubic
    F.interpolate of the side x side table with scale_factor ((gh + 0.1) / side, (gw + 0.1) / side), the first factor on the grid's rows
    (the image's height); a square grid of the table's own size is the table itself."""
    p = pos_embed.detach().float().cpu()
    N = p.shape[1] - 1
    if gh * gw == N and gh == gw:
        return p[0]
    side = int(math.sqrt(N))
    t = p[:, 1:].reshape(1, side, side, D).permute(0, 3, 1, 2)
    t = F.interpolate(t, scale_factor=((gh + 0.1) / math.sqrt(N), (gw + 0.1) / math.sqrt(N)), mode="bicubic")
    assert tuple(t.shape[-2:]) == (gh, gw)
    return torch.cat((p[0, :1], t.permute(0, 2, 3, 1).reshape(-1, D)), 0)


def softmax_scale(ntok, mode=None, train_avg_length=None):
    s = (D // HEADS) ** -0.5
    return s * math.log(ntok, train_avg_length) if mode == "entropy_invariance" else s


def attention(q, k, v, scale, split_operands=False):
    """softmax(q k^T scale) v on [B, heads, n, 64] tensors; with split_operands q * scale * log2(e), k, v and the probabilities
    exp2(s - max) are rounded to hi + lo, as the native core holds them."""
    if not split_operands:
        return torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v
    s = two_term(q * (scale * math.log2(math.e))) @ two_term(k).transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (two_term(p) @ two_term(v)) / p.sum(-1, keepdim=True)


def block(o, L, x, scale):
    """Block L (a key prefix) on tokens x [B, n + 1, 768]."""
    B, N, C = x.shape
    qkv = o.linear(o.ln(x, L + "norm1"), L + "attn.qkv").reshape(B, N, 3, HEADS, C // HEADS).permute(2, 0, 3, 1, 4)
    if x.is_cuda and x.dtype != torch.float64 and not o.split:
        a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], scale=scale)      # the device legs: the call the reference makes
    else:
        a = attention(qkv[0], qkv[1], qkv[2], scale, o.split)
    a = a.transpose(1, 2).reshape(B, N, C)
    x = x + _p(o.sd, L + "ls1.gamma", x) * o.linear(a, L + "attn.proj")
    return x + _p(o.sd, L + "ls2.gamma", x) * o.linear(F.gelu(o.linear(o.ln(x, L + "norm2"), L + "mlp.fc1")), L + "mlp.fc2")


def tokens(o, img):
    """prepare_tokens_with_masks: [B, 3, H, W] -> [B, n + 1, 768]."""
    B, _, H, W = img.shape
    gh, gw = H // PATCH, W // PATCH
    w = _p(o.sd, "patch_embed.proj.weight", img)
    t = F.conv2d(o.r(img), o.r(w), _p(o.sd, "patch_embed.proj.bias", img), stride=PATCH).flatten(2).transpose(1, 2)
    t = torch.cat((_p(o.sd, "cls_token", t).expand(B, -1, -1), t), 1)          # under autocast: fp32 class token, the cat promotes
    return t + position_table(o.sd["pos_embed"], gh, gw).to(device=t.device, dtype=t.dtype)


def vit(img, sd, depth=12, cross_interval_layers=3, dino_layer_idxs=None, softmax_scale_mode=None, train_avg_length=None,
        dtype=torch.float64, capture=None, split_operands=False):
    """img [B, 3, H, W] -> the list forward_interval_features returns ([B, n, 768] each) in `dtype` (None = keep the input's dtype: the
    autocast baseline).  `capture` (dict) receives "tokens" and ("block", i) = (input, output) of every block."""
    x = img if dtype is None else img.to(dtype)
    o = _Ops(sd, split_operands)
    cap = capture if capture is not None else {}
    x = tokens(o, x)
    cap["tokens"] = x
    scale = softmax_scale(x.shape[1], softmax_scale_mode, train_avg_length)
    feats = []
    interval = depth // cross_interval_layers if dino_layer_idxs is None else None
    for i in range(depth):
        y = block(o, "blocks.%d." % i, x, scale)
        cap[("block", i)] = (x, y)
        x = y
        emit = (i in dino_layer_idxs) if dino_layer_idxs is not None else (i + 1) % interval == 0
        if emit and i != depth - 1:
            feats.append(x[:, 1:])
    feats.append(o.ln(x, "norm")[:, 1:])
    return feats
