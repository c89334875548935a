"""TEST ORACLE: a from-scratch torch-functional restatement of the stage-1 transformer regulariser (the reference's PureTransformerCostReg,
models/module.py:602-646, with FlashAttnBlock :535-583, FFN :507-532, LayerNorm3D :586-599, the softmax attention of
models/dino/layers/attention.py and the Frustoconical position encoding of models/position_encoding.py:138-189), written from
include/mvs_hip.h section 8f #1 and the module's state-dict names, computed in fp64 by default: one function per native entry point
(csrc/transformer_kernels.hip) and `regulariser` for the whole module.  Tokens are rows [B, n, 64] in the native order
(td * H/rh + th) * W/rw + tw.  Pinned to fixtures F7 and F31 and to oracle/ref_path.py on the CPU (tests/test_transformer.py); it is the
oracle at the shapes the fixtures lack.

Two error models of the native arithmetic's FORMAT (never of the kernels' code):
  split_operands=True    every GEMM operand (and q, k, v and the probabilities of the attention) is rounded to hi + lo bf16: "bf16x3"
  attn16_operands=True   the attention's q (after the scale * log2 e pre-multiplication) and k are rounded to fp16, its probabilities
                         and v to bf16: the default attention ("attn16")"""
import math

import torch
import torch.nn.functional as F

LOG2E = 1.44269504088896340736


def two_term(t):
    """hi + lo with hi = bf16(t), lo = bf16(t - hi), returned in t's dtype."""
    f = t.float()
    hi = f.to(torch.bfloat16).float()
    lo = (f - hi).to(torch.bfloat16).float()
    return (hi.double() + lo.double()).to(t.dtype)


def _r(t, split):
    return two_term(t) if split else t


def _triple(rate):
    return (rate,) * 3 if isinstance(rate, int) else tuple(rate)


# ---------------------------------------------------------------- positions
def position3d_raw(K, hyp, dtype=torch.float64):
    """K [B, 3, 3], hyp [B, D, H, W] -> the frustum points K^-1 [x, y, 1] * depth, [B, 3, D, H, W]."""
    B, D, H, W = hyp.shape
    y, x = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    pix = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(H * W, dtype=dtype)))            # [3, HW]
    rays = torch.linalg.inv(K.to(dtype)) @ pix                                                   # [B, 3, HW]
    return (rays[:, :, None, :] * hyp.to(dtype).reshape(B, 1, D, H * W)).reshape(B, 3, D, H, W)


def position3d(K, hyp, depth_min, depth_max, ranges=None, dtype=torch.float64):
    """get_position_3d(normalize=True) -> (position3d [B, 3, D, H, W], ranges [4] = height_min, height_max, width_min, width_max);
    `ranges` None = measured over the whole batch."""
    p = position3d_raw(K, hyp, dtype)
    if ranges is None:
        ranges = torch.stack([p[:, 1].min(), p[:, 1].max(), p[:, 0].min(), p[:, 0].max()])
    hmin, hmax, wmin, wmax = [r.to(dtype) for r in ranges]
    dmin, dmax = torch.as_tensor(depth_min).to(dtype), torch.as_tensor(depth_max).to(dtype)
    out = torch.stack([(p[:, 0] - wmin) / (wmax - wmin + 1e-5), (p[:, 1] - hmin) / (hmax - hmin + 1e-5),
                       (torch.minimum(torch.maximum(p[:, 2], dmin), dmax) - dmin) / (dmax - dmin + 1e-5)], 1)
    return out, torch.stack([hmin, hmax, wmin, wmax])


def frequencies(C):
    """The reference's own fp32 table exp(2f * (-ln 1e4 / C))."""
    return torch.exp(torch.arange(0, C, 2).float() * (-math.log(10000.0) / C))


def position_encoding3d(pos, C, rescale=4.0, dtype=torch.float64):
    """pos [B, 3, D, H, W] -> [B, 3C, D, H, W]: channel ax * C + 2f = sin(pos_ax * rescale * div_f), + 1 = cos."""
    B = pos.shape[0]
    ang = pos.to(dtype)[:, :, None] * rescale * frequencies(C).to(dtype)[None, None, :, None, None, None]     # [B, 3, C/2, D, H, W]
    return torch.stack((torch.sin(ang), torch.cos(ang)), 3).reshape(B, 3 * C, *pos.shape[2:])


# ---------------------------------------------------------------- entry points
def embed(x, pos, pe_w, down_w, down_b, ln_w, ln_b, dtype=torch.float64, split_operands=False):
    """x [B, 8, D, H, W] (+ pos [B, 3, D, H, W]; pe_w = pe_proj.weight) -> LayerNorm(Conv3d(k = stride = rate)(x + pe_proj(PE))),
    tokens [B, n, 64].  The position term is added in plain arithmetic; the patch GEMM's operands are split."""
    t = lambda p: p.to(dtype)
    x = t(x)
    if pos is not None:
        x = x + F.conv3d(position_encoding3d(pos, 8, 4.0, dtype), t(pe_w).reshape(8, 24, 1, 1, 1))
    w = t(down_w)
    y = F.conv3d(_r(x, split_operands), _r(w, split_operands), t(down_b), stride=tuple(w.shape[2:]))
    return F.layer_norm(y.flatten(2).transpose(1, 2), (64,), t(ln_w), t(ln_b), 1e-6)


def linear(x, w, bias=None, epilogue="bias", residual=None, gamma=None, ln_w=None, ln_b=None, eps=1e-5, dtype=torch.float64,
           split_operands=False):
    """x [B, n, K], w [N, K]: "bias" x W^T (+ bias) | "gelu" the exact erf GELU of it | "res_ln" LayerNorm(residual + gamma * it)."""
    t = lambda p: p.to(dtype)
    y = F.linear(_r(t(x), split_operands), _r(t(w), split_operands), None if bias is None else t(bias))
    if epilogue == "bias":
        return y
    if epilogue == "gelu":
        return F.gelu(y)
    assert epilogue == "res_ln"
    return F.layer_norm(t(residual) + t(gamma) * y, (y.shape[-1],), t(ln_w), t(ln_b), eps)


def attention(q, k, v, scale, split_operands=False, attn16_operands=False):
    """softmax(q k^T scale) v on [B, heads, n, 16] tensors."""
    if not (split_operands or attn16_operands):
        return torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v
    qs = q * (scale * LOG2E)
    if attn16_operands:
        h16 = lambda u: u.float().clamp(-65504.0, 65504.0).half().to(u.dtype)
        b16 = lambda u: u.float().bfloat16().to(u.dtype)
        s = h16(qs) @ h16(k).transpose(-1, -2)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        return (b16(p) @ b16(v)) / p.sum(-1, keepdim=True)
    s = two_term(qs) @ two_term(k).transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (two_term(p) @ two_term(v)) / p.sum(-1, keepdim=True)


def tr_attention(x, wqkv, heads, scale, dtype=torch.float64, split_operands=False, attn16_operands=False):
    """x [B, n, 64] -> attn.qkv (no bias) + attention -> [B, n, 64]."""
    B, n, C = x.shape
    qkv = linear(x, wqkv, dtype=dtype, split_operands=split_operands).reshape(B, n, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    return attention(qkv[0], qkv[1], qkv[2], scale, split_operands, attn16_operands).transpose(1, 2).reshape(B, n, C)


def up_prob(tokens, dhw, up_w, up_b, ln_w, ln_b, prob_w, prob_b, dtype=torch.float64, split_operands=False):
    """tokens [B, n, 64] -> prob(LayerNorm3D(ConvTranspose3d(k = stride = rate)(tokens))) = logits [B, D, H, W]."""
    t = lambda p: p.to(dtype)
    w = t(up_w)
    rate = tuple(w.shape[2:])
    B = tokens.shape[0]
    D, H, W = dhw
    x = t(tokens).transpose(1, 2).reshape(B, 64, D // rate[0], H // rate[1], W // rate[2])
    y = F.conv_transpose3d(_r(x, split_operands), _r(w, split_operands), t(up_b), stride=rate)
    y = F.layer_norm(y.permute(0, 2, 3, 4, 1), (8,), t(ln_w), t(ln_b), 1e-6)
    return y @ t(prob_w).reshape(8) + t(prob_b).reshape(())


# ---------------------------------------------------------------- the module
def softmax_scale(n, cfg):
    s = (64 // cfg["num_heads"]) ** -0.5
    return s * math.log(n, cfg["train_avg_length"]) if cfg.get("softmax_scale") == "entropy_invariance" else s


def regulariser(x, pos, sd, cfg, dtype=torch.float64, split_operands=False, attn16_operands=False, capture=None):
    """PureTransformerCostReg(8, **cfg).forward(x [B, 8, D, H, W], pos [B, 3, D, H, W] or None) with the state dict `sd` -> logits
    [B, 1, D, H, W] in `dtype`.  `capture` (dict) receives "tokens" (after the embedding) and ("block", i) = the tokens after block i."""
    so = dict(dtype=dtype, split_operands=split_operands)
    B, _, D, H, W = x.shape
    cap = capture if capture is not None else {}
    tok = embed(x, pos, sd["pe_proj.weight"], sd["down.0.weight"], sd["down.0.bias"], sd["down.1.weight"], sd["down.1.bias"], **so)
    cap["tokens"] = tok
    scale = softmax_scale(tok.shape[1], cfg)
    for i in range(cfg["layer_num"]):
        L = lambda k: sd["attention_layers.%d.%s" % (i, k)]
        a = tr_attention(tok, L("attn.qkv.weight"), cfg["num_heads"], scale, attn16_operands=attn16_operands, **so)
        tok = linear(a, L("attn.proj.weight"), L("attn.proj.bias"), "res_ln", tok, L("gamma1"), L("norm1.weight"), L("norm1.bias"), 1e-5, **so)
        hdn = linear(tok, L("ffn.linear1.weight"), L("ffn.linear1.bias"), "gelu", **so)
        tok = linear(hdn, L("ffn.linear2.weight"), L("ffn.linear2.bias"), "res_ln", tok, L("gamma2"), L("norm2.weight"), L("norm2.bias"), 1e-5, **so)
        cap[("block", i)] = tok
    return up_prob(tok, (D, H, W), sd["up.0.weight"], sd["up.0.bias"], sd["up.1.weight"], sd["up.1.bias"], sd["prob.weight"],
                   sd["prob.bias"], **so).unsqueeze(1)
