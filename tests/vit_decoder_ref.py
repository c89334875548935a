"""TEST ORACLE: a from-scratch torch-functional restatement of the reference's CrossVITDecoder (models/module.py:273-364 with the Linear
attention class, pre-norm CrossBlock with pre_norm_query, LayerScale, Mlp, AAS mixing + norm_layers, proj / upsampler0 / upsampler1 with
eval BatchNorm and SiLU), computed in fp64 by default.  The reference itself cannot run in fp64 (CrossLinearAttention casts q, k, v to
fp32).  Pinned to fixture F27 on the CPU (tests/test_vit_decoder.py); it is the oracle at sizes the fixture lacks, and in fp32 / under
bf16 autocast the PyTorch baseline of scripts/bench_vit_decoder.py.  Parameters come as a state dict with the reference's key names;
tensors may live on any device.  `split_operands=True` rounds every GEMM / convolution operand to the two-term bf16 form (hi + lo, both
round-to-nearest-even: 2^-17 relative per operand) before the fp64 product: the error model of the native arithmetic's FORMAT."""
import torch
import torch.nn.functional as F

HEADS, D = 12, 768


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
        b = _p(self.sd, name + ".bias", t) if name + ".bias" in self.sd else None
        return F.linear(self.r(t), self.r(_p(self.sd, name + ".weight", t)), b)

    def ln(self, t, name, eps):
        return F.layer_norm(t, (D,), _p(self.sd, name + ".weight", t), _p(self.sd, name + ".bias", t), eps)


def block(o, L, x, kv=None):
    """CrossBlock L (a key prefix) on tokens x [B, n, 768]; kv = the reference view's features for cross attention, used un-normalised
    (pre_norm_query=True); None = self attention on norm1(x)."""
    xn = o.ln(x, L + "norm1", 1e-5)
    kvn = xn if kv is None else kv
    B, N, C = x.shape
    S = kvn.shape[1]
    acc = x.dtype if x.dtype == torch.float64 else torch.float32
    q = (F.elu(o.linear(xn, L + "attn.q_proj").to(acc)) + 1).reshape(B, N, HEADS, C // HEADS)
    k = (F.elu(o.linear(kvn, L + "attn.k_proj").to(acc)) + 1).reshape(B, S, HEADS, C // HEADS)
    v = o.linear(kvn, L + "attn.v_proj").to(acc).reshape(B, S, HEADS, C // HEADS)
    KV = torch.einsum("nshd,nshm->nhmd", k, v)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", q, k.sum(1)) + 1e-6)
    a = torch.einsum("nlhd,nhmd,nlh->nlhm", q, KV, Z).reshape(B, N, C).to(x.dtype)
    x = x + _p(o.sd, L + "ls1.gamma", x) * o.linear(a, L + "attn.proj")
    return x + _p(o.sd, L + "ls2.gamma", x) * o.linear(F.gelu(o.linear(o.ln(x, L + "norm2", 1e-5), L + "mlp.fc1")), L + "mlp.fc2")


def _bn_silu(o, t, name):
    sd = o.sd
    t = F.batch_norm(t, _p(sd, name + ".1.running_mean", t), _p(sd, name + ".1.running_var", t), _p(sd, name + ".1.weight", t),
                     _p(sd, name + ".1.bias", t), False, 0.0, 1e-5)
    return F.silu(t)


def head(o, tokens, h, w, capture=None):
    """tokens [N, h w, 768] -> proj -> upsampler0 -> upsampler1 -> [N, 64, 4 h, 4 w]."""
    cap = capture if capture is not None else {}
    t = tokens.reshape(tokens.shape[0], h, w, D).permute(0, 3, 1, 2)
    t = _bn_silu(o, F.conv2d(o.r(t), o.r(_p(o.sd, "proj.0.weight", t)), _p(o.sd, "proj.0.bias", t), padding=1), "proj")
    cap["proj"] = t
    t = _bn_silu(o, F.conv_transpose2d(o.r(t), o.r(_p(o.sd, "upsampler0.0.weight", t)), _p(o.sd, "upsampler0.0.bias", t), stride=2, padding=1), "upsampler0")
    cap["upsampler0"] = t
    t = _bn_silu(o, F.conv_transpose2d(o.r(t), o.r(_p(o.sd, "upsampler1.0.weight", t)), _p(o.sd, "upsampler1.0.bias", t), stride=2, padding=1), "upsampler1")
    cap["upsampler1"] = t
    return t


def vit_decoder(x, sd, vit_shape, dtype=torch.float64, capture=None, split_operands=False):
    """x = three [B, V, h w, 768] tensors -> [B V, 64, 4 h, 4 w] in `dtype` (None = keep the inputs' dtype: the autocast baseline).
    `capture` (dict) receives ("self", i) / ("cross", v, i) = (input, key or None, output) of every block, "refs" = ref_feat_list,
    "tokens" = the [B V, h w, 768] tensor before proj, and "proj" / "upsampler0" / "upsampler1"."""
    B, V, h, w, C = vit_shape
    xs = [t if dtype is None else t.to(dtype) for t in x]
    o = _Ops(sd, split_operands)
    cap = capture if capture is not None else {}
    mixed = lambda i, prev, v: o.ln(_p(sd, "prev_values.%d" % (i - 1), prev) * prev + xs[i][:, v], "norm_layers.%d" % (i - 1), 1e-6)
    refs = [xs[0][:, 0]]
    for i in (1, 2):
        y = block(o, "self_attn_blocks.%d." % (i - 1), refs[-1])
        cap[("self", i - 1)] = (refs[-1], None, y)
        refs.append(mixed(i, y, 0))
    cap["refs"] = refs
    views = [refs[-1]]
    for v in range(1, V):
        y = None
        for i in range(3):
            q = xs[0][:, v] if i == 0 else mixed(i, y, v)
            y = block(o, "cross_attn_blocks.%d." % i, q, refs[i])
            cap[("cross", v, i)] = (q, refs[i], y)
        views.append(y)
    tokens = torch.stack(views, 1).reshape(B * V, h * w, C)
    cap["tokens"] = tokens
    return head(o, tokens, h, w, cap)
