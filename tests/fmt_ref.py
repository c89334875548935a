"""TEST ORACLE: a from-scratch torch-functional restatement of the reference's FMT_with_pathway (models/FMT.py:35-206 with the Linear
attention class, pre-norm CrossBlock, LayerScale, Mlp), computed in fp64 by default.  The reference itself cannot run in fp64
(CrossLinearAttention casts q, k, v to fp32).  Pinned to fixture F26 on the CPU (tests/test_fmt.py); it is the oracle at sizes the
fixture lacks, and in fp32 / under bf16 autocast the PyTorch baseline of scripts/bench_fmt.py.  Parameters come as a state dict with the
reference's key names; tensors may live on any device."""
import math

import torch
import torch.nn.functional as F

LAYER_NAMES = ("self", "cross", "self", "cross")        # the shipped FMT_config


def position_encoding(H, W, d=64, dtype=torch.float64):
    """PositionEncodingSineNorm(d, max_shape=(128, 128)): fp32 positions and frequencies like the reference, then `dtype`."""
    p = torch.zeros(d, H, W)
    y = torch.ones(H, W).cumsum(0).float().unsqueeze(0) * 128 / H
    x = torch.ones(H, W).cumsum(1).float().unsqueeze(0) * 128 / W
    div = torch.exp(torch.arange(0, d // 2, 2).float() * (-math.log(10000.0) / (d // 2)))[:, None, None]
    p[0::4] = torch.sin(x * div)
    p[1::4] = torch.cos(x * div)
    p[2::4] = torch.sin(y * div)
    p[3::4] = torch.cos(y * div)
    return p.to(dtype)


def _p(sd, key, like):
    """Parameter `key` for an op on `like`.  Under autocast it is handed over as it is: autocast casts it itself and, for leaf tensors
    that require grad (nn.Parameters, as in the reference's modules), caches the cast for the whole autocast region."""
    if like.is_cuda and torch.is_autocast_enabled():
        return sd[key]
    return sd[key].to(device=like.device, dtype=like.dtype)


def block(sd, i, x, kv=None):
    """Block i on tokens x [B, n, 64]; kv = the reference view's tokens for cross attention (the layer's own norm1 is applied to them)."""
    L = "FMT.layers.%d." % i
    ln = lambda t, n: F.layer_norm(t, (64,), _p(sd, L + n + ".weight", t), _p(sd, L + n + ".bias", t), 1e-5)
    lin = lambda t, n: F.linear(t, _p(sd, L + n + ".weight", t), _p(sd, L + n + ".bias", t) if L + n + ".bias" in sd else None)
    xn = ln(x, "norm1")
    kvn = xn if kv is None else ln(kv, "norm1")
    B, N, C = x.shape
    S = kvn.shape[1]
    q = (F.elu(lin(xn, "attn.q_proj")) + 1).reshape(B, N, 4, 16).to(x.dtype if x.dtype == torch.float64 else torch.float32)
    k = (F.elu(lin(kvn, "attn.k_proj")) + 1).reshape(B, S, 4, 16).to(q.dtype)
    v = lin(kvn, "attn.v_proj").reshape(B, S, 4, 16).to(q.dtype)
    KV = torch.einsum("nshd,nshm->nhmd", k, v)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", q, k.sum(1)) + 1e-6)
    a = torch.einsum("nlhd,nhmd,nlh->nlhm", q, KV, Z).reshape(B, N, C).to(x.dtype)
    x = x + _p(sd, L + "ls1.gamma", x) * lin(a, "attn.proj")
    return x + _p(sd, L + "ls2.gamma", x) * lin(F.gelu(lin(ln(x, "norm2"), "mlp.fc1")), "mlp.fc2")


def level(sd, k, prev, lat):
    """Pathway level k: smooth_k(bilinear(dim_reduction_k(prev), size of lat, align_corners=False) + lat); `merged` is its smooth input."""
    r = F.conv2d(prev, _p(sd, "dim_reduction_%d.weight" % k, prev))
    merged = F.interpolate(r.float() if r.dtype != torch.float64 else r, size=lat.shape[-2:], mode="bilinear") + lat
    return F.conv2d(merged, _p(sd, "smooth_%d.weight" % k, merged), padding=1), merged


def fmt(feats, sd, names=LAYER_NAMES, dtype=torch.float64, capture=None):
    """-> {'stage1'..'stage4': [B, V, C, H, W]} in `dtype`; `capture` (dict) receives every block's (input, output) tokens per view
    under ("blk", view, i), the refs list under "refs" and each level's merged maps under ("merged", k) (lists over views)."""
    f1 = feats["stage1"].to(dtype)
    B, V, C, H, W = f1.shape
    P = position_encoding(H, W, C, dtype).to(f1.device)
    tok = lambda t: (t + P).flatten(2).transpose(1, 2)
    img = lambda t: t.transpose(1, 2).reshape(B, C, H, W)
    outs, refs = {1: [], 2: [], 3: [], 4: []}, []
    cap = capture if capture is not None else {}
    for v in range(V):
        x = tok(f1[:, v])
        for i, n in enumerate(names):
            if v == 0 and n != "self":
                continue
            y = block(sd, i, x) if n == "self" else block(sd, i, x, refs[i] if len(refs) == len(names) else refs[i // 2])
            cap[("blk", v, i)] = (x, y)
            x = y
            if v == 0:
                refs.append(x)
        prev = img(x)
        outs[1].append(prev)
        for k in (1, 2, 3):
            prev, merged = level(sd, k, prev, feats["stage%d" % (k + 1)][:, v].to(dtype))
            cap.setdefault(("merged", k), []).append(merged)
            outs[k + 1].append(prev)
    cap["refs"] = refs
    return {"stage%d" % k: torch.stack(outs[k], 1) for k in outs}
