"""CPU: the stage-1 transformer regulariser (mvsformerplusplus_amd.module.PureTransformerCostReg, csrc/transformer_kernels.hip) kernel by
kernel on the host emulator against the fp64 restatement (tests/transformer_ref.py): the token GEMM with every instantiated prologue
and epilogue (ops.tr_linear, ops.tr_embed, ops.tr_up_prob), the pos3d_* family, the attention at its padding boundaries, the whole
module at B = 2 for the shipped patch (2, 4, 4) and the constructor's default cubic patch (down_rate = 4: the K = 512 embedding and the
N = 512 up-projection), fixture F31 (the reference at B = 2, down_rate = 4; tests/golden/make_golden.py) and every refusal.  The
check_* functions take a device; tests/test_transformer_gpu.py runs them on an MI355X.

Bars.  "bf16x3" entry points: LAYER_BAR x max(1, max|ref|); "bf16x3" whole module: MODULE_BAR x the output's range (the project's
bars for the same split-bf16 arithmetic, tests/test_fmt.py); on every case the restatement's split_operands model stays below half
the bar (asserted), so the bar has room for the kernel's accumulation order.  Positions 1e-5, ranges 1e-3 (absolute), the encoding 2e-6:
the bars of parity_cases.case_transformer_golden / case_position_encoding_golden.  The default attention ("attn16") at module level:
the kernel's distance from fp64 is at most 4 x the distance of the restatement's attn16_operands model from fp64 on the same case (the
factor covers what the model leaves out: the running maximum's rescale points, the accumulation order and the split GEMMs around it).
Attention alone at n = 1, 2: the formats' own rounding, see attention_small_bound.

Measured (pytest -s prints every figure next to its model figure).  Kernel figure [split_operands / attn16_operands model figure]:
                                                      emulator     MI355X      model
  tr_linear bias / gelu / res_ln, x max(1, max|ref|)  6.1e-6 / 1.8e-6 / 6.5e-6   6.0e-6 / 1.8e-6 / 6.6e-6   [5.3e-6 / 1.3e-6 / 4.3e-6]
  tr_embed  (2,4,4) (4,4,4) (4,2,4) (1,4,8)           6.6e-6 6.5e-6 5.9e-6 7.1e-6   6.7e-6 6.5e-6 5.9e-6 7.1e-6   [4.1e-6 5.1e-6 5.3e-6 4.9e-6]
  tr_up_prob (2,4,4) (4,4,4) (4,2,4) (1,4,8)          7.8e-6 7.2e-6 6.2e-6 7.3e-6   7.7e-6 7.2e-6 6.3e-6 7.0e-6   [4.5e-6 6.1e-6 5.2e-6 5.3e-6]
  position3d 2x8x16x24 / 2x8x144x192, ranges          1.3e-7 / 1.4e-7, 4.3e-5 / 2.0e-5 on both; raw 2.4e-5; encoding 1.3e-7 (MI355X 1.4e-7)
  attention n = 1 / 2: bf16x3                         2.4e-5 / 3.0e-5          1.9e-5 / 3.0e-5     (the formats allow 1.0e-4)
                       bf16p                          2.4e-5 / 2.5e-3          1.9e-5 / 2.5e-3     (6.6e-3 / 6.7e-3)
                       attn16                         6.5e-3 / 5.0e-3          the same            (1.8e-2 / 2.1e-2)
  module, shipped patch, 936 tokens, of the range     bf16x3 1.3e-5, attn16 9.9e-5    1.3e-5, 9.0e-5    [9.5e-6, 1.0e-4]
  module, down_rate = 4 (K = 512), 96 tokens          bf16x3 2.2e-5, attn16 6.4e-4    2.9e-5, 5.4e-4    [1.6e-5, 4.7e-4]
  F31 y / y_nope  bf16x3 (against the reference)      8.8e-6 / 1.2e-5          7.9e-6 / 1.1e-5     [7.2e-6 / 8.7e-6]
                  attn16 (against fp64)               8.1e-4 / 1.5e-3          5.4e-4 / 1.1e-3     [7.4e-4 / 1.2e-3]
The K = 512 embedding and the N = 512 up-projection launch on the MI355X as written (the kernel asks for its 132 864 bytes of dynamic
LDS through hipFuncSetAttribute).  The restatement itself: F7 / F31 within 1.3e-6 x max(1, max|ref|) in fp32 and fp64, oracle/ref_path.py
at B = 2 within 7.8e-7.
"""
import ctypes as C
import functools
import json
import math

import pytest
import torch

import parity_cases as P
import transformer_ref as R
from conftest import golden_weights, load_golden
from mvsformerplusplus_amd import PositionEncoding3D, PureTransformerCostReg, _lib, get_position_3d, ops, packing, synth
from mvsformerplusplus_amd._lib import ptr, stream_of
from test_fmt import LAYER_BAR, MODULE_BAR

CFG = {"base_channel": 8, "mid_channel": 64, "num_heads": 4, "down_rate": [2, 4, 4], "mlp_ratio": 4, "layer_num": 6, "drop": 0.0,
       "attn_drop": 0.0, "position_encoding": True, "attention_type": "FLASH2", "softmax_scale": "entropy_invariance",
       "train_avg_length": 12185, "use_pe_proj": True}                        # the shipped transformer_config
RATES = ((2, 4, 4), (4, 4, 4), (4, 2, 4), (1, 4, 8))                           # K = 256, 512, 256, 256
GRIDS = {1: (1, 1, 1), 12: (2, 2, 3), 45: (3, 3, 5), 96: (4, 4, 6)}            # tokens -> token grid: one tile, ragged, two tiles (ragged second)
BATCHES = (1, 3)
LINEAR_N = (1, 63, 64, 65, 200)
ATTENTION_N = (63, 64, 65, 255, 256, 257, 512)
ATTENTION_MODES = ("bf16x3", "bf16p", "attn16")
SENTINEL = -12345.0
PAD_ROWS = 67                                                                 # sentinel rows behind every output: more than one 64-token tile
BF = _lib.PREC_BF16X3


def rel(got, want):
    """max |got - want| / max(1, max |want|)"""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return float((got.double() - want.double()).abs().max()) / max(1.0, float(want.abs().max()))


def of_range(got, want):
    """max |got - want| / (max(want) - min(want))"""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return float((got.double() - want.double()).abs().max()) / float(want.max() - want.min())


def _dev(t, device):
    return None if t is None else t.to(device).contiguous()


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ---------------------------------------------------------------- token GEMM: ops.tr_linear
def linear_combos(epi):
    if epi == "bias":
        return [dict(K=64, N=N, has_bias=hb) for N in (64, 192, 256) for hb in (True, False)]
    if epi == "gelu":
        return [dict(K=64, N=256)]
    return [dict(K=K, N=64, gamma=gm, eps=eps) for K in (64, 256) for gm in (1e-2, 1.7) for eps in (1e-5, 1e-6)]


def linear_inputs(epi, B, n, K, N, has_bias=True, gamma=None, eps=1e-5):
    """Every batch item its own data.  "gelu": pre-activations span +-6 in every case (the bias carries the span).  "res_ln": residual
    rows with per-token means up to +-8 and unit spread."""
    g = _gen(B, n, K, N, len(epi))
    a = dict(x=torch.randn(B, n, K, generator=g), w=torch.randn(N, K, generator=g) / math.sqrt(K), epilogue=epi, eps=eps,
             bias=torch.randn(N, generator=g) * 0.5 if has_bias else None)
    if epi == "gelu":
        a["x"] = a["x"] * 0.5
        a["bias"] = torch.linspace(-6.0, 6.0, N)
    if epi == "res_ln":
        a["residual"] = torch.randn(B, n, 64, generator=g) + (torch.rand(B, n, 1, generator=g) * 16.0 - 8.0)
        a["gamma"] = torch.tensor([gamma], dtype=torch.float32)
        a["ln_w"] = torch.rand(64, generator=g) + 0.5
        a["ln_b"] = torch.randn(64, generator=g) * 0.2
    return a


def run_linear(device, a):
    """mvs_tr_linear_fwd into a buffer pre-filled with a sentinel: rows past B n stay untouched; ops.tr_linear gives the same bits."""
    B, n, K = a["x"].shape
    N = a["w"].shape[0]
    code = {"bias": _lib.TR_EPI_BIAS, "gelu": _lib.TR_EPI_GELU, "res_ln": _lib.TR_EPI_RES_LN}[a["epilogue"]]
    x, wp, bias = _dev(a["x"], device), _dev(packing.pack_linear_bf16x3(a["w"]), device), _dev(a["bias"], device)
    res, gm, lw, lb = (_dev(a.get(k), device) for k in ("residual", "gamma", "ln_w", "ln_b"))
    buf = torch.full((B * n + PAD_ROWS, N), SENTINEL, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().mvs_tr_linear_fwd(ptr(x), ptr(wp), ptr(bias), code, ptr(res), ptr(gm), ptr(lw), ptr(lb), float(a["eps"]), ptr(buf),
                                            B, n, K, N, BF, stream_of(x)), "mvs_tr_linear_fwd")
    out = buf.cpu()
    assert bool((out[B * n:] == SENTINEL).all()), "rows past B n were written"
    got = out[:B * n].reshape(B, n, N)
    assert torch.equal(got, ops.tr_linear(x, wp, bias, code, N, BF, residual=res, gamma=gm, ln_w=lw, ln_b=lb, ln_eps=a["eps"]).cpu())
    return got


def ref_linear(a, **kw):
    return R.linear(a["x"], a["w"], a["bias"], a["epilogue"], a.get("residual"), a.get("gamma"), a.get("ln_w"), a.get("ln_b"), a["eps"], **kw)


def check_linear(device, epi):
    """-> (worst kernel error, worst split_operands-model error), both x max(1, max|ref|), over the epilogue's combinations x B x n."""
    worst, worst_model = 0.0, 0.0
    for combo in linear_combos(epi):
        for B in BATCHES:
            for n in LINEAR_N:
                a = linear_inputs(epi, B, n, **combo)
                ref = ref_linear(a)
                if epi == "gelu":
                    pre = R.linear(a["x"], a["w"], a["bias"])
                    assert float(pre.min()) < -5.0 and float(pre.max()) > 5.0
                if epi == "res_ln":
                    assert n < 8 or float(a["residual"].mean(-1).abs().max()) > 6.0
                model = rel(ref_linear(a, split_operands=True), ref)
                assert model <= 0.5 * LAYER_BAR, ("the case leaves the bar no room: change the case", epi, combo, B, n, model)
                err = rel(run_linear(device, a), ref)
                assert err <= LAYER_BAR, (epi, combo, B, n, err, model)
                worst, worst_model = max(worst, err), max(worst_model, model)
    return worst, worst_model


# ---------------------------------------------------------------- patch embedding and up-projection: ops.tr_embed, ops.tr_up_prob
def volume_of(rate, n):
    return tuple(t * r for t, r in zip(GRIDS[n], rate))


def embed_inputs(rate, B, n, with_pos):
    D, H, W = volume_of(rate, n)
    g = _gen(B, n, int(with_pos), *rate)
    K = 8 * rate[0] * rate[1] * rate[2]
    return dict(x=torch.randn(B, 8, D, H, W, generator=g), pos=torch.rand(B, 3, D, H, W, generator=g) if with_pos else None,
                pe_w=torch.randn(8, 24, 1, 1, 1, generator=g) * 0.3, down_w=torch.randn(64, 8, *rate, generator=g) / math.sqrt(K),
                down_b=torch.randn(64, generator=g) * 0.2, ln_w=torch.rand(64, generator=g) + 0.5, ln_b=torch.randn(64, generator=g) * 0.2)


def run_embed(device, a, precision=BF):
    """mvs_tr_embed_fwd into a sentinel-padded token buffer; ops.tr_embed gives the same bits."""
    B, _, D, H, W = a["x"].shape
    rate = tuple(a["down_w"].shape[2:])
    n = (D // rate[0]) * (H // rate[1]) * (W // rate[2])
    vol = _dev(a["x"].permute(0, 2, 3, 4, 1), device)
    pos, pe_w = _dev(a["pos"], device), _dev(a["pe_w"].reshape(8, 24), device)
    wp = _dev(packing.pack_linear_bf16x3(packing.patch_embed_matrix(a["down_w"])), device)
    bias, lw, lb = _dev(a["down_b"], device), _dev(a["ln_w"], device), _dev(a["ln_b"], device)
    div = R.frequencies(8).tolist()
    cdiv = (C.c_float * 4)(*div)
    buf = torch.full((B * n + PAD_ROWS, 64), SENTINEL, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().mvs_tr_embed_fwd(ptr(vol), ptr(pos), ptr(pe_w) if pos is not None else None,
                                           C.cast(cdiv, C.c_void_p) if pos is not None else None, ptr(wp), ptr(bias), ptr(lw), ptr(lb),
                                           ptr(buf), B, D, H, W, rate[0], rate[1], rate[2], precision, stream_of(vol)), "mvs_tr_embed_fwd")
    out = buf.cpu()
    assert bool((out[B * n:] == SENTINEL).all()), "rows past B n were written"
    got = out[:B * n].reshape(B, n, 64)
    assert torch.equal(got, ops.tr_embed(vol, pos, pe_w, div, wp, bias, lw, lb, rate, precision).cpu())
    return got


def ref_embed(a, **kw):
    return R.embed(a["x"], a["pos"], a["pe_w"], a["down_w"], a["down_b"], a["ln_w"], a["ln_b"], **kw)


def up_inputs(rate, B, n):
    """The up-projection's bias spreads the 8 channels of a voxel (+-3), so that no voxel's LayerNorm3D divides by a chance-small spread."""
    g = _gen(B, n, 5, *rate)
    return dict(tokens=torch.randn(B, n, 64, generator=g), dhw=volume_of(rate, n), up_w=torch.randn(64, 8, *rate, generator=g) / 8.0,
                up_b=torch.linspace(-3.0, 3.0, 8), ln_w=torch.rand(8, generator=g) + 0.5, ln_b=torch.randn(8, generator=g) * 0.2,
                prob_w=torch.randn(1, 8, 1, 1, 1, generator=g) * 0.5, prob_b=torch.randn(1, generator=g) * 0.2)


def run_up_prob(device, a, precision=BF):
    """mvs_tr_up_prob_fwd into a NaN pre-filled logits buffer with one patch layer of padding behind it: every voxel is written (no NaN
    left, and the values are the reference's), nothing behind the volume is; ops.tr_up_prob gives the same bits."""
    B = a["tokens"].shape[0]
    D, H, W = a["dhw"]
    rate = tuple(a["up_w"].shape[2:])
    tok = _dev(a["tokens"], device)
    wp = _dev(packing.pack_linear_bf16x3(packing.patch_expand_matrix(a["up_w"])), device)
    ub, lw, lb = _dev(a["up_b"], device), _dev(a["ln_w"], device), _dev(a["ln_b"], device)
    pw, pb = _dev(a["prob_w"].reshape(8), device), _dev(a["prob_b"].reshape(1), device)
    total = B * D * H * W
    buf = torch.full((total + rate[0] * H * W + 64,), float("nan"), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().mvs_tr_up_prob_fwd(ptr(tok), ptr(wp), ptr(ub), ptr(lw), ptr(lb), ptr(pw), ptr(pb), ptr(buf), B, D, H, W,
                                             rate[0], rate[1], rate[2], precision, stream_of(tok)), "mvs_tr_up_prob_fwd")
    out = buf.cpu()
    assert bool(torch.isnan(out[total:]).all()), "voxels behind the volume were written"
    got = out[:total].reshape(B, D, H, W)
    assert not bool(torch.isnan(got).any()), "a logit voxel was never written"
    assert torch.equal(got, ops.tr_up_prob(tok, wp, ub, lw, lb, pw, pb, (D, H, W), rate, precision).cpu())
    return got


def ref_up_prob(a, **kw):
    return R.up_prob(a["tokens"], a["dhw"], a["up_w"], a["up_b"], a["ln_w"], a["ln_b"], a["prob_w"], a["prob_b"], **kw)


def check_patch_kernels(device, rate):
    """Embed (with and without positions) and up-projection + prob at one patch, B in {1, 3}, n in {1, 12, 45, 96}
    -> {"embed" | "up_prob": (worst kernel error, worst model error)} x max(1, max|ref|)."""
    worst = {"embed": [0.0, 0.0], "up_prob": [0.0, 0.0]}
    for B in BATCHES:
        for n in GRIDS:
            cases = [("embed", embed_inputs(rate, B, n, wp), run_embed, ref_embed) for wp in (True, False)]
            cases.append(("up_prob", up_inputs(rate, B, n), run_up_prob, ref_up_prob))
            for what, a, run, ref_fn in cases:
                ref = ref_fn(a)
                model = rel(ref_fn(a, split_operands=True), ref)
                assert model <= 0.5 * LAYER_BAR, ("the case leaves the bar no room: change the case", what, rate, B, n, model)
                err = rel(run(device, a), ref)
                assert err <= LAYER_BAR, (what, rate, B, n, err, model)
                worst[what] = [max(worst[what][0], err), max(worst[what][1], model)]
    return worst


# ---------------------------------------------------------------- positions: ops.position3d, position3d_raw, position_encoding3d
def frustum(B, D, H, W, seed):
    """B intrinsics (all different) and per-item hypotheses [B, D, H, W] between 430 and 900."""
    g = _gen(B, D, H, W, seed)
    K = torch.zeros(B, 3, 3)
    for b in range(B):
        K[b] = torch.tensor([[2.0 * W * (1 + 0.17 * b), 0.0, 0.5 * W - 0.4 * b], [0.0, 2.1 * W * (1 - 0.08 * b), 0.5 * H + 0.3 * b], [0.0, 0.0, 1.0]])
    near = torch.tensor([430.0 + 45.0 * b for b in range(B)])
    far = torch.tensor([900.0 - 60.0 * b for b in range(B)])
    base = 1.0 / (1.0 / far[:, None] + (1.0 / near - 1.0 / far)[:, None] * torch.linspace(0.0, 1.0, D)[None])
    hyp = (base[:, :, None, None] * (1 + 0.02 * torch.rand(B, D, H, W, generator=g))).contiguous()
    dv = torch.arange(425.0, 2.65 * 191.5 + 425.0, 2.65)[None].repeat(B, 1)
    return K, hyp, dv


def check_positions(device, B, D, H, W):
    """get_position_3d with the range measured over the whole batch, reused, and given -> (worst position error, worst range error)."""
    K, hyp, dv = frustum(B, D, H, W, 1)
    ref, ref_rng = R.position3d(K, hyp, dv.min(), dv.max())
    Kd, hd = _dev(K, device), _dev(hyp, device)
    pos, hmin, hmax, wmin, wmax = get_position_3d(B, H, W, Kd, hd, float(dv.min()), float(dv.max()), None, None, None, None)
    e_pos = float((pos.cpu().double() - ref).abs().max())
    e_rng = float((torch.stack([hmin, hmax, wmin, wmax]).cpu().double() - ref_rng).abs().max())
    assert pos.shape == (B, 3, D, H, W) and e_pos <= 1e-5 and e_rng <= 1e-3, (e_pos, e_rng)
    # the per-item part really differs between the items, and the range is the whole batch's, not one item's
    one = R.position3d(K[:1], hyp[:1], dv.min(), dv.max())[1]
    assert float((one - ref_rng).abs().max()) > 1.0
    again = get_position_3d(B, H, W, Kd, hd, dv.min(), dv.max(), hmin, hmax, wmin, wmax)[0]
    assert torch.equal(again, pos), "reusing the measured range must reproduce the positions"
    given = torch.tensor([-310.5, 287.25, -402.0, 377.5])                   # a later stage's call: another stage's range
    ref_g = R.position3d(K, hyp, dv.min(), dv.max(), ranges=given.double())[0]
    pos_g, *back = get_position_3d(B, H, W, Kd, hd, dv.min(), dv.max(), *[given[i].to(device) for i in range(4)])
    assert torch.equal(torch.stack(back).cpu(), given)
    e_given = float((pos_g.cpu().double() - ref_g).abs().max())
    assert e_given <= 1e-5, e_given
    return max(e_pos, e_given), e_rng


def check_raw_and_encoding(device):
    """position3d_raw and PositionEncoding3D as a tensor at B = 2, C = 8, N = 399 voxels (no multiple of 256)."""
    B, D, H, W = 2, 3, 7, 19
    K, hyp, dv = frustum(B, D, H, W, 2)
    raw = get_position_3d(B, H, W, _dev(K, device), _dev(hyp, device), 0.0, 1.0, None, None, None, None, normalize=False)[0].cpu()
    ref_raw = R.position3d_raw(K, hyp)
    assert torch.allclose(raw.double(), ref_raw, rtol=1e-5, atol=1e-4)      # F19's bar (parity_cases.case_position_encoding_golden)
    pos = R.position3d(K, hyp, dv.min(), dv.max())[0].float()
    worst = 0.0
    for C, rescale in ((8, 4.0), (6, 2.5)):
        pe = PositionEncoding3D(_dev(pos, device), C, rescale=rescale).cpu()
        err = float((pe.double() - R.position_encoding3d(pos, C, rescale)).abs().max())
        assert pe.shape == (B, 3 * C, D, H, W) and err <= 2e-6, (C, err)
        worst = max(worst, err)
    return float((raw.double() - ref_raw).abs().max()), worst


# ---------------------------------------------------------------- attention
def attention_gain(n):
    """case_attention_stress's scores must exceed three times the lazy threshold (it asserts so itself): with few keys its default gain
    of 2 falls short of that, 3 gets there.  An input choice; the case's tolerances stay as they are."""
    return 2.0 if n >= 200 else 3.0


def check_attention_stress(device, n, mode):
    return P.case_attention_stress(device, n=n, gain=attention_gain(n), mode=mode)


def attention_small_bound(q, k, v, scale, mode):
    """What the operand formats themselves allow at a handful of keys, x max|v|: out = sum p_j v_j with p and v rounded to bf16 (2^-9
    relative each; "bf16p": p only) and, for "attn16", q and k rounded to fp16 (2^-12 relative each, which moves a score, and with it
    ln p, by at most 2 x 2^-12 x scale x sum_d |q_d k_d|); the split-bf16 rest gets LAYER_BAR."""
    sabs = float((q.abs() @ k.abs().transpose(-1, -2)).max()) * scale
    fmt = {"bf16x3": 0.0, "bf16p": 2.0 ** -9, "attn16": 2.0 ** -9 + 2.0 ** -9 + 2.0 * 2.0 ** -12 * sabs}[mode]
    return fmt * float(v.abs().max()) + LAYER_BAR * max(1.0, float(v.abs().max()))


def check_attention_small(device, n, mode, B=2):
    """ops.tr_attention at n = 1, 2 against fp64 -> (error, bound)."""
    g = _gen(n, 11)
    x = torch.randn(B, n, 64, generator=g)
    w = torch.randn(192, 64, generator=g) * 0.125
    scale = 0.25
    code = {"attn16": _lib.PREC_ATTN16, "bf16p": _lib.PREC_BF16P, "bf16x3": None}[mode]
    got = ops.tr_attention(_dev(x, device), _dev(packing.pack_linear_bf16x3(w), device), 4, scale, BF, code).cpu()
    ref = R.tr_attention(x, w, 4, scale)
    qkv = R.linear(x, w).reshape(B, n, 3, 4, 16).permute(2, 0, 3, 1, 4)
    bound = attention_small_bound(qkv[0], qkv[1], qkv[2], scale, mode)
    err = float((got.double() - ref).abs().max())
    assert got.shape == ref.shape and err <= bound, (n, mode, err, bound)
    if n == 1:                                                              # one key: the output is v itself, whatever the scores
        assert rel(got, qkv[2].transpose(1, 2).reshape(B, n, 64)) <= (2.0 ** -9 if mode == "attn16" else LAYER_BAR)
    return err, bound


# ---------------------------------------------------------------- the whole module
MODULE_CASES = {"shipped": dict(rate=[2, 4, 4], B=2, D=16, H=36, W=52),        # 936 tokens: ragged for the 64- and the 256-token padding
                "cubic": dict(rate=4, B=2, D=16, H=16, W=24)}                  # 96 tokens, K = 512


def make_module(cfg, sd, device, attention_precision):
    net = PureTransformerCostReg(8, **dict(cfg, attention_precision=attention_precision))
    net.load_state_dict(sd, strict=True)
    return net.eval().to(device)


@functools.lru_cache(maxsize=None)
def module_case(name):
    """Inputs, seeded weights and the three host figures of a whole-module case, computed once: the fp64 restatement and its two format
    models' distances from it (fractions of the output's range)."""
    c = MODULE_CASES[name]
    cfg = dict(CFG, down_rate=c["rate"])
    B, D, H, W = c["B"], c["D"], c["H"], c["W"]
    sd = synth.seeded_state_dict(synth.state_dict_manifest(PureTransformerCostReg(8, **cfg).state_dict()), 3100 + D + W)
    x = torch.randn(B, 8, D, H, W, generator=_gen(B, D, H, W, 9))
    K, hyp, dv = frustum(B, D, H, W, 3)
    pos = R.position3d(K, hyp, dv.min(), dv.max())[0].float()
    with torch.no_grad():
        ref = R.regulariser(x, pos, sd, cfg)
        split = of_range(R.regulariser(x, pos, sd, cfg, split_operands=True), ref)
        attn16 = of_range(R.regulariser(x, pos, sd, cfg, attn16_operands=True), ref)
    return dict(cfg=cfg, sd=sd, x=x, pos=pos, ref=ref, split=split, attn16=attn16)


def judge_module(got, ref, precision, split, attn16, what):
    """-> the kernel's distance from fp64 as a fraction of the output's range, held against the precision's bar."""
    frac = of_range(got, ref)
    if precision == "bf16x3":
        assert split <= 0.5 * MODULE_BAR, ("the case leaves the bar no room: change the case", what, split)
        assert frac <= MODULE_BAR, (what, precision, frac, split)
    else:
        assert frac <= 4.0 * attn16, (what, precision, frac, attn16)
    return frac


def check_module(device, name, precision):
    """The whole module at B = 2, six layers, seeded weights, with positions, against regulariser() in fp64 -> (kernel, model) fractions."""
    c = module_case(name)
    net = make_module(c["cfg"], c["sd"], device, precision)
    with torch.no_grad():
        got = net(_dev(c["x"], device), _dev(c["pos"], device)).cpu()
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    return judge_module(got, c["ref"], precision, c["split"], c["attn16"], name), c["split" if precision == "bf16x3" else "attn16"]


def f31():
    fx = load_golden("f31_transformer_batch.npz")
    return fx, json.loads(fx["cfg"]), golden_weights(fx)


def check_f31(device, precision):
    """Fixture F31 (the reference at B = 2, down_rate = 4): get_position_3d, then the module with and without positions.  "bf16x3" against
    the reference's own outputs, "attn16" against the fp64 restatement (pinned to F31 by test_restatement_pinned_to_fixtures)."""
    fx, cfg, sd = f31()
    B, _, D, H, W = fx["x"].shape
    dv = fx["depth_values"]
    pos, hmin, hmax, wmin, wmax = get_position_3d(B, H, W, _dev(fx["K"], device), _dev(fx["hyp"], device), float(dv.min()), float(dv.max()),
                                                  None, None, None, None)
    assert float((pos.cpu() - fx["position3d"]).abs().max()) <= 1e-5
    assert float((torch.stack([hmin, hmax, wmin, wmax]).cpu() - fx["pe_range"]).abs().max()) <= 1e-3
    net = make_module(cfg, sd, device, precision)
    out = []
    with torch.no_grad():
        for p, key in ((fx["position3d"], "y"), (None, "y_nope")):
            got = net(_dev(fx["x"], device), _dev(p, device)).cpu()
            ref = R.regulariser(fx["x"], p, sd, cfg)
            if precision == "bf16x3":
                frac = of_range(got, fx[key])
                assert frac <= MODULE_BAR, (key, frac)
                model = of_range(R.regulariser(fx["x"], p, sd, cfg, split_operands=True), ref)
                assert model <= 0.5 * MODULE_BAR, model
            else:
                model = of_range(R.regulariser(fx["x"], p, sd, cfg, attn16_operands=True), ref)
                frac = judge_module(got, ref, precision, None, model, key)
            out.append((frac, model))
    return out


def figure(what, kernel, model, bar):
    print("%s: kernel %.3g, model %.3g (bar %s)" % (what, kernel, model, bar))


# ---------------------------------------------------------------- the restatement is tied to what the project already trusts
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_pinned_to_fixtures(dtype):
    """tests/transformer_ref.py reproduces F7 (B = 1, the shipped patch) and F31 (B = 2, down_rate = 4) within the bars
    parity_cases.case_transformer_golden holds the kernels to."""
    for name in ("f7_transformer.npz", "f31_transformer_batch.npz"):
        fx = load_golden(name)
        cfg, sd, dv = json.loads(fx["cfg"]), golden_weights(fx), fx["depth_values"]
        pos, rng = R.position3d(fx["K"], fx["hyp"], dv.min(), dv.max(), dtype=dtype)
        assert pos.dtype == dtype and float((pos - fx["position3d"]).abs().max()) <= 1e-5
        assert float((rng - fx["pe_range"]).abs().max()) <= 1e-3
        again = R.position3d(fx["K"], fx["hyp"], dv.min(), dv.max(), ranges=fx["pe_range"], dtype=dtype)[0]
        assert float((again - fx["position3d"]).abs().max()) <= 1e-5
        with torch.no_grad():
            for p, key in ((fx["position3d"], "y"), (None, "y_nope")):
                y = R.regulariser(fx["x"], p, sd, cfg, dtype=dtype)
                err = rel(y, fx[key])
                assert y.dtype == dtype and err <= 2e-4, (name, key, err)
                print("%s %s in %s: %.3g x max(1, max|ref|)" % (name, key, dtype, err))


def test_restatement_agrees_with_the_oracle_at_batch_two():
    """oracle/ref_path.py (fp32; the reference's "(h w d)" token order) and the restatement on a B = 2 case with a non-cubic patch: the
    positions, their whole-batch ranges and the regulariser, to fp32 noise."""
    from oracle import ref_path as O
    B, D, H, W = 2, 4, 8, 16
    cfg = dict(CFG, down_rate=[4, 2, 4], layer_num=3)
    sd = synth.seeded_state_dict(synth.state_dict_manifest(PureTransformerCostReg(8, **cfg).state_dict()), 77)
    K, hyp, dv = frustum(B, D, H, W, 4)
    x = torch.randn(B, 8, D, H, W, generator=_gen(77))
    with torch.no_grad():
        opos, hmin, hmax, wmin, wmax = O.get_position_3d(H, W, K, hyp, dv.min(), dv.max())
        pos, rng = R.position3d(K, hyp, dv.min(), dv.max())
        assert float((pos - opos).abs().max()) <= 1e-5 and float((rng - torch.stack([hmin, hmax, wmin, wmax])).abs().max()) <= 1e-3
        assert float((R.position_encoding3d(opos, 8) - O.position_encoding_3d(opos, 8)).abs().max()) <= 2e-6
        for p in (opos, None):
            want = O.pure_transformer_cost_reg(x, p, sd, num_heads=4, train_avg_length=cfg["train_avg_length"], prefix="")
            for dtype in (torch.float32, torch.float64):
                err = rel(R.regulariser(x, p, sd, cfg, dtype=dtype), want)
                print("restatement in %s vs oracle/ref_path.py (fp32): %.3g x max(1, max|ref|)" % (dtype, err))
                assert err <= 1e-5, err                                      # three blocks of fp32 rounding, each some 1e-7


def test_format_models_differ_from_plain_fp64():
    """The two options do something: the split model moves the output at the 1e-6 level, the 16-bit attention model by far more."""
    c = module_case("cubic")
    assert 1e-8 < c["split"] < 0.5 * MODULE_BAR and c["attn16"] > 4.0 * c["split"], (c["split"], c["attn16"])


# ---------------------------------------------------------------- the kernels on the emulator
@pytest.mark.parametrize("epi", ["bias", "gelu", "res_ln"])
def test_linear(emu, epi):
    worst, model = check_linear(emu, epi)
    figure("tr_linear %s, x max(1, max|ref|)" % epi, worst, model, LAYER_BAR)


@pytest.mark.parametrize("rate", RATES, ids=lambda r: "x".join(map(str, r)))
def test_embed_and_up_prob(emu, rate):
    for what, (worst, model) in check_patch_kernels(emu, rate).items():
        figure("tr_%s patch %s, x max(1, max|ref|)" % (what, rate), worst, model, LAYER_BAR)


@pytest.mark.parametrize("shape", [(2, 8, 16, 24), (2, 8, 144, 192)], ids=["small", "grid_wraps"])
def test_positions(emu, shape):
    """(2, 8, 144, 192) has more than 1024 x 256 voxels: the partial pass's 1024 blocks each walk more than one stride."""
    e_pos, e_rng = check_positions(emu, *shape)
    print("position3d %s: |error| %.3g (bar 1e-5), ranges %.3g (bar 1e-3)" % (shape, e_pos, e_rng))


def test_raw_positions_and_encoding(emu):
    e_raw, e_pe = check_raw_and_encoding(emu)
    print("position3d_raw |error| %.3g; position_encoding3d |error| %.3g (bar 2e-6)" % (e_raw, e_pe))


@pytest.mark.parametrize("mode", ATTENTION_MODES)
@pytest.mark.parametrize("n", ATTENTION_N)
def test_attention_at_padding_boundaries(emu, n, mode):
    print("attention stress n = %d %s: |error| %.3g" % (n, mode, check_attention_stress(emu, n, mode)))


@pytest.mark.parametrize("mode", ATTENTION_MODES)
@pytest.mark.parametrize("n", [1, 2])
def test_attention_one_and_two_tokens(emu, n, mode):
    err, bound = check_attention_small(emu, n, mode)
    print("attention n = %d %s: |error| %.3g (the formats allow %.3g)" % (n, mode, err, bound))


@pytest.mark.parametrize("precision", ["bf16x3", "attn16"])
@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_module_against_fp64(emu, name, precision):
    frac, model = check_module(emu, name, precision)
    figure("module %s %s, of the output's range" % (name, precision), frac, model, MODULE_BAR if precision == "bf16x3" else "4 x model")


@pytest.mark.parametrize("precision", ["bf16x3", "attn16"])
def test_module_against_f31(emu, precision):
    for (frac, model), key in zip(check_f31(emu, precision), ("y", "y_nope")):
        figure("F31 %s %s, of the output's range" % (key, precision), frac, model, MODULE_BAR if precision == "bf16x3" else "4 x model")


def check_refusals(device):
    """What is not built is refused before any launch: a volume that is no multiple of the patch, a patch whose K is neither 256 nor 512,
    a precision other than PREC_BF16X3."""
    a = embed_inputs((2, 4, 4), 1, 12, True)
    with pytest.raises(_lib.MvsHipError, match="not a multiple"):
        run_embed(device, dict(a, x=a["x"][:, :, :, :7], pos=a["pos"][:, :, :, :7]))
    u = up_inputs((2, 4, 4), 1, 12)
    with pytest.raises(_lib.MvsHipError, match="unsupported patch"):
        run_up_prob(device, dict(u, dhw=(u["dhw"][0], u["dhw"][1] - 1, u["dhw"][2])))
    for rate in ((2, 2, 4), (1, 2, 2), (4, 4, 8)):                          # K = 128, 32, 1024
        b = embed_inputs((2, 4, 4), 1, 1, False)
        b["x"] = torch.zeros(1, 8, *rate)
        b["down_w"] = torch.zeros(64, 8, *rate)
        with pytest.raises(_lib.MvsHipError, match="not instantiated"):
            run_embed(device, b)
    v = up_inputs((2, 4, 4), 1, 1)
    with pytest.raises(_lib.MvsHipError, match="unsupported patch"):
        run_up_prob(device, dict(v, dhw=(1, 2, 2), up_w=torch.zeros(64, 8, 1, 2, 2), tokens=torch.zeros(1, 1, 64)))      # N = 32: no 64-feature chunk
    for prec in (_lib.PREC_FP32, _lib.PREC_F16X2, _lib.PREC_ATTN16):
        with pytest.raises(_lib.MvsHipError, match="split-bf16"):
            run_embed(device, a, precision=prec)
        with pytest.raises(_lib.MvsHipError, match="split-bf16"):
            run_up_prob(device, u, precision=prec)
        with pytest.raises(_lib.MvsHipError, match="split-bf16"):
            ops.tr_linear(torch.zeros(1, 4, 64, device=device), _dev(packing.pack_linear_bf16x3(torch.zeros(64, 64)), device), None,
                          _lib.TR_EPI_BIAS, 64, prec)
    with pytest.raises(_lib.MvsHipError, match="not instantiated"):         # K = 128 is no instantiation of the token GEMM
        ops.tr_linear(torch.zeros(1, 4, 128, device=device), _dev(packing.pack_linear_bf16x3(torch.zeros(64, 128)), device), None,
                      _lib.TR_EPI_BIAS, 64, BF)
    with pytest.raises(_lib.MvsHipError, match="multiple of 64"):
        ops.tr_linear(torch.zeros(1, 4, 64, device=device), _dev(packing.pack_linear_bf16x3(torch.zeros(32, 64)), device), None,
                      _lib.TR_EPI_BIAS, 32, BF)
    # the module: the volume check comes first, a patch that is not built fails loudly at the first call
    net = PureTransformerCostReg(8, **CFG).eval().to(device)
    with pytest.raises(ValueError, match="not a multiple of down_rate"):
        net(torch.zeros(1, 8, 4, 8, 10, device=device), None)
    odd = PureTransformerCostReg(8, **dict(CFG, down_rate=[2, 2, 4])).eval().to(device)
    with pytest.raises(_lib.MvsHipError, match="not instantiated"):
        odd(torch.zeros(1, 8, 4, 4, 8, device=device), None)


def test_refusals(emu):
    check_refusals(emu)
