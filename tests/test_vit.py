"""CPU: the native DINOv2 ViT-B/14 (mvsformerplusplus_amd.vit, csrc/vitdec_kernels.hip, csrc/vit_attention_kernels.hip) on the host emulator
against fixture F28 (the reference's own vit_base, tests/golden/make_golden_vit.py) and the fp64 restatement (tests/vit_ref.py); the
attention core alone on constructed inputs; the position table; the module contract (state-dict names, patch_vit, patch_all) and every
refusal.

Bars (the project's, as tests/test_vit_decoder.py uses them for the same split-bf16 arithmetic): LAYER_BAR for one entry point on its
captured input, MODULE_BAR per level for the whole module.  The ViT chains 12 blocks where the decoder chains 5, so the FORMAT's own error
was measured first: the fp64 restatement with every GEMM and attention operand rounded to hi + lo bf16 sits 6.0e-6 .. 7.0e-6 of each
level's range from the plain fp64 restatement on both F28 cases - a thirtieth of MODULE_BAR, far below the half of it at which a derived
bar would be due - and the reference's own fp32 run sits 5.5e-7 .. 8.1e-7 from fp64.  So the project's bars hold and no new bar was
derived.  Measured on the emulator: whole module 6.7e-6 .. 7.8e-6 (case a) / 9.0e-6 .. 1.2e-5 (case b) of each level's range.  The tests
print their figures (pytest -s)."""
import hashlib
import json
import math

import pytest
import torch
import torch.nn as nn

import vit_ref as R
from conftest import load_golden
from mvsformerplusplus_amd import _lib, ops, packing, synth
from mvsformerplusplus_amd import vit as V
from mvsformerplusplus_amd.vit import DinoVisionTransformer, patch_all, patch_vit, vit_base

LAYER_BAR = 3e-5          # per entry point: x max(1, max|ref|)          (tests/test_fpn.py, tests/test_fmt.py, tests/test_vit_decoder.py)
MODULE_BAR = 2e-4         # whole module: x each level's range
F28_FILES = ("f28_vit_a_in.npz", "f28_vit_a_blk0.npz", "f28_vit_a_blk3.npz", "f28_vit_a_blk7.npz", "f28_vit_a_blk11.npz", "f28_vit_a_out.npz",
             "f28_vit_b.npz")
BLOCKS = (0, 3, 7, 11)
_FX = {}


def f28():
    if not _FX:
        for name in F28_FILES:
            _FX.update({k: v for k, v in load_golden(name).items() if k != "__name__"})
    return _FX


def f28_config(fx):
    return json.loads(fx["vit.config"])


def f28_weights(fx):
    """The state dict F28 was generated with: manifest + seed, pos_embed and cls_token replaced by seeded N(0, 1) values (the override
    stored in F28), checked against the SHA-256 stored in F28."""
    if "sd" not in _FX:
        man = {k: tuple(json.loads(s)) for k, s in zip(fx["vit.keys"], fx["vit.shapes"])}
        sd = synth.seeded_state_dict(man, int(fx["vit.seed"]))
        g = torch.Generator().manual_seed(int(fx["vit.override_seed"]))
        for key in fx["vit.override_keys"]:
            sd[key] = torch.randn(man[key], generator=g)
        h = hashlib.sha256()
        for k in sorted(sd):
            h.update(k.encode())
            h.update(sd[k].contiguous().numpy().tobytes())
        assert h.hexdigest() == fx["vit.sha256"], "torch / numpy generator changed: regenerate F28 (tests/golden/make_golden_vit.py)"
        _FX["sd"] = sd
    return _FX["sd"]


def module(fx, device="cpu", **changes):
    m = vit_base(**dict(f28_config(fx), **changes))
    m.load_state_dict(f28_weights(fx), strict=True)
    return m.eval().to(device)


def close(got, want, bar, what):
    err = float((got.double() - want.double()).abs().max())
    lim = bar * max(1.0, float(want.abs().max()))
    assert got.shape == want.shape and err <= lim, (what, tuple(got.shape), tuple(want.shape), err, lim)
    return err / max(1.0, float(want.abs().max()))


def within_range(got, want, bar, what):
    """max |got - want| <= bar x (max(want) - min(want)); returns the measured fraction of the range."""
    rng = float(want.max() - want.min())
    frac = float((got.double() - want.double()).abs().max()) / rng
    assert got.shape == want.shape and frac <= bar, (what, frac, bar)
    return frac


def padded(t, device):
    """tokens [NV, ntok, 768] -> the residual stream of the native module: fp32 [NV npad, 768], the rows past ntok zero."""
    NV, ntok = t.shape[:2]
    npad = ops.vit_npad(ntok)
    x = torch.zeros(NV, npad, 768)
    x[:, :ntok] = t
    return x.reshape(NV * npad, 768).to(device), NV, ntok, npad


def check_entry_points(fx, device):
    """Every native entry point against F28 case a, each on its captured input: patch gather + embedding + position, blocks 0, 3, 7
    and 11, the final norm."""
    m = module(fx, device)
    p = m._params(torch.device(device))
    tok, NV, n, npad = m.prepare_tokens(fx["a/img"].to(device))
    assert (NV, n, npad) == (3, 24, 32) and tok.shape == (96, 768)
    tok = tok.cpu().view(NV, npad, 768)
    worst = close(tok[:, :n + 1], fx["a/tokens"], LAYER_BAR, "tokens")
    assert float(tok[:, n + 1:].abs().max()) == 0.0                  # the padding rows start as zeros
    q_scale = m.softmax_scale_for(n + 1) * math.log2(math.e)
    for i in BLOCKS:
        x, NV, ntok, npad = padded(fx["a/blk%d_in" % i], device)
        got = m.block(p["blocks"][i], x, NV, ntok, npad, q_scale).cpu().view(NV, npad, 768)
        assert bool(torch.isfinite(got).all())                       # the padding rows stay finite
        worst = max(worst, close(got[:, :ntok], fx["a/blk%d_out" % i], LAYER_BAR, ("block", i)))
    x, NV, ntok, npad = padded(fx["a/blk11_out"], device)
    got = ops.vit_rows(x, norm=p["norm"])[0].cpu().view(NV, npad, 768)
    worst = max(worst, close(got[:, 1:ntok], fx["a/level2"], LAYER_BAR, "final norm"))
    return worst


def check_module(fx, device):
    """Whole module, cases a (3 views, 4 x 6 patches) and b (2 views, 5 x 3 patches: tall) -> per case the measured fraction of each
    level's range.  The levels are strided views of the module's padded buffers."""
    m = module(fx, device)
    out = {}
    for case, NV, n in (("a", 3, 24), ("b", 2, 15)):
        got = m.forward_interval_features(fx[case + "/img"].to(device))
        assert len(got) == 3
        fr = []
        for i, t in enumerate(got):
            assert t.dtype == torch.float32 and t.shape == (NV, n, 768) and t.stride() == (32 * 768, 768, 1)
            fr.append(within_range(t.cpu(), fx["%s/level%d" % (case, i)], MODULE_BAR, (case, i)))
        out[case] = fr
    return out


def test_restatement_pinned_to_f28():
    """tests/vit_ref.py (fp64) reproduces every capture of F28 at 1e-5 x max(1, max|ref|): the oracle at sizes the fixture lacks."""
    fx = f28()
    sd = f28_weights(fx)
    for case in "ab":
        cap = {}
        out = R.vit(fx[case + "/img"], sd, capture=cap)
        close(cap["tokens"], fx[case + "/tokens"], 1e-5, (case, "tokens"))
        for i in range(3):
            close(out[i], fx["%s/level%d" % (case, i)], 1e-5, (case, "level", i))
        if case == "a":
            for i in BLOCKS:
                close(cap[("block", i)][0], fx["a/blk%d_in" % i], 1e-5, ("in", i))
                close(cap[("block", i)][1], fx["a/blk%d_out" % i], 1e-5, ("out", i))
    assert fx["a/img"].shape == (3, 3, 56, 84) and fx["a/tokens"].shape == (3, 25, 768) and fx["b/img"].shape == (2, 3, 70, 42)
    assert fx["b/tokens"].shape == (2, 16, 768) and fx["b/level0"].shape == (2, 15, 768)


def test_entry_points_against_f28(emu):
    worst = check_entry_points(f28(), emu)
    print("vit entry points vs F28: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (worst, LAYER_BAR))


def test_module_against_f28(emu):
    """Both cases against F28 at MODULE_BAR per level, printed beside the format's own error (split_operands=True against fp64) and the
    reference's own fp32-vs-fp64 distance.  The format's error must stay below half of MODULE_BAR for the project's bar to stand (it is a
    thirtieth of it): asserted here, from the restatement alone."""
    fx = f28()
    fr = check_module(fx, emu)
    sd = f28_weights(fx)
    for case in "ab":
        o64 = R.vit(fx[case + "/img"], sd)
        osp = R.vit(fx[case + "/img"], sd, split_operands=True)
        for i in range(3):
            want = fx["%s/level%d" % (case, i)]
            rng = float(want.max() - want.min())
            model = float((osp[i] - o64[i]).abs().max()) / rng
            ref32 = float((want.double() - o64[i]).abs().max()) / rng
            assert model <= MODULE_BAR / 2, (case, i, model)
            print("ViT vs F28 case %s level %d: |error| = %.3g of the level's range (bar %g); two-term operand model %.3g; the reference's own "
                  "fp32 vs fp64 %.3g" % (case, i, fr[case][i], MODULE_BAR, model, ref32))


# ---- the attention core alone ----------------------------------------------------------------------------------------------------------
def attention_native(q, k, v, scale, device):
    """q, k, v [NV, 12, ntok, 64] -> [NV, ntok, 12, 64] through the native core (host-packed operands)."""
    NV, _, ntok, _ = q.shape
    npad = ops.vit_npad(ntok)
    buf = packing.pack_vit_qkv(q * (scale * math.log2(math.e)), k, v, npad).to(device)
    out = ops.vit_attention(buf, NV, ntok, npad)
    return packing.unpack_tokens_split(out.cpu(), NV * npad, 768).reshape(NV, npad, 12, 64)[:, :ntok]


def attention_fp64(q, k, v, scale, split=False):
    return R.attention(q.double(), k.double(), v.double(), scale, split).transpose(1, 2)


def forced_rescale_inputs(ntok=75, seed=11):
    """Plain random q, k, v [2, 12, ntok, 64] except three heads in which one key is a multiple of a chosen query, scaled so that its
    score is exactly 40 nats at scale 1/8 against a crowd within a few nats: head 0 - key 32 (the first of the second key step) for query
    rows 3 and 40; head 1 - the LAST valid key for query rows 0 and ntok - 1; head 2 - every key before the last step is zero (a flat
    start: all scores 0, the running max does not move) and key 5 of the last step dominates for query row 17.  The query rows of a head
    that share a key are equal.  -> (q, k, v, {head: (query rows, key)})."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(2, 12, ntok, 64, generator=g) for _ in range(3))
    last0 = (ntok - 1) // 32 * 32
    spikes = {0: ((3, 40), 32), 1: ((0, ntok - 1), ntok - 1), 2: ((17,), last0 + 5)}
    k[:, 2, :last0] = 0.0
    for h, (rows, kj) in spikes.items():
        for qi in rows[1:]:
            q[:, h, qi] = q[:, h, rows[0]]
        qr = q[:, h, rows[0]]
        k[:, h, kj] = qr * (40.0 / (0.125 * (qr * qr).sum(-1, keepdim=True)))
    return q, k, v, spikes


def check_forced_rescale(device):
    """A rescale that bounded random data never exercises needs an input that forces it: rows whose running max jumps by >= 30 nats at a chosen key step, compared on the FULL tensor
    against fp64.  The margins are chosen so that the format alone (the split_operands restatement of the same inputs) stays within
    LAYER_BAR: checked here on the CPU (measured 8.8e-6 x max(1, max|ref|); the native core 1.15e-5)."""
    q, k, v, spikes = forced_rescale_inputs()
    scale = 0.125
    s = torch.einsum("vhqd,vhkd->vhqk", q.double(), k.double()) * scale
    for h, (rows, kj) in spikes.items():
        for qi in rows:
            row = s[:, h, qi].clone()
            top = row[:, kj].clone()
            row[:, kj] = -1e9
            assert float((top - row.amax(-1)).min()) >= 30.0, (h, qi, kj)
    want = attention_fp64(q, k, v, scale)
    fmt = close(attention_fp64(q, k, v, scale, split=True), want, LAYER_BAR, "the format alone")
    got = close(attention_native(q, k, v, scale, device), want, LAYER_BAR, "forced rescale")
    return got, fmt


@pytest.mark.parametrize("ntok", [1, 16, 17, 32, 33, 75])
def test_attention_against_fp64(emu, ntok):
    """Token counts 1, 16, 17, the key step 32 and one past it, and 75 = three key steps with a ragged last one; both scale forms."""
    g = torch.Generator().manual_seed(ntok)
    q, k, v = (torch.randn(2, 12, ntok, 64, generator=g) for _ in range(3))
    for scale in (R.softmax_scale(ntok), R.softmax_scale(max(ntok, 2), "entropy_invariance", 762)):
        want = attention_fp64(q, k, v, scale)
        err = close(attention_native(q, k, v, scale, emu), want, LAYER_BAR, (ntok, scale))
        print("attention %d tokens, scale %.4f: %.3g x max(1, max|ref|)" % (ntok, scale, err))


def test_attention_views_are_independent(emu):
    """Several views in one call equal per-view calls, bit for bit; two runs are bit-identical."""
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(3, 12, 41, 64, generator=g) for _ in range(3))
    both = attention_native(q, k, v, 0.125, emu)
    assert torch.equal(both, attention_native(q, k, v, 0.125, emu))
    for i in range(3):
        assert torch.equal(attention_native(q[i:i + 1], k[i:i + 1], v[i:i + 1], 0.125, emu)[0], both[i]), i


def test_attention_forced_rescale(emu):
    got, fmt = check_forced_rescale(emu)
    print("forced rescale: native %.3g, the format alone %.3g x max(1, max|ref|) (bar %g)" % (got, fmt, LAYER_BAR))


def test_qkv_epilogue_writes_the_attention_operands(emu):
    """The qkv projection's epilogue (bias, q pre-scale, per-head packed q | k, transposed v) writes, bit for bit, what the host packer
    builds from the same fp32 values - so the attention tests above exercise the layout the module uses."""
    g = torch.Generator().manual_seed(8)
    NV, ntok = 2, 19
    npad = ops.vit_npad(ntok)
    w = torch.randn(2304, 768, generator=g) * 0.03
    b = torch.randn(2304, generator=g)
    x = torch.zeros(NV, npad, 768)
    x[:, :ntok] = torch.randn(NV, ntok, 768, generator=g)
    xp = packing.pack_tokens_split(x.reshape(-1, 768)).view(torch.uint8)
    got = ops.vit_qkv(xp, packing.pack_linear_bf16x3(w), b, NV, npad, 1.0)
    # fp32 values of the projection, from the plain fp32 epilogue of the same GEMM (N = 768 per call)
    cols = [ops.vitdec_linear(xp, NV * npad, packing.pack_linear_bf16x3(w[i * 768:(i + 1) * 768]), 768, 768, ops.VITDEC_EPI_RESID,
                              bias=b[i * 768:(i + 1) * 768].contiguous(), gamma=torch.ones(768), residual=torch.zeros(NV * npad, 768))
            for i in range(3)]
    q, k, v = (c.reshape(NV, npad, 12, 64).permute(0, 2, 1, 3).contiguous() for c in cols)
    assert torch.equal(got, packing.pack_vit_qkv(q, k, v, npad))


# ---- position embedding --------------------------------------------------------------------------------------------------------------
def test_position_table_and_cache():
    """The cached table equals the reference recipe (restated in vit_ref.py) at 4 x 6, 5 x 3, 36 x 48, 34 x 60 and 37 x 37 (the shortcut:
    the table itself); F28's token captures pin the two fixture grids against the reference's own run (test_entry_points_against_f28,
    test_restatement_pinned_to_f28).  A tall and a wide grid differ, so the axis order is pinned.  The table is built once per grid and
    parameter version."""
    fx = f28()
    m = module(fx)
    pe = f28_weights(fx)["pos_embed"]
    for gh, gw in ((4, 6), (5, 3), (36, 48), (34, 60), (37, 37)):
        pos, cls_pos = m._positions(torch.device("cpu"), gh, gw)
        want = R.position_table(pe, gh, gw)
        assert pos.dtype == torch.float32 and pos.shape == (gh * gw + 1, 768) and torch.equal(pos, want), (gh, gw)
        assert torch.equal(cls_pos, m.cls_token.reshape(-1) + want[0])
        assert m._positions(torch.device("cpu"), gh, gw)[0] is pos                       # cached
    assert torch.equal(m._positions(torch.device("cpu"), 37, 37)[0], pe[0])
    tall, wide = m._positions(torch.device("cpu"), 5, 3)[0], m._positions(torch.device("cpu"), 3, 5)[0]
    assert not torch.allclose(tall[1:].reshape(5, 3, 768).transpose(0, 1), wide[1:].reshape(3, 5, 768), atol=1e-3)
    old = m._positions(torch.device("cpu"), 4, 6)[0]
    with torch.no_grad():
        m.pos_embed.mul_(2.0)
    new = m._positions(torch.device("cpu"), 4, 6)[0]
    assert new is not old and torch.allclose(new, 2 * old, atol=1e-5)


# ---- module contract -----------------------------------------------------------------------------------------------------------------
def test_state_dict_names_match_the_reference():
    """The 175 keys and their shapes are the reference's (F28 stores the reference module's manifest), so a checkpoint's vit.* entries
    load with strict=True and round-trip unchanged; every parameter is frozen."""
    fx = f28()
    ref = {k: tuple(json.loads(s)) for k, s in zip(fx["vit.keys"], fx["vit.shapes"])}
    mod = vit_base(**f28_config(fx))
    assert len(ref) == 175 and {k: tuple(v.shape) for k, v in mod.state_dict().items()} == ref
    assert ref["pos_embed"] == (1, 1370, 768) and ref["blocks.11.attn.qkv.bias"] == (2304,) and ref["mask_token"] == (1, 768)
    assert all(not p.requires_grad for p in mod.parameters())
    assert (mod.embed_dim, mod.patch_size, mod.num_heads, mod.n_blocks) == (768, 14, 12, 12)
    sd = f28_weights(fx)
    mod.load_state_dict(sd, strict=True)
    again = vit_base(**f28_config(fx))
    again.load_state_dict(mod.state_dict(), strict=True)
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k]), k


class _RefBlock(nn.Module):
    def __init__(self, d=768):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(d, eps=1e-6), nn.LayerNorm(d, eps=1e-6)
        self.attn = nn.Module()
        self.attn.qkv, self.attn.proj = nn.Linear(d, 3 * d), nn.Linear(d, d)
        self.attn.softmax_scale, self.attn.train_avg_length = "entropy_invariance", 500
        self.ls1, self.ls2 = nn.Module(), nn.Module()
        self.ls1.gamma, self.ls2.gamma = nn.Parameter(torch.ones(d)), nn.Parameter(torch.ones(d))
        self.mlp = nn.Module()
        self.mlp.fc1, self.mlp.fc2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)
        self.drop_path1, self.drop_path2 = nn.Identity(), nn.Identity()


class _StandIn(nn.Module):
    """A network with the reference's attribute names; vit is built from reference-named plain modules (depth 3)."""

    def __init__(self):
        super().__init__()
        v = self.vit = nn.Module()
        v.cls_token, v.pos_embed, v.mask_token = nn.Parameter(torch.zeros(1, 1, 768)), nn.Parameter(torch.zeros(1, 17, 768)), nn.Parameter(torch.zeros(1, 768))
        v.patch_embed = nn.Module()
        v.patch_embed.proj = nn.Conv2d(3, 768, 14, stride=14)
        v.blocks = nn.ModuleList([_RefBlock() for _ in range(3)])
        v.norm = nn.LayerNorm(768, eps=1e-6)
        v.cross_interval_layers, v.dino_layer_idxs, v.num_heads = 3, [0, 1], 12
        self.encoder, self.decoder = nn.Conv2d(3, 8, 3), nn.Conv2d(8, 8, 3)
        self.decoder_vit, self.FMT_module = nn.Linear(4, 4), nn.Linear(4, 4)


def test_patch_vit_swaps_only_the_vit():
    net = _StandIn()
    net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 4), strict=True)
    net = net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    others = {n: getattr(net, n) for n in ("encoder", "decoder", "decoder_vit", "FMT_module")}
    assert patch_vit(net) is net
    new = net.vit
    assert isinstance(new, DinoVisionTransformer) and not new.training and all(not p.requires_grad for p in new.parameters())
    assert (new.cross_interval_layers, new.dino_layer_idxs, new.softmax_scale, new.train_avg_length) == (3, [0, 1], "entropy_invariance", 500)
    assert (new.embed_dim, new.patch_size, new.num_heads, new.n_blocks) == (768, 14, 12, 3)
    for n, mod in others.items():
        assert getattr(net, n) is mod
    after = net.state_dict()
    assert sorted(after) == sorted(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert patch_vit(_StandIn().train()).vit.training                     # the mode is carried over
    net = _StandIn()
    del net.vit.blocks[0].ls1
    with pytest.raises(NotImplementedError, match="ls1.gamma"):
        patch_vit(net)
    net = _StandIn()
    net.vit.blocks[1].drop_path1 = nn.Module()
    net.vit.blocks[1].drop_path1.drop_prob = 0.1
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        patch_vit(net)


def test_patch_all_is_the_chain(monkeypatch):
    from mvsformerplusplus_amd import cascade, features, fmt, vit_decoder
    order = []

    def step(name):
        def f(model):
            order.append(name)
            return model
        return f
    monkeypatch.setattr(cascade, "patch_model", step("model"))
    monkeypatch.setattr(features, "patch_fpn", step("fpn"))
    monkeypatch.setattr(fmt, "patch_fmt", step("fmt"))
    monkeypatch.setattr(vit_decoder, "patch_vit_decoder", step("vit_decoder"))
    monkeypatch.setattr(V, "patch_vit", step("vit"))
    net = nn.Module()
    assert patch_all(net) is net and order == ["model", "fpn", "fmt", "vit_decoder", "vit"]
    import mvsformerplusplus_amd as pkg
    assert pkg.patch_all is patch_all and pkg.patch_vit is patch_vit and pkg.DinoVisionTransformer is DinoVisionTransformer


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def small(**changes):
    """A depth-3 module (one block per level) with seeded weights: the cheap stand-in of the input-form and refusal tests."""
    kw = dict(img_size=56, patch_size=14, init_values=1.0, block_chunks=0, ffn_layer="mlp", depth=3, cross_interval_layers=3)
    kw.update(changes)
    m = vit_base(**kw)
    sd = synth.seeded_state_dict(synth.state_dict_manifest(m.state_dict()), 5)
    g = torch.Generator().manual_seed(6)
    sd["pos_embed"], sd["cls_token"] = torch.randn(1, 17, 768, generator=g), torch.randn(1, 1, 768, generator=g)
    m.load_state_dict(sd, strict=True)
    return m.eval()


def test_refusals(emu):
    base = dict(img_size=518, patch_size=14, init_values=1.0, block_chunks=0, ffn_layer="mlp", cross_interval_layers=3)
    for bad, match in ((dict(embed_dim=384), "embed_dim"), (dict(num_heads=6), "num_heads"), (dict(patch_size=16), "patch_size"),
                       (dict(in_chans=1), "in_chans"), (dict(ffn_layer="swiglu"), "ffn_layer"), (dict(init_values=None), "init_values"),
                       (dict(init_values=0), "init_values"), (dict(block_chunks=1), "block_chunks"), (dict(qkv_bias=False), "qkv_bias"),
                       (dict(proj_bias=False), "proj_bias"), (dict(ffn_bias=False), "ffn_bias"), (dict(drop_path_rate=0.1), "drop_path_rate"),
                       (dict(cross_interval_layers=5), "cross_interval_layers")):
        with pytest.raises(NotImplementedError, match=match):
            DinoVisionTransformer(**dict(base, **bad))
    DinoVisionTransformer(**dict(base, use_flash2_dino=True, softmax_scale="entropy_invariance", train_avg_length=762, depth=6))   # accepted
    m = small()
    x = torch.randn(1, 3, 14, 28, generator=torch.Generator().manual_seed(1))
    with pytest.raises(NotImplementedError, match="masks"):
        m.forward_interval_features(x, masks=torch.zeros(1, 2, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="list"):
        m.forward_interval_features([x])
    for name in ("forward", "forward_features", "forward_features_list", "forward_features_with_idxs", "get_intermediate_layers"):
        with pytest.raises(NotImplementedError, match="forward_interval_features"):
            getattr(m, name)(x)
    with pytest.raises(ValueError, match="multiples of 14"):
        m.forward_interval_features(torch.zeros(1, 3, 15, 28))
    with pytest.raises(RuntimeError, match="no autograd"):
        m.forward_interval_features(x.clone().requires_grad_(True))
    with torch.no_grad():
        ev = m.forward_interval_features(x.clone().requires_grad_(True))      # grad disabled: accepted
    tr = m.train().forward_interval_features(x)                               # train() mode: accepted, the same arithmetic
    assert len(tr) == 3 and all(torch.equal(a, b) for a, b in zip(tr, ev)) and tr[0].shape == (1, 2, 768) and not tr[0].requires_grad
    # dino_layer_idxs replace the interval rule
    mi = small(dino_layer_idxs=[1])
    mi.load_state_dict(m.state_dict(), strict=True)
    got = mi.eval().forward_interval_features(x)
    assert len(got) == 2 and torch.equal(got[0], ev[1]) and torch.equal(got[1], ev[2])
    # the C ABI: a loud refusal of anything not built
    L = _lib.lib()
    buf = torch.zeros(L.mvs_vit_qkv_bytes(1, 32), dtype=torch.uint8)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vit_attention(buf, 1, 5, 32, heads=8)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vit_attention(buf, 1, 5, 32, head_dim=16)
    # the wrappers: layouts and sizes before any pointer is taken
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.vit_attention(buf, 1, 5, 16)
    with pytest.raises(ValueError, match="mvs_vit_qkv_bytes"):
        ops.vit_attention(buf[:-16], 1, 5, 32)
    with pytest.raises(ValueError, match="multiples of 14"):
        ops.vit_patches(torch.zeros(1, 3, 14, 20))
    with pytest.raises(ValueError, match="multiples of 14"):
        ops.vit_patches(torch.zeros(1, 4, 14, 14))
    with pytest.raises(ValueError, match="residual stream"):
        ops.vit_rows(torch.zeros(4, 384), norm=(torch.zeros(768), torch.zeros(768)))
    with pytest.raises(ValueError, match="exactly one"):
        ops.vit_rows(torch.zeros(4, 768))
    a = torch.zeros(L.mvs_vitdec_packed_bytes(32, 768), dtype=torch.uint8)
    with pytest.raises(ValueError, match="pack_linear_bf16x3"):
        ops.vit_qkv(a, packing.pack_linear_bf16x3(torch.zeros(768, 768)), torch.zeros(2304), 1, 32, 1.0)
    with pytest.raises(ValueError, match="2304 elements"):
        ops.vit_qkv(a, packing.pack_linear_bf16x3(torch.zeros(2304, 768)), torch.zeros(768), 1, 32, 1.0)
    with pytest.raises(ValueError, match="pack_vit_patch_embed"):
        ops.vit_embed(torch.zeros(L.mvs_vitdec_packed_bytes(2, 640), dtype=torch.uint8), torch.zeros(8, dtype=torch.bfloat16), torch.zeros(768),
                      torch.zeros(3, 768), torch.zeros(768), 1, 2)


def test_host_tensors_are_refused(monkeypatch, emu_lib):
    """There is no CPU route: with the device requirement in force (the product setting) a host tensor raises before any launch.  The
    emulated library only stands in for the size queries that come before the first pointer is taken."""
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    assert _lib._REQUIRE_DEVICE
    m = small()
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        m.forward_interval_features(torch.zeros(1, 3, 14, 28))


def test_input_forms(emu):
    """A batch equals per-view calls and a channels-last image equals its contiguous copy through the whole (depth-3) module; bf16 and
    fp16 images equal their widening and a sliced image equals its contiguous copy at the tokens, the only place where the image's
    dtype and strides are read (the rest of the chain is the same launches on the same values) - all bit for bit."""
    m = small()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 14, 42, generator=g)
    both = m.forward_interval_features(x)
    assert len(both) == 3 and both[0].shape == (2, 3, 768)
    for i in range(2):
        one = m.forward_interval_features(x[i:i + 1])
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, both)), i
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and all(torch.equal(a, b) for a, b in zip(m.forward_interval_features(cl), both))
    tokens = lambda t: m.prepare_tokens(t)[0]
    big = torch.randn(2, 4, 30, 50, generator=g)
    sl = big[:, 1:, 2:16, 5:47]
    assert not sl.is_contiguous() and sl.shape == x.shape and torch.equal(tokens(sl), tokens(sl.contiguous()))
    assert torch.equal(tokens(cl), tokens(x))
    for dt in (torch.bfloat16, torch.float16):
        xl = x.to(dt)
        assert tokens(xl).dtype == torch.float32 and torch.equal(tokens(xl), tokens(xl.float())), dt
    a, b = m.forward_interval_features(x[:1].to(torch.bfloat16)), m.forward_interval_features(x[:1].to(torch.bfloat16).float())
    assert all(torch.equal(s, t) for s, t in zip(a, b))
