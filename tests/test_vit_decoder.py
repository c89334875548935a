"""CPU: the native CrossVITDecoder (mvsformerplusplus_amd.vit_decoder, csrc/vitdec_kernels.hip) on the host emulator against fixture F27
(the reference's own CrossVITDecoder, tests/golden/make_golden_vit_decoder.py) and the fp64 restatement (tests/vit_decoder_ref.py); the
module contract (state-dict names, patch_vit_decoder), the packed layouts and every refusal.

Bars (the project's, as tests/test_fpn.py and tests/test_fmt.py use them for the same split-bf16 arithmetic): LAYER_BAR for one entry
point on its captured input, MODULE_BAR for the whole module.  They were set for K <= 576; here K reaches 3072 (fc2) and 6912 (proj).
Measured on the emulator: entry points 9.73e-6 x max(1, max|ref|); whole module 1.08e-5 (case a) / 1.29e-5 (case b) of the output's range.
The error of the FORMAT alone (the fp64 restatement with every GEMM operand rounded to hi + lo bf16, 2^-17 per operand) is 8.1e-6 / 1.28e-5
of the range, the reference's own fp32 run sits 1.5e-6 / 1.8e-6 from fp64: the project's bars hold with an order of magnitude to spare, so
no new bar was derived.  On an MI355X (tests/test_vit_decoder_gpu.py): entry points 8.38e-6, module 1.11e-5 / 1.20e-5, both full sizes at
V = 5 against fp64 1.03e-5.  The tests print their figures (pytest -s)."""
import hashlib
import json

import pytest
import torch
import torch.nn as nn

import vit_decoder_ref as R
from conftest import load_golden
from mvsformerplusplus_amd import _lib, ops, packing, synth
from mvsformerplusplus_amd.vit_decoder import CrossVITDecoder, patch_vit_decoder

LAYER_BAR = 3e-5          # per entry point: x max(1, max|ref|)          (tests/test_fpn.py, tests/test_fmt.py)
MODULE_BAR = 2e-4         # whole module: x the output's range
F27_FILES = ("f27_vitdec_a_in.npz", "f27_vitdec_a_ref.npz", "f27_vitdec_a_src.npz", "f27_vitdec_a_head.npz", "f27_vitdec_b.npz")
SHAPE_A, SHAPE_B = [1, 3, 4, 6, 768], [2, 2, 3, 5, 768]


def f27():
    fx = {}
    for name in F27_FILES:
        fx.update({k: v for k, v in load_golden(name).items() if k != "__name__"})
    return fx


def f27_args(fx):
    return json.loads(fx["vitdec.config"])


def f27_weights(fx):
    """The state dict F27 was generated with, rebuilt from its manifest + seed and checked against the SHA-256 stored in F27."""
    shapes = [tuple(json.loads(s)) for s in fx["vitdec.shapes"]]
    sd = synth.seeded_state_dict(dict(zip(fx["vitdec.keys"], shapes)), int(fx["vitdec.seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == fx["vitdec.sha256"], "torch / numpy generator changed: regenerate F27 (tests/golden/make_golden_vit_decoder.py)"
    return sd


def module(fx, device="cpu"):
    m = CrossVITDecoder(f27_args(fx))
    m.load_state_dict(f27_weights(fx), strict=True)
    return m.eval().to(device)


def inputs(fx, case, device="cpu"):
    return [fx["%s/x%d" % (case, i)].to(device) for i in range(3)]


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


def planar_to_packed(t, device):
    """[N, C, H, W] -> the packed-split token tensor of the map (host packer)."""
    N, C = t.shape[:2]
    return packing.pack_tokens_split(t.permute(0, 2, 3, 1).reshape(-1, C)).view(torch.uint8).to(device)


def packed_to_planar(p, N, C, H, W):
    return packing.unpack_tokens_split(p.cpu(), N * H * W, C).reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous()


def run_block(m, p, kind, i, x, key, device):
    """Block (kind, i) on tokens x [N, n, 768] with the keys / values of `key` [Nk, n, 768] (None = self attention) -> [N, n, 768]."""
    pb = p["%s%d" % (kind, i)]
    N, n = x.shape[:2]
    cur, _, cur_n = ops.vitdec_rows(x.to(device).unsqueeze(0), 0, N, ln=(pb["norm1.weight"], pb["norm1.bias"]))
    if key is None:
        kvp, Nk = cur_n, N
    else:
        Nk = key.shape[0]
        kvp = ops.vitdec_rows(key.to(device).unsqueeze(0), 0, Nk, want_x=False, want_packed=True)[1]
    return m.block(pb, cur, cur_n, kvp, N, Nk, n, N // Nk).reshape(N, n, 768).cpu()


def check_entry_points(fx, device):
    """Every native entry point against F27 case a, each on its captured input: both self blocks (reference view), the three cross
    blocks (source view 1, the summary from the captured reference features), the AAS mix + norm step (reference and source view),
    proj, upsampler0, upsampler1."""
    m = module(fx, device)
    p = m._params(torch.device(device))
    refs = [fx["a/x0"][:, 0], fx["a/ref/feat1"], fx["a/ref/feat2"]]
    worst = 0.0
    for i in range(2):
        got = run_block(m, p, "self", i, fx["a/ref/blk%d_in" % i], None, device)
        worst = max(worst, close(got, fx["a/ref/blk%d_out" % i], LAYER_BAR, ("self block", i)))
    for i in range(3):
        got = run_block(m, p, "cross", i, fx["a/src/blk%d_in" % i], refs[i], device)
        worst = max(worst, close(got, fx["a/src/blk%d_out" % i], LAYER_BAR, ("cross block", i)))
    for i in (1, 2):
        mix = dict(prev_value=p["pv%d" % (i - 1)], mix=p["mix%d" % (i - 1)])
        x = ops.vitdec_rows(fx["a/x%d" % i].to(device), 0, 1, prev=fx["a/ref/blk%d_out" % (i - 1)][0].to(device).contiguous(), **mix)[0]
        worst = max(worst, close(x.cpu().reshape(1, 24, 768), refs[i], LAYER_BAR, ("AAS + norm, reference view", i)))
        x, xp, _ = ops.vitdec_rows(fx["a/x%d" % i].to(device), 1, 1, prev=fx["a/src/blk%d_out" % (i - 1)][0].to(device).contiguous(),
                                   want_packed=True, **mix)
        worst = max(worst, close(x.cpu().reshape(1, 24, 768), fx["a/src/blk%d_in" % i], LAYER_BAR, ("AAS + norm, source view", i)))
        close(packing.unpack_tokens_split(xp.cpu(), 24, 768), x.cpu(), 2.0 ** -16, "packed-split of the same rows")
    tok = ops.vitdec_rows(fx["a/tokens"].to(device).unsqueeze(0), 0, 3, want_x=False, want_packed=True)[1]
    got = ops.vitdec_conv(tok, *p["proj"], ops.VITDEC_PROJ, 3, 4, 6)
    worst = max(worst, close(packed_to_planar(got, 3, 256, 4, 6), fx["a/proj"], LAYER_BAR, "proj"))
    got = ops.vitdec_conv(tok, *p["proj"], ops.VITDEC_PROJ, 3, 4, 6, planar=True)
    worst = max(worst, close(got.cpu(), fx["a/proj"], LAYER_BAR, "proj planar"))
    got = ops.vitdec_conv(planar_to_packed(fx["a/proj"], device), *p["upsampler0"], ops.VITDEC_UP0, 3, 4, 6)
    worst = max(worst, close(packed_to_planar(got, 3, 128, 8, 12), fx["a/upsampler0"], LAYER_BAR, "upsampler0"))
    got = ops.vitdec_conv(planar_to_packed(fx["a/upsampler0"], device), *p["upsampler1"], ops.VITDEC_UP1, 3, 8, 12, planar=True)
    worst = max(worst, close(got.cpu(), fx["a/upsampler1"], LAYER_BAR, "upsampler1"))
    return worst


def check_module(fx, device):
    """Whole module, cases a (1 x 3 views, 4 x 6 tokens) and b (2 x 2 views, 15 tokens, levels 1 and 2 x30) -> per case the measured
    fraction of the output's range."""
    m = module(fx, device)
    out = {}
    with torch.no_grad():
        for case, shape in (("a", SHAPE_A), ("b", SHAPE_B)):
            want = fx["a/upsampler1"] if case == "a" else fx["b/out"]
            got = m(inputs(fx, case, device), vit_shape=shape)
            assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape
            out[case] = within_range(got.cpu(), want, MODULE_BAR, case)
    return out


def test_restatement_pinned_to_f27():
    """tests/vit_decoder_ref.py (fp64) reproduces every capture of F27 at 1e-5 x max(1, max|ref|): the oracle at sizes the fixture lacks."""
    fx = f27()
    sd = f27_weights(fx)
    cap = {}
    out = R.vit_decoder(inputs(fx, "a"), sd, SHAPE_A, capture=cap)
    close(out, fx["a/upsampler1"], 1e-5, "a out")
    for i in range(2):
        close(cap[("self", i)][0], fx["a/ref/blk%d_in" % i], 1e-5, ("ref in", i))
        close(cap[("self", i)][2], fx["a/ref/blk%d_out" % i], 1e-5, ("ref out", i))
    for i in range(3):
        close(cap[("cross", 1, i)][0], fx["a/src/blk%d_in" % i], 1e-5, ("src in", i))
        close(cap[("cross", 1, i)][2], fx["a/src/blk%d_out" % i], 1e-5, ("src out", i))
    for i in (1, 2):
        close(cap["refs"][i], fx["a/ref/feat%d" % i], 1e-5, ("feat", i))
    close(cap["tokens"], fx["a/tokens"], 1e-5, "tokens")
    for name in ("proj", "upsampler0", "upsampler1"):
        close(cap[name], fx["a/" + name], 1e-5, name)
    close(R.vit_decoder(inputs(fx, "b"), sd, SHAPE_B), fx["b/out"], 1e-5, "b out")
    assert fx["a/x0"].shape == (1, 3, 24, 768) and fx["b/x2"].shape == (2, 2, 15, 768) and fx["b/out"].shape == (4, 64, 12, 20)


def test_entry_points_against_f27(emu):
    worst = check_entry_points(f27(), emu)
    print("vitdec entry points vs F27: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (worst, LAYER_BAR))


def test_module_against_f27(emu):
    fx = f27()
    fr = check_module(fx, emu)
    sd = f27_weights(fx)
    for case, shape in (("a", SHAPE_A), ("b", SHAPE_B)):
        want = fx["a/upsampler1"] if case == "a" else fx["b/out"]
        rng = float(want.max() - want.min())
        o64 = R.vit_decoder(inputs(fx, case), sd, shape)
        model = float((R.vit_decoder(inputs(fx, case), sd, shape, split_operands=True) - o64).abs().max()) / rng
        ref32 = float((want.double() - o64).abs().max()) / rng
        print("CrossVITDecoder vs F27 case %s: |error| = %.3g of the output's range (bar %g); two-term operand model %.3g; the reference's "
              "own fp32 vs fp64 %.3g" % (case, fr[case], MODULE_BAR, model, ref32))


def test_summary_once_and_batched_views(emu):
    """A cross block's key/value summary depends on the reference view only: computed once and shared by the source views (what the
    module does) it gives bit for bit what one call per source view gives; a batch of views equals per-view calls."""
    fx = f27()
    m = module(fx)
    p = m._params(torch.device("cpu"))
    g = torch.Generator().manual_seed(5)
    n = 7
    ref = torch.randn(2, n, 768, generator=g)                      # two batch elements
    src = torch.randn(4, n, 768, generator=g)                      # two source views each
    batched = run_block(m, p, "cross", 1, src, ref, "cpu")
    for i in range(4):
        one = run_block(m, p, "cross", 1, src[i:i + 1], ref[i // 2:i // 2 + 1], "cpu")
        assert torch.equal(one[0], batched[i]), i
    pb = p["cross1"]
    kvp = ops.vitdec_rows(ref.unsqueeze(0), 0, 2, want_x=False, want_packed=True)[1]
    both = ops.vitdec_kv(ops.vitdec_linear(kvp, 2 * n, pb["kv"], 768, 1536, ops.VITDEC_EPI_F32, elu_cols=768), 2, n)
    for b in range(2):
        kv1 = ops.vitdec_rows(ref[b:b + 1].unsqueeze(0), 0, 1, want_x=False, want_packed=True)[1]
        one = ops.vitdec_kv(ops.vitdec_linear(kv1, n, pb["kv"], 768, 1536, ops.VITDEC_EPI_F32, elu_cols=768), 1, n)
        assert torch.equal(one[0], both[b]), b
    # the summary against fp64: KV_h[d][m] = sum_s k[s][d] v[s][m], ksum_h[d] = sum_s k[s][d]
    kv = ops.vitdec_linear(kvp, 2 * n, pb["kv"], 768, 1536, ops.VITDEC_EPI_F32, elu_cols=768).double().reshape(2, n, 2, 12, 64)
    want = torch.einsum("bshd,bshm->bhdm", kv[:, :, 0], kv[:, :, 1])
    close(both[:, :, :4096].reshape(2, 12, 64, 64), want, 1e-6, "KV_h")
    close(both[:, :, 4096:], kv[:, :, 0].sum(1), 1e-6, "ksum_h")


def test_batches_views_and_input_forms(emu):
    """Batched equals per batch element; V = 1 equals view 0 of a larger call; bf16 input equals its widening; a strided x[:, 1:]-style
    input (row stride 768, view stride (n + 1) 768: the ViT's output minus its class token) equals its contiguous copy - all bit for
    bit."""
    fx = f27()
    m = module(fx)
    g = torch.Generator().manual_seed(9)
    B, V, h, w = 2, 2, 1, 5
    n = h * w
    with_cls = [torch.randn(B * V, n + 1, 768, generator=g) for _ in range(3)]
    strided = [t[:, 1:].unflatten(0, (B, V)) for t in with_cls]
    assert not strided[0].is_contiguous() and strided[0].stride() == (V * (n + 1) * 768, (n + 1) * 768, 768, 1)
    dense = [t.contiguous() for t in strided]
    shape = [B, V, h, w, 768]
    with torch.no_grad():
        both = m(dense, vit_shape=shape)
        assert torch.equal(m(strided, vit_shape=shape), both)
        for b in range(B):
            one = m([t[b:b + 1] for t in dense], vit_shape=[1, V, h, w, 768])
            assert torch.equal(one, both[b * V:(b + 1) * V]), b
        ref_only = m([t[:, :1] for t in dense], vit_shape=[B, 1, h, w, 768])
        assert torch.equal(ref_only, both[0::V])
        xb = [t.to(torch.bfloat16) for t in dense]
        a, c = m(xb, vit_shape=shape), m([t.float() for t in xb], vit_shape=shape)
        assert a.dtype == torch.float32 and torch.equal(a, c)
        xh = [t[:1].to(torch.float16) for t in dense]               # fp16 likewise (one batch element: the shared-rows route of the keys)
        a, c = m(xh, vit_shape=[1, V, h, w, 768]), m([t.float() for t in xh], vit_shape=[1, V, h, w, 768])
        assert a.dtype == torch.float32 and torch.equal(a, c)
        # an expanded view (row stride 0) is materialised by the module, and refused by the wrapper itself
        ex = [t[:1, :, :1].expand(1, V, n, 768) for t in dense]
        assert torch.equal(m(ex, vit_shape=[1, V, h, w, 768]), m([t.contiguous() for t in ex], vit_shape=[1, V, h, w, 768]))
        with pytest.raises(ValueError, match="do not overlap"):
            ops.vitdec_rows(ex[0], 0, 1)


def test_state_dict_names_match_the_reference():
    """The 102 keys and their shapes are the reference's (F27 stores the reference module's manifest), so a checkpoint's decoder_vit.*
    entries load with strict=True and round-trip unchanged."""
    fx = f27()
    ref = {k: tuple(json.loads(s)) for k, s in zip(fx["vitdec.keys"], fx["vitdec.shapes"])}
    mod = CrossVITDecoder(f27_args(fx))
    assert len(ref) == 102 and {k: tuple(v.shape) for k, v in mod.state_dict().items()} == ref
    assert ref["prev_values.0"] == () and ref["proj.0.weight"] == (256, 768, 3, 3) and ref["upsampler1.0.weight"] == (128, 64, 4, 4)
    sd = f27_weights(fx)
    mod.load_state_dict(sd, strict=True)
    again = CrossVITDecoder(f27_args(fx))
    again.load_state_dict(mod.state_dict(), strict=True)
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_pack_tokens_split_layout():
    """packed[row >> 4][k >> 5][hi|lo][((k >> 3) & 3) * 16 + (row & 15)][k & 7] (small integers: hi exact, lo zero); rows padded to 16."""
    x = (torch.arange(20 * 64, dtype=torch.float32).reshape(20, 64) % 251) - 125
    p = packing.pack_tokens_split(x).float().reshape(2, 2, 2, 4, 16, 8)
    assert float(p[:, :, 1].abs().max()) == 0.0 and float(p[1, :, :, :, 4:].abs().max()) == 0.0
    for row, k in ((0, 0), (19, 63), (7, 41), (16, 8), (15, 31)):
        assert float(p[row >> 4, k >> 5, 0, (k >> 3) & 3, row & 15, k & 7]) == float(x[row, k])
    assert torch.equal(packing.unpack_tokens_split(packing.pack_tokens_split(x), 20, 64), x)
    y = torch.randn(5, 32, generator=torch.Generator().manual_seed(1))
    assert float((packing.unpack_tokens_split(packing.pack_tokens_split(y).view(torch.uint8), 5, 32) - y).abs().max()) <= 2.0 ** -16 * float(y.abs().max())


def _bn(c):
    return {"weight": torch.ones(c), "bias": torch.zeros(c), "running_mean": torch.zeros(c), "running_var": torch.ones(c), "eps": 0.0}


def test_pack_vitdec_conv_layout():
    """column (ky * 3 + kx) * Cin + c of the [Cout, 9 Cin] matrix, then pack_linear_bf16x3: packed[step][mb][hi|lo][g * 16 + j][e] =
    M[16 mb + j][32 step + 8 g + e]; the folded bias is (b - mean) * scale + beta."""
    w = ((torch.arange(128 * 64 * 9, dtype=torch.float32).reshape(128, 64, 3, 3) * 7) % 253) - 126
    b = torch.arange(128, dtype=torch.float32)
    p, bias = packing.pack_vitdec_conv(w, b, _bn(128))
    p = p.float().reshape(18, 8, 2, 4, 16, 8)
    assert float(p[:, :, 1].abs().max()) == 0.0 and torch.equal(bias, b)
    for co, c, ky, kx in ((0, 0, 0, 0), (127, 63, 2, 2), (17, 40, 1, 2), (100, 9, 2, 0)):
        col = (ky * 3 + kx) * 64 + c
        assert float(p[col >> 5, co >> 4, 0, (col >> 3) & 3, co & 15, col & 7]) == float(w[co, c, ky, kx])
    bn = dict(_bn(128), weight=torch.full((128,), 2.0), running_mean=torch.full((128,), 3.0), bias=torch.full((128,), 0.5))
    p2, bias2 = packing.pack_vitdec_conv(w, b, bn)
    assert torch.equal(bias2, (b - 3.0) * 2.0 + 0.5) and torch.equal(p2.float(), 2 * packing.pack_vitdec_conv(w, b, _bn(128))[0].float())


def test_pack_vitdec_deconv_layout():
    """class cls = 2 py + px, column (2 ay + ax) * Cin + c holds w[c][co][1 - py + 2 ay][1 - px + 2 ax]; Cout zero-padded to 128."""
    w = ((torch.arange(64 * 64 * 16, dtype=torch.float32).reshape(64, 64, 4, 4) * 5) % 251) - 125
    p, bias = packing.pack_vitdec_deconv(w, torch.zeros(64), _bn(64))
    p = p.float().reshape(4, 8, 8, 2, 4, 16, 8)
    assert float(p[:, :, :, 1].abs().max()) == 0.0 and float(p[:, :, 4:].abs().max()) == 0.0 and bias.shape == (64,)
    for cls, co, c, ay, ax in ((0, 0, 0, 0, 0), (3, 63, 63, 1, 1), (1, 20, 33, 0, 1), (2, 5, 50, 1, 0)):
        py, px = cls >> 1, cls & 1
        col = (2 * ay + ax) * 64 + c
        assert float(p[cls, col >> 5, co >> 4, 0, (col >> 3) & 3, co & 15, col & 7]) == float(w[c, co, 1 - py + 2 * ay, 1 - px + 2 * ax])


def test_pack_vitdec_block_layout():
    sd = synth.seeded_state_dict({k: tuple(v.shape) for k, v in CrossVITDecoder(f27_args(f27())).self_attn_blocks[0].state_dict().items()}, 3)
    p = packing.pack_vitdec_block(sd)
    assert sorted(p) == sorted(("q", "kv", "proj", "fc1", "fc2") + packing.VITDEC_VECTORS)
    assert torch.equal(p["kv"], packing.pack_linear_bf16x3(torch.cat([sd["attn.k_proj.weight"], sd["attn.v_proj.weight"]])))
    assert torch.equal(p["fc2"], packing.pack_linear_bf16x3(sd["mlp.fc2.weight"])) and p["fc1"].numel() == 2 * 768 * 3072
    assert torch.equal(p["ls2.gamma"], sd["ls2.gamma"]) and p["mlp.fc1.bias"].shape == (3072,)


class _RefBlock(nn.Module):
    def __init__(self, d=768):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.attn = nn.Module()
        for n in ("q_proj", "k_proj", "v_proj"):
            setattr(self.attn, n, nn.Linear(d, d, bias=False))
        self.attn.proj = nn.Linear(d, d)
        self.ls1, self.ls2 = nn.Module(), nn.Module()
        self.ls1.gamma, self.ls2.gamma = nn.Parameter(torch.ones(d)), nn.Parameter(torch.ones(d))
        self.mlp = nn.Module()
        self.mlp.fc1, self.mlp.fc2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)
        self.post_norm, self.pre_norm_query = False, True         # CrossBlock's attributes as the shipped decoder_cfg sets them


class _StandIn(nn.Module):
    """A network with the reference's attribute names; decoder_vit is built from reference-named plain modules."""

    def __init__(self):
        super().__init__()
        d = self.decoder_vit = nn.Module()
        d.self_attn_blocks = nn.ModuleList([_RefBlock() for _ in range(2)])
        d.cross_attn_blocks = nn.ModuleList([_RefBlock() for _ in range(3)])
        d.norm_layers = nn.ModuleList([nn.LayerNorm(768, eps=1e-6) for _ in range(2)])
        d.prev_values = nn.ParameterList([nn.Parameter(torch.tensor(0.5)) for _ in range(2)])
        d.proj = nn.Sequential(nn.Conv2d(768, 256, 3, padding=1), nn.BatchNorm2d(256), nn.SiLU())
        d.upsampler0 = nn.Sequential(nn.ConvTranspose2d(256, 128, 4, stride=2, padding=1), nn.BatchNorm2d(128), nn.SiLU())
        d.upsampler1 = nn.Sequential(nn.ConvTranspose2d(128, 64, 4, stride=2, padding=1), nn.BatchNorm2d(64), nn.SiLU())
        d.no_combine_norm, d.self_cross_types = False, None
        d.decoder_cfg = {"attention_type": "Linear", "d_model": 768, "nhead": 12, "ffn_type": "ffn", "init_values": 1.0, "prev_values": 0.5}
        d.dino_cfg = {"cross_interval_layers": 3, "decoder_cfg": d.decoder_cfg}
        self.encoder, self.decoder = nn.Conv2d(3, 8, 3), nn.Conv2d(8, 8, 3)
        self.vit, self.FMT_module = nn.Linear(4, 4), nn.Linear(4, 4)
        self.fusions = nn.ModuleList([nn.Conv3d(8, 8, 3)])


def test_patch_vit_decoder_swaps_only_the_decoder():
    net = _StandIn()
    net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 4), strict=True)
    net = net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    others = {n: getattr(net, n) for n in ("encoder", "decoder", "vit", "FMT_module", "fusions")}
    assert patch_vit_decoder(net) is net
    assert isinstance(net.decoder_vit, CrossVITDecoder) and not net.decoder_vit.training
    for n, mod in others.items():
        assert getattr(net, n) is mod
    after = net.state_dict()
    assert sorted(after) == sorted(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert patch_vit_decoder(_StandIn().train()).decoder_vit.training     # train mode is carried over (and then refused at forward)


def _with(args, **changes):
    """arch.args with decoder_cfg / dino_cfg / top-level keys replaced (a key is routed to the dict that owns it)."""
    a = json.loads(json.dumps(args))
    for k, v in changes.items():
        if k in ("out_ch", "vit_ch"):
            a[k] = v
        elif k == "cross_interval_layers":
            a["dino_cfg"][k] = v
        else:
            a["dino_cfg"]["decoder_cfg"][k] = v
    return a


def test_refusals(emu):
    args = f27_args(f27())
    for bad, match in ((dict(attention_type="FLASH2"), "attention_type"), (dict(self_cross_types=["Linear", "FLASH2"]), "self_cross_types"),
                       (dict(d_model=384), "d_model"), (dict(nhead=8), "nhead"), (dict(vit_ch=1024), "vit_ch"), (dict(out_ch=32), "out_ch"),
                       (dict(ffn_type="glu"), "ffn_type"), (dict(init_values=None), "init_values"), (dict(post_norm=True), "post_norm"),
                       (dict(pre_norm_query=False), "pre_norm_query"), (dict(no_combine_norm=True), "no_combine_norm"),
                       (dict(cross_interval_layers=4), "cross_interval_layers")):
        with pytest.raises(NotImplementedError, match=match):
            CrossVITDecoder(_with(args, **bad))
    CrossVITDecoder(_with(args, softmax_scale="entropy_invariance", train_avg_length=1000, self_cross_types=["Linear", "Linear"]))    # accepted
    m = CrossVITDecoder(args)
    x = [torch.zeros(1, 2, 6, 768) for _ in range(3)]
    shape = [1, 2, 2, 3, 768]
    with pytest.raises(RuntimeError, match="reference's models/module.py"):
        m(x, vit_shape=shape)                                        # train() mode (a fresh module)
    m.eval()
    with pytest.raises(RuntimeError, match="no autograd"):
        m([x[0], x[1].clone().requires_grad_(True), x[2]], vit_shape=shape)
    with pytest.raises(ValueError, match="Fmats"):
        m(x, Fmats=torch.zeros(1), vit_shape=shape)
    with pytest.raises(ValueError, match="three"):
        m(x[:2], vit_shape=shape)
    with pytest.raises(ValueError, match="three"):
        m(x, vit_shape=[1, 2, 3, 3, 768])
    assert m(x, vit_shape=shape).shape == (2, 64, 8, 12)              # a tiny map runs (n = 6 tokens)
    # what the old module does is not in the state dict: patch_vit_decoder reads it from the blocks and the module
    for where, attr, value, match in (("block", "pre_norm_query", False, "pre_norm_query"), ("block", "post_norm", True, "post_norm"),
                                      ("module", "no_combine_norm", True, "no_combine_norm"),
                                      ("module", "self_cross_types", ["FLASH2", "Linear"], "self_cross_types")):
        net = _StandIn()
        setattr(net.decoder_vit.cross_attn_blocks[1] if where == "block" else net.decoder_vit, attr, value)
        with pytest.raises(NotImplementedError, match=match):
            patch_vit_decoder(net)
    net = _StandIn()
    del net.decoder_vit.self_attn_blocks[0].ls1
    with pytest.raises(NotImplementedError, match="ls1.gamma"):
        patch_vit_decoder(net)
    # the C ABI: a loud refusal of anything not built
    a64 = torch.zeros(_lib.lib().mvs_vitdec_packed_bytes(4, 64), dtype=torch.uint8)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vitdec_linear(a64, 4, packing.pack_linear_bf16x3(torch.zeros(128, 64)), 64, 128, ops.VITDEC_EPI_F32)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vitdec_kv(torch.zeros(4, 768), 1, 4)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vitdec_apply(torch.zeros(4, 1536), torch.zeros(1, 12, 4160), 1, 4)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vitdec_conv(a64, torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8), 3, 1, 2, 2)
    # the wrappers: layouts and packed sizes before any pointer is taken
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.vitdec_rows(torch.zeros(1, 1, 4, 384), 0, 1)
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.vitdec_rows(torch.zeros(1, 1, 768, 4).transpose(2, 3), 0, 1)
    with pytest.raises(ValueError, match="views"):
        ops.vitdec_rows(torch.zeros(1, 2, 4, 768), 1, 2)
    with pytest.raises(ValueError, match="768 elements"):
        ops.vitdec_rows(torch.zeros(1, 1, 4, 768), 0, 1, ln=(torch.zeros(64), torch.zeros(768)))
    with pytest.raises(ValueError, match="packed-split"):
        ops.vitdec_linear(a64, 4, packing.pack_linear_bf16x3(torch.zeros(768, 768)), 768, 768, ops.VITDEC_EPI_F32)
    a768 = torch.zeros(_lib.lib().mvs_vitdec_packed_bytes(4, 768), dtype=torch.uint8)
    with pytest.raises(ValueError, match="pack_linear_bf16x3"):
        ops.vitdec_linear(a768, 4, packing.pack_linear_bf16x3(torch.zeros(768, 64)), 768, 768, ops.VITDEC_EPI_F32)
    with pytest.raises(ValueError, match="gamma"):
        ops.vitdec_linear(a768, 4, packing.pack_linear_bf16x3(torch.zeros(768, 768)), 768, 768, ops.VITDEC_EPI_RESID, bias=torch.zeros(768))
    with pytest.raises(ValueError, match="summary"):
        ops.vitdec_apply(torch.zeros(4, 768), torch.zeros(1, 12, 64), 1, 4)
    with pytest.raises(ValueError, match="pack_vitdec_deconv"):
        ops.vitdec_conv(torch.zeros(_lib.lib().mvs_vitdec_packed_bytes(4, 256), dtype=torch.uint8), torch.zeros(8, dtype=torch.bfloat16),
                        torch.zeros(128), ops.VITDEC_UP0, 1, 2, 2)


def test_host_tensors_are_refused(monkeypatch, emu_lib):
    """There is no CPU route: with the device requirement in force (the product setting) a host tensor raises before any launch.  The
    emulated library only stands in for the size queries that come before the first pointer is taken."""
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    assert _lib._REQUIRE_DEVICE
    m = CrossVITDecoder(f27_args(f27())).eval()
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        m([torch.zeros(1, 1, 6, 768) for _ in range(3)], vit_shape=[1, 1, 2, 3, 768])
