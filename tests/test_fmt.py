"""CPU: the native FMT_with_pathway (mvsformerplusplus_amd.fmt, csrc/fmt_kernels.hip) on the host emulator against fixture F26 (the
reference's own FMT_with_pathway, tests/golden/make_golden_fmt.py), F20's smooth_k captures and the fp64 restatement (tests/fmt_ref.py);
the module contract (state-dict names, patch_fmt) and every refusal.

Bars (the project's, as tests/test_fpn.py uses them for the same split-bf16 arithmetic): LAYER_BAR for one entry point on its captured
input, MODULE_BAR for the whole module.  Measured on the emulator: entry points 1.26e-5 x max(1, max|ref|); whole module 9.9e-6 of an
output's range (cases a and b).  On an MI355X: entry points 1.15e-5, F26 1.39e-5; 1152 x 1536 and 1088 x 1920 at V = 5 against fp64:
1.07e-5 / 1.02e-5 (tests/test_fmt_gpu.py)."""
import hashlib
import json

import pytest
import torch
import torch.nn as nn

import fmt_ref as R
from conftest import load_golden
from mvsformerplusplus_amd import _lib, fmt, ops, packing, synth
from mvsformerplusplus_amd.fmt import FMT_with_pathway, patch_fmt

LAYER_BAR = 3e-5          # per entry point: x max(1, max|ref|)
MODULE_BAR = 2e-4         # whole module: x each output's range
STAGES = ("stage1", "stage2", "stage3", "stage4")


def f26():
    fx = load_golden("f26_fmt.npz")
    for name in ("f26_fmt_a_out.npz", "f26_fmt_a_full.npz", "f26_fmt_a_full_out.npz", "f26_fmt_b.npz"):
        fx.update({k: v for k, v in load_golden(name).items() if k != "__name__"})
    return fx


def f26_config(fx):
    return json.loads(fx["fmt.config"])


def f26_weights(fx):
    """The state dict F26 was generated with, rebuilt from its manifest + seed and checked against the SHA-256 stored in F26."""
    shapes = [tuple(json.loads(s)) for s in fx["fmt.shapes"]]
    sd = synth.seeded_state_dict(dict(zip(fx["fmt.keys"], shapes)), int(fx["fmt.seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == fx["fmt.sha256"], "torch / numpy generator changed: regenerate F26 (tests/golden/make_golden_fmt.py)"
    return sd


def module(fx, device="cpu"):
    m = FMT_with_pathway(**f26_config(fx))
    m.load_state_dict(f26_weights(fx), strict=True)
    return m.eval().to(device)


def inputs(fx, case, device="cpu"):
    return {s: fx["%s/%s" % (case, s)].to(device) for s in STAGES}


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


def planar(tokens):
    """captured tokens [N, n, 64] -> the native layout [N, 64, n]"""
    return tokens.transpose(1, 2).contiguous()


def check_entry_points(fx, device):
    """Every native entry point against F26 case a: each block on its captured input (reference view: self layers; source view 1: all
    layers, the cross layers with the summary of the captured refs), each pathway level fused and unfused on the captured maps."""
    m = module(fx, device)
    p = m._params(torch.device(device))
    names = m.FMT.layer_names
    worst = 0.0
    for view in ("ref", "src"):
        for i, n in enumerate(names):
            if view == "ref" and n != "self":
                continue
            wp, vec = p["block%d" % i]
            x = planar(fx["a/%s/blk%d_in" % (view, i)]).to(device)
            kv = ops.fmt_kv(x if n == "self" else planar(fx["a/refs"][i // 2]).to(device), wp, vec)
            got = ops.fmt_block(x, kv, wp, vec).cpu()
            worst = max(worst, close(got, planar(fx["a/%s/blk%d_out" % (view, i)]), LAYER_BAR, (view, "block", i)))
    prev = fx["a/out_stage1"][0]
    for k in (1, 2, 3):
        lat, want = fx["a/stage%d" % (k + 1)][0], fx["a/out_stage%d" % (k + 1)][0]
        w_red, w_sm = p["level%d" % k]
        worst = max(worst, close(ops.fmt_path(prev.to(device), lat.to(device), w_red, w_sm).cpu(), want, LAYER_BAR, ("level fused", k)))
        merged = ops.fmt_merge(prev.to(device), lat.to(device), w_red)
        ref_merged = fx["a/smooth%d_in" % k] if k < 3 else fx["a/smooth3_in_v1"]
        worst = max(worst, close(merged.cpu() if k < 3 else merged[1:2].cpu(), ref_merged, LAYER_BAR, ("merge", k)))
        worst = max(worst, close(ops.fmt_smooth(merged, w_sm).cpu(), want, LAYER_BAR, ("level unfused", k)))
        worst = max(worst, close(ops.fmt_smooth(ref_merged.to(device), w_sm).cpu(), want if k < 3 else want[1:2], LAYER_BAR, ("smooth", k)))
        prev = want
    return worst


def check_module(fx, device):
    """Whole module, cases a (1 x 3 views, 8 x 12 tokens) and b (2 x 2 views, ragged levels) -> the worst fraction of an output's range."""
    m = module(fx, device)
    worst = 0.0
    with torch.no_grad():
        for case in ("a", "b"):
            out = m(inputs(fx, case, device))
            assert sorted(out) == sorted(STAGES)
            for s in STAGES:
                t = out[s]
                assert t.dtype == torch.float32 and t.is_contiguous()
                worst = max(worst, within_range(t.cpu(), fx["%s/out_%s" % (case, s)], MODULE_BAR, (case, s)))
    return worst


def test_restatement_pinned_to_f26():
    """tests/fmt_ref.py (fp64) reproduces every capture of F26: the oracle used at sizes the fixture lacks."""
    fx = f26()
    sd = f26_weights(fx)
    names = f26_config(fx)["layer_names"]
    cap = {}
    oa = R.fmt(inputs(fx, "a"), sd, names, capture=cap)
    for s in STAGES:
        close(oa[s], fx["a/out_" + s], 1e-5, "a " + s)
    for i, n in enumerate(names):
        for view, v in (("ref", 0), ("src", 1)):
            if v == 0 and n != "self":
                continue
            close(cap[("blk", v, i)][0], fx["a/%s/blk%d_in" % (view, i)], 1e-5, (view, i, "in"))
            close(cap[("blk", v, i)][1], fx["a/%s/blk%d_out" % (view, i)], 1e-5, (view, i, "out"))
    close(torch.stack(cap["refs"]), fx["a/refs"], 1e-5, "refs")
    for k in (1, 2):
        close(torch.cat(cap[("merged", k)]), fx["a/smooth%d_in" % k], 1e-5, ("merged", k))
    close(cap[("merged", 3)][1], fx["a/smooth3_in_v1"], 1e-5, ("merged", 3))
    ob = R.fmt(inputs(fx, "b"), sd, names)
    for s in STAGES:
        close(ob[s], fx["b/out_" + s], 1e-5, "b " + s)
    assert fx["a/stage1"].shape == (1, 3, 64, 8, 12) and fx["b/stage4"].shape == (2, 2, 8, 20, 72)


def test_entry_points_against_f26(emu):
    worst = check_entry_points(f26(), emu)
    print("FMT entry points vs F26: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (worst, LAYER_BAR))


def test_module_against_f26(emu):
    worst = check_module(f26(), emu)
    print("FMT_with_pathway vs F26: worst |error| = %.3g of an output's range (bar %g)" % (worst, MODULE_BAR))


def test_smooth_against_f20(emu):
    """smooth_k alone on F20's captures of the reference's FMT_with_pathway.smooth_k (ragged sizes 5 x 18, 10 x 36, 20 x 72)."""
    fx = load_golden("f20_feature_heads.npz")
    for k in (1, 2, 3):
        x, y = fx["fmt%d_x" % k][0], fx["fmt%d_y" % k][0]
        close(ops.fmt_smooth(x, packing.pack_fpn_conv_weights(fx["fmt%d_w" % k], 1)), y, LAYER_BAR, "F20 fmt%d" % k)


def test_cross_summary_once_equals_per_source_view(emu):
    """The cross layer's key/value summary depends on the reference view only: computed once and shared by the source views (what the
    module does) it gives bit for bit what one call per source view gives; and a batch of views equals per-view calls."""
    fx = f26()
    m = module(fx)
    wp, vec = m._params(torch.device("cpu"))["block1"]
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(2, 64, 7, 11, generator=g)                  # two batch elements, n = 77 (a ragged last tile)
    src = torch.randn(6, 64, 7, 11, generator=g)                  # three source views each
    kv = ops.fmt_kv(ref, wp, vec)
    batched = ops.fmt_block(src, kv, wp, vec, kv_div=3)
    for i in range(6):
        kv_i = ops.fmt_kv(ref[i // 3:i // 3 + 1], wp, vec)
        assert torch.equal(kv_i[0], kv[i // 3])
        assert torch.equal(ops.fmt_block(src[i:i + 1], kv_i, wp, vec)[0], batched[i])
    own = ops.fmt_kv(src, wp, vec)                                # self attention: per-view summaries, batched == per view
    for i in range(6):
        assert torch.equal(ops.fmt_kv(src[i:i + 1], wp, vec)[0], own[i])


def test_batched_views_equal_per_view_calls(emu):
    fx = f26()
    m = module(fx)
    feats = inputs(fx, "b")
    with torch.no_grad():
        both = m(feats)
        for b in range(2):
            one = m({s: feats[s][b:b + 1] for s in STAGES})
            for s in STAGES:
                assert torch.equal(one[s][0], both[s][b]), s
        ref_only = m({s: feats[s][:, :1] for s in STAGES})        # V = 1: the reference view alone
        for s in STAGES:
            assert torch.equal(ref_only[s][:, 0], both[s][:, 0]), s


def test_bf16_input_is_widened(emu):
    fx = f26()
    m = module(fx)
    fb = {s: t.to(torch.bfloat16) for s, t in inputs(fx, "b").items()}
    with torch.no_grad():
        a, b = m(fb), m({s: t.float() for s, t in fb.items()})
    for s in STAGES:
        assert a[s].dtype == torch.float32 and torch.equal(a[s], b[s])


def test_state_dict_names_match_the_reference():
    """The 66 keys and their shapes are the reference's (F26 stores the reference module's manifest), so a checkpoint's FMT_module.*
    entries load with strict=True and round-trip unchanged."""
    fx = f26()
    ref = {k: tuple(json.loads(s)) for k, s in zip(fx["fmt.keys"], fx["fmt.shapes"])}
    mod = FMT_with_pathway(**f26_config(fx))
    assert len(ref) == 66 and {k: tuple(v.shape) for k, v in mod.state_dict().items()} == ref
    sd = f26_weights(fx)
    mod.load_state_dict(sd, strict=True)
    again = FMT_with_pathway(**f26_config(fx))
    again.load_state_dict(mod.state_dict(), strict=True)
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_pack_fmt_linear_layout():
    """packed[step][mb][hi|lo][g*16+j][e] = w[16 mb + j][32 step + 16 (e >> 2) + 4 g + (e & 3)] (small integers: hi exact, lo zero)."""
    w = (torch.arange(32 * 64, dtype=torch.float32).reshape(32, 64) % 251) - 125
    p = packing.pack_fmt_linear(w).float().reshape(2, 2, 2, 4, 16, 8)
    assert float(p[:, :, 1].abs().max()) == 0.0
    for step, mb, g, j, e in ((0, 0, 0, 0, 0), (1, 1, 3, 15, 7), (0, 1, 2, 5, 4), (1, 0, 1, 9, 3)):
        assert float(p[step, mb, 0, g, j, e]) == float(w[16 * mb + j, 32 * step + 16 * (e >> 2) + 4 * g + (e & 3)])


class _RefBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(64), nn.LayerNorm(64)
        self.attn = nn.Module()
        for n in ("q_proj", "k_proj", "v_proj"):
            setattr(self.attn, n, nn.Linear(64, 64, bias=False))
        self.attn.proj = nn.Linear(64, 64)
        self.ls1, self.ls2 = nn.Module(), nn.Module()
        self.ls1.gamma, self.ls2.gamma = nn.Parameter(torch.ones(64)), nn.Parameter(torch.ones(64))
        self.mlp = nn.Module()
        self.mlp.fc1, self.mlp.fc2 = nn.Linear(64, 256), nn.Linear(256, 64)
        self.post_norm, self.pre_norm_query = False, False        # CrossBlock's attributes as the shipped FMT_config sets them


class _StandIn(nn.Module):
    """A network with the reference's attribute names: FMT_module (reference-named plain modules), encoder, decoder, vit, decoder_vit,
    fusions."""

    def __init__(self):
        super().__init__()
        self.FMT_module = nn.Module()
        self.FMT_module.FMT = nn.Module()
        self.FMT_module.FMT.layers = nn.ModuleList([_RefBlock() for _ in range(4)])
        self.FMT_module.FMT.layer_names = ["self", "cross", "self", "cross"]
        self.FMT_module.FMT.attention_type, self.FMT_module.FMT.d_model, self.FMT_module.FMT.nhead = "Linear", 64, 4
        for k, c in ((1, 32), (2, 16), (3, 8)):
            setattr(self.FMT_module, "dim_reduction_%d" % k, nn.Conv2d(2 * c, c, 1, bias=False))
            setattr(self.FMT_module, "smooth_%d" % k, nn.Conv2d(c, c, 3, padding=1, bias=False))
        self.encoder, self.decoder = nn.Conv2d(3, 8, 3), nn.Conv2d(8, 8, 3)
        self.vit, self.decoder_vit = nn.Linear(4, 4), nn.Linear(4, 4)
        self.fusions = nn.ModuleList([nn.Conv3d(8, 8, 3)])


def test_patch_fmt_swaps_only_the_fmt_module():
    net = _StandIn()
    net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 4), strict=True)
    net = net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    others = {n: getattr(net, n) for n in ("encoder", "decoder", "vit", "decoder_vit", "fusions")}
    assert patch_fmt(net) is net
    assert isinstance(net.FMT_module, FMT_with_pathway) and not net.FMT_module.training
    for n, mod in others.items():
        assert getattr(net, n) is mod
    after = net.state_dict()
    assert sorted(after) == sorted(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert patch_fmt(_StandIn().train()).FMT_module.training          # train mode is carried over (and then refused at forward)


def test_refusals(emu):
    cfg = f26_config(f26())
    for bad, match in ((dict(attention_type="FLASH2"), "attention_type"), (dict(d_model=128), "d_model"), (dict(nhead=8), "nhead"),
                       (dict(ffn_type="glu"), "ffn_type"), (dict(init_values=None), "init_values"), (dict(post_norm=True), "post_norm"),
                       (dict(pre_norm_query=True), "pre_norm_query"), (dict(self_cross_types=["Linear", "Linear"]), "self_cross_types"),
                       (dict(layer_names=["cross", "self"]), "layer_names"), (dict(layer_names=["self", "other"]), "layer_names"),
                       (dict(layer_names=["self", "cross", "cross"]), "layer_names"), (dict(base_channel=4), "base_channel")):
        with pytest.raises(NotImplementedError, match=match):
            FMT_with_pathway(**dict(cfg, **bad))
    # the reference's CrossBlock defaults pre_norm_query to True (block.py:333): a config that omits the key is that configuration
    with pytest.raises(NotImplementedError, match="pre_norm_query"):
        FMT_with_pathway(**{k: v for k, v in cfg.items() if k != "pre_norm_query"})
    FMT_with_pathway(**{k: v for k, v in cfg.items() if k != "post_norm"})                                       # its default is False
    FMT_with_pathway(**dict(cfg, layer_names=["self", "self", "cross"], softmax_scale=None, train_avg_length=1))     # accepted
    m = FMT_with_pathway(**cfg)
    feats = {"stage1": torch.zeros(1, 2, 64, 2, 3), "stage2": torch.zeros(1, 2, 32, 4, 6), "stage3": torch.zeros(1, 2, 16, 8, 12),
             "stage4": torch.zeros(1, 2, 8, 16, 24)}
    with pytest.raises(RuntimeError, match="reference's models/FMT.py"):
        m(feats)                                                      # train() mode (a fresh module)
    m.eval()
    with pytest.raises(RuntimeError, match="no autograd"):
        m(dict(feats, stage3=feats["stage3"].clone().requires_grad_(True)))
    with pytest.raises(ValueError, match="stage1..stage4"):
        m(dict(feats, stage2=torch.zeros(1, 2, 16, 4, 6)))
    with pytest.raises(ValueError, match="stage1..stage4"):
        m(dict(feats, stage4=torch.zeros(1, 3, 8, 16, 24)))
    out = m(feats)                                                    # a tiny map runs (n = 6 tokens)
    assert out["stage4"].shape == (1, 2, 8, 16, 24)
    # what the old module's blocks do is not in the state dict: patch_fmt reads it from the blocks (an attribute that is absent
    # means the reference's default: pre_norm_query True)
    for attr, value, match in (("pre_norm_query", True, "pre_norm_query"), ("post_norm", True, "post_norm")):
        net = _StandIn()
        setattr(net.FMT_module.FMT.layers[1], attr, value)
        with pytest.raises(NotImplementedError, match=match):
            patch_fmt(net)
    net = _StandIn()
    del net.FMT_module.FMT.layers[3].pre_norm_query
    with pytest.raises(NotImplementedError, match="pre_norm_query"):
        patch_fmt(net)
    net = _StandIn()
    del net.FMT_module.FMT.layers[0].ls1
    with pytest.raises(NotImplementedError, match="ls1.gamma"):
        patch_fmt(net)
    # the C ABI: a loud refusal of anything not built
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.fmt_path(torch.zeros(1, 8, 2, 2), torch.zeros(1, 4, 4, 4), torch.zeros(4, 8), packing.pack_fpn_conv_weights(torch.zeros(8, 8, 3, 3), 1))
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.fmt_smooth(torch.zeros(1, 24, 4, 4), packing.pack_fpn_conv_weights(torch.zeros(24, 24, 3, 3), 1))
    with pytest.raises(ValueError, match=r"\[N, 64, n\]"):
        ops.fmt_kv(torch.zeros(1, 32, 8), torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match="pack_fmt_block"):
        ops.fmt_kv(torch.zeros(1, 64, 8), torch.zeros(1), torch.zeros(1))
    wp, vec = packing.pack_fmt_block({k[len("FMT.layers.0."):]: v for k, v in m.state_dict().items() if k.startswith("FMT.layers.0.")})
    with pytest.raises(ValueError, match="position table"):
        ops.fmt_kv(torch.zeros(1, 64, 2, 3), wp, vec, pe=torch.zeros(64, 8))         # a table for another map size
    with pytest.raises(ValueError, match="position table"):
        ops.fmt_block(torch.zeros(1, 64, 6), torch.zeros(1, 20480, dtype=torch.uint8), wp, vec, pe=torch.zeros(64, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="pack_fpn_conv_weights"):
        ops.fmt_smooth(torch.zeros(1, 8, 4, 4), packing.pack_fpn_conv_weights(torch.zeros(16, 16, 3, 3), 1))
    with pytest.raises(ValueError, match="pack_fpn_conv_weights"):
        ops.fmt_path(torch.zeros(1, 16, 2, 2), torch.zeros(1, 8, 4, 4), torch.zeros(8, 16), torch.zeros(8, dtype=torch.bfloat16))
    assert fmt.STAGE_CHANNELS == (64, 32, 16, 8)


def test_host_tensors_are_refused(monkeypatch, emu_lib):
    """There is no CPU route: with the device requirement in force (the product setting) a host tensor raises before any launch.  The
    emulated library only stands in for the size queries that come before the first pointer is taken."""
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    assert _lib._REQUIRE_DEVICE
    m = FMT_with_pathway(**f26_config(f26())).eval()
    feats = {"stage1": torch.zeros(1, 1, 64, 2, 3), "stage2": torch.zeros(1, 1, 32, 4, 6), "stage3": torch.zeros(1, 1, 16, 8, 12),
             "stage4": torch.zeros(1, 1, 8, 16, 24)}
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        m(feats)
