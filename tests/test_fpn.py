"""CPU: the native FPN encoder / decoder (mvsformerplusplus_amd.features, csrc/fpn_kernels.hip) on the host emulator against fixture
F25 (the reference's own FPNEncoder / FPNDecoder, tests/golden/make_golden_fpn.py), F20's FPN head captures and the fp64 restatement
(tests/fpn_ref.py); the module contract (state-dict names, patch_fpn) and every refusal."""
import hashlib
import json

import pytest
import torch
import torch.nn as nn

import fpn_ref as R
from conftest import load_golden
from mvsformerplusplus_amd import _lib, features, ops, packing, synth
from mvsformerplusplus_amd.features import FPNDecoder, FPNEncoder, patch_fpn

LAYER_BAR = 3e-5          # per layer: x max(1, max|ref|) (F20's bar for the same arithmetic)
MODULE_BAR = 2e-4         # whole module: x each output's range


def f25():
    fx = load_golden("f25_fpn.npz")
    fx.update({k: v for k, v in load_golden("f25_fpn_decoder.npz").items() if k != "__name__"})
    fx.update({k: v for k, v in load_golden("f25_fpn_n2.npz").items() if k != "__name__"})
    return fx


def f25_weights(fx, prefix):
    """The state dict F25 was generated with, rebuilt from its manifest + seed and checked against the SHA-256 stored in F25."""
    keys = fx[prefix + "keys"]
    shapes = [tuple(json.loads(s)) for s in fx[prefix + "shapes"]]
    sd = synth.seeded_state_dict(dict(zip(keys, shapes)), int(fx[prefix + "seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == fx[prefix + "sha256"], "torch / numpy generator changed: regenerate F25 (tests/golden/make_golden_fpn.py)"
    return sd


def modules(fx, device="cpu"):
    enc, dec = FPNEncoder([8, 16, 32, 64]), FPNDecoder([8, 16, 32, 64])
    enc.load_state_dict(f25_weights(fx, "enc."), strict=True)
    dec.load_state_dict(f25_weights(fx, "dec."), strict=True)
    return enc.eval().to(device), dec.eval().to(device)


def close(got, want, bar, what):
    err = float((got.double() - want.double()).abs().max())
    lim = bar * max(1.0, float(want.abs().max()))
    assert got.shape == want.shape and err <= lim, (what, tuple(got.shape), tuple(want.shape), err, lim)
    return err


def within_range(got, want, bar, what):
    """max |got - want| <= bar x (max(want) - min(want)); returns the measured fraction of the range."""
    rng = float(want.max() - want.min())
    frac = float((got.double() - want.double()).abs().max()) / rng
    assert got.shape == want.shape and frac <= bar, (what, frac, bar)
    return frac


def check_layers(fx, device):
    """Every native entry point against F25 case a: each encoder layer on its captured input, out0 .. out2 on theirs, the two lateral
    merges, the fused last level and its unfused composition."""
    enc, dec = modules(fx, device)
    pe, pd = enc._params(torch.device(device)), dec._params(torch.device(device))
    prev = fx["a/x"]
    for name, k, s in FPNEncoder.LAYERS:
        got = ops.fpn_conv(prev.to(device), *pe[name], getattr(enc, name).conv.out_channels, k, s, ops.FPN_ACT_LEAKY).cpu()
        close(got, fx["a/" + name], LAYER_BAR, name)
        prev = fx["a/" + name]
    c01, c11, c21, c31 = (fx["a/" + n].to(device) for n in ("conv01", "conv11", "conv21", "conv31"))
    close(ops.fpn_conv(c31, *pd["out0"], 64, 1, 1, ops.FPN_ACT_SWISH).cpu(), fx["a/out0"], LAYER_BAR, "out0")
    close(ops.fpn_merge(c31, c21, *pd["inner1"]).cpu(), fx["a/intra1"], LAYER_BAR, "intra1")
    close(ops.fpn_conv(fx["a/intra1"].to(device), *pd["out1"], 32, 3, 1, ops.FPN_ACT_SWISH).cpu(), fx["a/out1"], LAYER_BAR, "out1")
    intra2 = fx["a/intra2"].to(device)
    close(ops.fpn_merge(fx["a/intra1"].to(device), c11, *pd["inner2"]).cpu(), fx["a/intra2"], LAYER_BAR, "intra2")
    close(ops.fpn_conv(intra2, *pd["out2"], 16, 3, 1, ops.FPN_ACT_SWISH).cpu(), fx["a/out2"], LAYER_BAR, "out2")
    fused = ops.fpn_merge_conv(intra2, c01, *pd["inner3"], *pd["out3"], 8, ops.FPN_ACT_SWISH).cpu()
    close(fused, fx["a/out3"], LAYER_BAR, "out3 fused")
    intra3 = ops.fpn_merge(intra2, c01, *pd["inner3"])
    unfused = ops.fpn_conv(intra3, *pd["out3"], 8, 3, 1, ops.FPN_ACT_SWISH).cpu()
    close(unfused, fx["a/out3"], LAYER_BAR, "out3 unfused")


def check_modules(fx, device):
    """Whole encoder and decoder, cases a (1 x 64 x 96) and b (2 x 40 x 56) -> the worst fraction of an output's range."""
    enc, dec = modules(fx, device)
    worst = 0.0
    with torch.no_grad():
        for case in ("a", "b"):
            eo = enc(fx[case + "/x"].to(device))
            for t, n in zip(eo, ("conv01", "conv11", "conv21", "conv31")):
                assert t.dtype == torch.float32 and t.is_contiguous()
                worst = max(worst, within_range(t.cpu(), fx[case + "/" + n], MODULE_BAR, (case, n)))
            do = dec(*eo)
            for k, t in enumerate(do):
                worst = max(worst, within_range(t.cpu(), fx["%s/out%d" % (case, k)], MODULE_BAR, (case, "out%d" % k)))
    return worst


def test_restatement_pinned_to_f25():
    """tests/fpn_ref.py (fp64) reproduces every capture of F25: the oracle used at sizes the fixture lacks."""
    fx = f25()
    sde, sdd = f25_weights(fx, "enc."), f25_weights(fx, "dec.")
    layers, inter = {}, {}
    ea = R.encoder(fx["a/x"], sde, layers=layers)
    for name, _, _ in R.ENC:
        close(layers[name], fx["a/" + name], 1e-5, name)
    da = R.decoder(*[fx["a/" + n] for n in ("conv01", "conv11", "conv21", "conv31")], sdd, inter=inter)
    for k in range(4):
        close(da[k], fx["a/out%d" % k], 1e-5, "out%d" % k)
    close(inter["intra1"], fx["a/intra1"], 1e-5, "intra1")
    close(inter["intra2"], fx["a/intra2"], 1e-5, "intra2")
    eb = R.encoder(fx["b/x"], sde)
    for t, n in zip(eb, ("conv01", "conv11", "conv21", "conv31")):
        close(t, fx["b/" + n], 1e-5, "b " + n)
    for k, t in enumerate(R.decoder(*eb, sdd)):
        close(t, fx["b/out%d" % k], 1e-5, "b out%d" % k)
    assert ea[0].shape == (1, 8, 64, 96) and fx["b/conv31"].shape == (2, 64, 5, 7)


def test_layers_against_f25(emu):
    check_layers(f25(), emu)


def test_modules_against_f25(emu):
    worst = check_modules(f25(), emu)
    print("FPN modules vs F25: worst |error| = %.3g of an output's range (bar %g)" % (worst, MODULE_BAR))


def test_decoder_heads_against_f20(emu):
    """The decoder's out1 / out2 / out3 layers on F20's captures of the reference's FPNDecoder.out_k (Conv2d + BatchNorm2d + Swish)."""
    fx = load_golden("f20_feature_heads.npz")
    dec = FPNDecoder([8, 16, 32, 64]).eval()
    for k in (1, 2, 3):
        seq = getattr(dec, "out%d" % k)
        seq[0].weight.data.copy_(fx["fpn%d_w" % k])
        seq[0].bias.data.copy_(fx["fpn%d_b" % k])
        seq[1].eps = float(fx["fpn%d_bn_eps" % k])
        for n in ("weight", "bias", "running_mean", "running_var"):
            getattr(seq[1], n).data.copy_(fx["fpn%d_bn_%s" % (k, n)])
    p = dec._params(torch.device("cpu"))
    for k in (1, 2, 3):
        y = fx["fpn%d_y" % k]
        close(ops.fpn_conv(fx["fpn%d_x" % k], *p["out%d" % k], y.shape[1], 3, 1, ops.FPN_ACT_SWISH), y, LAYER_BAR, "F20 fpn%d" % k)


def test_per_view_calls_equal_one_batched_call(emu):
    fx = f25()
    enc, dec = modules(fx)
    x = fx["b/x"]
    with torch.no_grad():
        batched = enc(x) + dec(*enc(x))
        for n in range(x.shape[0]):
            one = enc(x[n:n + 1]) + dec(*enc(x[n:n + 1]))
            for a, b in zip(one, batched):
                assert torch.equal(a[0], b[n])


def test_bf16_input_is_widened(emu):
    """A bf16 image gives exactly what its fp32 widening gives (the reference's autocast hands bf16 tensors around)."""
    fx = f25()
    enc, _ = modules(fx)
    xb = fx["b/x"][:1].to(torch.bfloat16)
    with torch.no_grad():
        for a, b in zip(enc(xb), enc(xb.float())):
            assert a.dtype == torch.float32 and torch.equal(a, b)


def test_state_dict_names_match_the_reference():
    """Submodule, parameter and buffer names and shapes are the reference's (F25 stores the reference modules' manifests), so a
    checkpoint's encoder.* / decoder.* entries load with strict=True and round-trip unchanged."""
    fx = f25()
    for prefix, mod in (("enc.", FPNEncoder([8, 16, 32, 64])), ("dec.", FPNDecoder([8, 16, 32, 64]))):
        ref = {k: tuple(json.loads(s)) for k, s in zip(fx[prefix + "keys"], fx[prefix + "shapes"])}
        assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == ref
        sd = f25_weights(fx, prefix)
        mod.load_state_dict(sd, strict=True)
        again = type(mod)([8, 16, 32, 64])
        again.load_state_dict(mod.state_dict(), strict=True)
        for k, v in again.state_dict().items():
            assert torch.equal(v, sd[k]), k


class _RefConv2d(nn.Module):
    def __init__(self, ci, co, k, s):
        super().__init__()
        self.conv = nn.Conv2d(ci, co, k, stride=s, padding=k // 2, bias=False)
        self.bn = nn.BatchNorm2d(co)


class _StandIn(nn.Module):
    """A network with the reference's attribute names: encoder / decoder (reference-named plain modules), vit, decoder_vit, FMT, fusions."""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Module()
        for name, k, s in FPNEncoder.LAYERS:
            ci, co = {"conv00": (3, 8), "conv01": (8, 8), "downsample1": (8, 16), "conv10": (16, 16), "conv11": (16, 16),
                      "downsample2": (16, 32), "conv20": (32, 32), "conv21": (32, 32), "downsample3": (32, 64), "conv30": (64, 64),
                      "conv31": (64, 64)}[name]
            setattr(self.encoder, name, _RefConv2d(ci, co, k, s))
        self.decoder = nn.Module()
        for k, (co, ks) in enumerate(((64, 1), (32, 3), (16, 3), (8, 3))):
            setattr(self.decoder, "out%d" % k, nn.Sequential(nn.Conv2d(64, co, ks, padding=ks // 2), nn.BatchNorm2d(co), nn.SiLU()))
        for k, ci in ((1, 32), (2, 16), (3, 8)):
            setattr(self.decoder, "inner%d" % k, nn.Conv2d(ci, 64, 1))
        self.vit = nn.Linear(4, 4)
        self.decoder_vit = nn.Linear(4, 4)
        self.FMT_with_pathway = nn.Conv2d(8, 8, 3)
        self.fusions = nn.ModuleList([nn.Conv3d(8, 8, 3)])


def test_patch_fpn_swaps_only_encoder_and_decoder():
    net = _StandIn()
    net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 3), strict=True)
    net = net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    others = {n: getattr(net, n) for n in ("vit", "decoder_vit", "FMT_with_pathway", "fusions")}
    assert patch_fpn(net) is net
    assert isinstance(net.encoder, FPNEncoder) and isinstance(net.decoder, FPNDecoder)
    assert not net.encoder.training and not net.decoder.training
    for n, m in others.items():
        assert getattr(net, n) is m
    after = net.state_dict()
    assert sorted(after) == sorted(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    # train mode is carried over (and then refused at forward)
    net2 = patch_fpn(_StandIn().train())
    assert net2.encoder.training and net2.decoder.training


def test_refusals(emu):
    with pytest.raises(NotImplementedError, match="feat_chs"):
        FPNEncoder([8, 16, 32, 32])
    with pytest.raises(NotImplementedError, match="feat_chs"):
        FPNDecoder([16, 32, 64, 64])
    with pytest.raises(NotImplementedError, match="norm_type"):
        FPNEncoder([8, 16, 32, 64], norm_type="IN")
    net = _StandIn()
    net.encoder.conv00.bn = nn.InstanceNorm2d(8)
    with pytest.raises(NotImplementedError, match="BatchNorm2d"):
        patch_fpn(net)
    enc, dec = FPNEncoder([8, 16, 32, 64]), FPNDecoder([8, 16, 32, 64])
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="reference's models/module.py"):
        enc(x)                                                            # train() mode (a fresh module)
    enc.eval()
    with pytest.raises(RuntimeError, match="no autograd"):
        enc(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="multiples of 8"):
        enc(torch.zeros(1, 3, 20, 16))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        enc(torch.zeros(1, 4, 16, 16))
    dec.eval()
    feats = [torch.zeros(1, 8, 16, 16), torch.zeros(1, 16, 8, 8), torch.zeros(1, 32, 4, 4), torch.zeros(1, 64, 2, 2)]
    with pytest.raises(ValueError, match="twice"):
        dec(feats[0], feats[1], feats[2], torch.zeros(1, 64, 3, 2))
    with pytest.raises(RuntimeError, match="no autograd"):
        dec(feats[0], feats[1], feats[2], feats[3].clone().requires_grad_(True))
    dec.train()
    with pytest.raises(RuntimeError, match="FPNDecoder"):
        dec(*feats)
    # the C ABI: what is built, and a loud refusal of anything else
    for ci, co, k, s in ((3, 8, 7, 1), (8, 16, 5, 2), (32, 64, 3, 2), (64, 64, 1, 1), (64, 8, 3, 1)):
        assert ops.fpn_conv_is_built(ci, co, k, s)
    assert not ops.fpn_conv_is_built(24, 24, 3, 1) and not ops.fpn_conv_is_built(3, 8, 7, 2)
    assert ops.fpn_merge_is_built(32) and ops.fpn_merge_is_built(8, 8) and not ops.fpn_merge_is_built(64) and not ops.fpn_merge_is_built(16, 16)
    w = packing.pack_fpn_conv_weights(torch.zeros(24, 24, 3, 3), 1)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.fpn_conv(torch.zeros(1, 24, 8, 8), w, None, 24, 3, 1)
    with pytest.raises(_lib.MvsHipError, match="lateral width"):
        ops.fpn_merge(torch.zeros(1, 64, 4, 4), torch.zeros(1, 64, 8, 8), torch.zeros(64, 64), torch.zeros(64))
    assert features.SUPPORTED_FEAT_CHS == [8, 16, 32, 64]
