"""CPU: the REFERENCE's own top-level network (DINOv2MVSNet, shipped config) with its ``fusions`` swapped by ``patch_model`` - the
one-line integration of INTEGRATION.md - must reproduce the unpatched model.  The reference network is recorded at its ``fusions[i]``
boundary in tests/golden/f21_dropin_network*.npz (tests/golden/make_golden.py: f21_dropin_network): the seeded weights of every fusion
(manifest + seed, pinned in weights_sha256.json), the exact call its cascade loop made to ``fusions[i].forward`` (features out of its
backbone + FMT, projection matrices, depth hypotheses, tmp, 3D position encoding) and what came back, plus the network's final outputs.  Here the
recorded fusions are handed to ``patch_model`` as the reference model's ``fusions``, every patched stage answers the recorded call, and
the network's final outputs are assembled the way its loop assembles them.  The HIP kernels run through the host emulator."""
import json

import torch
import torch.nn as nn
import torch.nn.functional as F

import pytest

from conftest import golden_weights, load_golden, rel_l1


class _RecordedStage(nn.Module):
    """Stands in for a reference ``models.cost_volume.StageNet`` as far as ``patch_model`` reads one: ``args``, ``ndepth``,
    ``stage_idx``, ``state_dict()``, its parameters' device and the train / eval mode."""

    def __init__(self, fx, prefix):
        super().__init__()
        self.args = json.loads(fx[prefix + "args"])
        self.ndepth = int(fx[prefix + "ndepth"])
        self.stage_idx = int(fx[prefix + "stage_idx"])
        self._sd = golden_weights(fx, prefix + "w.")
        self.anchor = nn.Parameter(torch.zeros(1))

    def state_dict(self, *args, **kwargs):
        return dict(self._sd)


class _RecordedNetwork(nn.Module):
    def __init__(self, fx):
        super().__init__()
        self.fusions = nn.ModuleList([_RecordedStage(fx, "s%d." % s) for s in range(1, 5)])


def _call(fx, s):
    """-> (features, proj, hyp) and keyword arguments of the reference loop's call to fusions[s - 1].forward."""
    p = "s%d." % s
    return (fx[p + "features"], fx[p + "proj"], fx[p + "hyp"]), {"tmp": float(fx[p + "tmp"]), "position3d": fx.get(p + "pos")}


def _network_outputs(stage_outs, H, W):
    """The reference loop's final outputs: the last stage's depth and the mean of the stage confidences, nearest-upsampled."""
    confs = [o["photometric_confidence"] for o in stage_outs]
    confs = [c if c.shape[-2:] == (H, W) else F.interpolate(c.unsqueeze(1), [H, W], mode="nearest").squeeze(1) for c in confs]
    return stage_outs[-1]["depth"], sum(confs) / len(confs)


def _check_eval(fx, patched, depth_bound, conf_bound):
    outs = []
    with torch.no_grad():
        for s in range(1, 5):
            args, kw = _call(fx, s)
            o = patched.fusions[s - 1](*args, **kw)
            assert set(o.keys()) == set(fx["s%d.out_names" % s]), s
            assert rel_l1(o["depth"], fx["s%d.depth" % s]) <= depth_bound, s
            outs.append(o)
    ref_depth, ref_conf = fx["refined_depth"], fx["photometric_confidence"]
    depth, conf = _network_outputs(outs, *ref_depth.shape[-2:])
    r = rel_l1(depth, ref_depth)
    assert r <= depth_bound, r
    assert (conf - ref_conf).abs().max() <= conf_bound


@pytest.mark.parametrize("prec", [None, "bf16x3"])
def test_patch_model_on_the_reference_network(emu, prec):
    """prec None = the product defaults (policy "stagemix": fp32-equivalent coarse stages, fp16 regulariser activations on the fine ones; 16-bit attention operands): 5e-4 on depth; "bf16x3" = the
    fp32-equivalent forms of both: 2e-4 (the residue is the feature extractor's own fp32 summation order)."""
    from mvsformerplusplus_amd import patch_model
    from mvsformerplusplus_amd.cost_volume import StageNet as HipStageNet
    fx = load_golden("f21_dropin_network.npz")
    model = _RecordedNetwork(fx).eval()
    patched = patch_model(model, conv_precision=prec, attention_precision=prec)
    assert all(isinstance(f, HipStageNet) for f in patched.fusions)
    assert patched.fusions[0].cost_reg.kind == "transformer"           # the shipped stage-1 regulariser
    assert set(fx["net_names"]) == set(fx["s4.out_names"]) | {"stage1", "stage2", "stage3", "stage4", "refined_depth"}
    _check_eval(fx, patched, 2e-4 if prec else 5e-4, 5e-3 if prec else 3e-2)


def test_patch_model_on_the_reference_network_other_base_ch(emu):
    """The reference's own network built with base_ch = 4 (not a shipped value) and all-"Normal" regularisers: cost_volume.py:29-49 then
    builds CostRegNet(4, 4) / CostRegNet3D(4, 4).  patch_model must take the model as it is (strict state-dict load) and reproduce it -
    the stages run the direct gather with 4 groups and the shape-generic exact-fp32 convolution kernel (ABI v10)."""
    from mvsformerplusplus_amd import patch_model
    fx = load_golden("f21_dropin_network_base_ch4.npz")
    model = _RecordedNetwork(fx).eval()
    assert model.fusions[0].state_dict()["cost_reg.conv1.conv.weight"].shape[:2] == (8, 4)
    patched = patch_model(model, conv_precision="bf16x3")
    assert all(f._generic_regulariser() for f in patched.fusions)
    _check_eval(fx, patched, 2e-4, 5e-3)


def test_patch_model_trains_like_the_reference_network(emu):
    """train.py's use: the reference's network in .train() mode with its stages swapped by patch_model.  The stage-1 loss (before any
    argmax-dependent hypothesis scheduling) on the recorded stage-1 call must give the reference fusion's gradients for the stage's own
    parameters AND for the features it is handed (what flows back into the reference's feature extractor): every gradient tensor is
    stored as its absolute maximum and 256 elements at fixed indices (all of it when smaller), and both are compared.  The later stages
    must produce finite gradients for everything."""
    from mvsformerplusplus_amd import patch_model
    fx = load_golden("f21_dropin_network.npz")
    patched = patch_model(_RecordedNetwork(fx).train())
    assert all(f.training for f in patched.fusions)
    (feat, proj, hyp), kw = _call(fx, 1)
    feat = feat.clone().requires_grad_(True)
    out = patched.fusions[0](feat, proj, hyp, **kw)
    (torch.softmax(out["prob_volume_pre"], 1) * fx["train.R"]).sum().backward()
    names = sorted(k[len("train.grad."):-len(".absmax")] for k in fx if k.startswith("train.grad.") and k.endswith(".absmax"))
    hip_g = {n: p.grad for n, p in patched.fusions[0].named_parameters() if p.grad is not None}
    hip_g["features"] = feat.grad
    assert set(names) == set(hip_g)
    # parameters whose gradient is analytically zero (a bias in front of a normalisation, a constant added to every logit under
    # the softmax) hold rounding noise in both models: they are compared on an absolute floor, not relative to themselves
    top = max(float(fx["train.grad.%s.absmax" % n]) for n in names)
    worst, n_cmp = 0.0, 0
    for n in names:
        amax = float(fx["train.grad.%s.absmax" % n])
        g = hip_g[n].reshape(-1)
        if amax <= 1e-6 * top:
            assert float(g.abs().max()) <= 1e-5 * top, n
            continue
        idx, val = torch.as_tensor(fx["train.grad.%s.idx" % n]).long().reshape(-1), torch.as_tensor(fx["train.grad.%s.val" % n]).reshape(-1)
        worst = max(worst, float((g[idx] - val).abs().max()) / amax, abs(float(g.abs().max()) - amax) / amax)
        n_cmp += 1
    assert n_cmp > 90 and worst <= 2e-3, (n_cmp, worst)             # measured: 6e-4 worst (a scalar gamma) over 99 of the 101 tensors
    assert any(n.startswith("cost_reg.attention_layers") for n in names) and float(feat.grad.abs().max()) > 0
    # all four stages in the loss (stages 2-4: the native U-Net training path): every parameter that receives a gradient gets a finite one
    patched.zero_grad()
    outs, feats = [], []
    for s in range(1, 5):
        (f, p, h), kw = _call(fx, s)
        feats.append(f.clone().requires_grad_(True))
        outs.append(patched.fusions[s - 1](feats[-1], p, h, **kw))
    sum(o["prob_volume_pre"].square().mean() for o in outs).backward()
    got = {n: p.grad for n, p in patched.named_parameters() if p.grad is not None}
    assert all(torch.isfinite(g).all() for g in got.values()) and all(torch.isfinite(f.grad).all() for f in feats)
    for s in (1, 2, 3):
        assert float(got["fusions.%d.cost_reg.conv1.conv.weight" % s].abs().max()) > 0
