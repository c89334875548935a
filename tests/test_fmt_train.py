"""CPU: training of FMT_with_pathway (mvsformerplusplus_amd.training.fmt_forward_train, fmt.TrainableFMT_with_pathway, DESIGN.md section
4.17) on the host emulator against fp64 autograd through the restatement tests/fmt_ref.py, which is itself pinned to fixture F32 (the
reference's own module in train mode, tests/golden/make_golden_fmt_train.py).

Bar, for EVERY gradient tensor g (inputs and parameters): max|g - g64| <= MODULE_BAR x max|g64|, MODULE_BAR = 2e-4 (the project's bar for
this split-bf16 arithmetic, tests/test_fmt.py).  Reference points on the CPU: fp32 autograd of the restatement sits at 7.0e-6 / 4.1e-6
(cases a / b), operands rounded to hi + lo bf16 at 2.5e-5 / 3.6e-5.  Measured for the native path on the emulator, worst tensor:
pathway levels 6.8e-6, single blocks 1.1e-6, whole module 1.6e-5 (case a) / 2.1e-5 (case b); on an MI355X 6.7e-6, 9.8e-7, 1.7e-5 / 1.9e-5
(tests/test_fmt_train_gpu.py).  The backward itself is fp32; what it inherits from the split-bf16 forward is the saved activations."""
import functools
import glob
import hashlib
import os

import pytest
import torch

import fmt_ref as R
import test_fmt as T
from conftest import GOLDEN, load_golden
from mvsformerplusplus_amd import _lib, fmt, ops, training
from mvsformerplusplus_amd.fmt import FMT_with_pathway, TrainableFMT_with_pathway, patch_fmt

BAR = T.MODULE_BAR
STAGES = T.STAGES
COT_SEED = 32                      # fixture F32's


def cotangents(shapes, seed=COT_SEED):
    """A fixed standard normal per output stage, drawn in stage order."""
    g = torch.Generator().manual_seed(seed)
    return {s: torch.randn(shapes[s], generator=g) for s in STAGES}


def worst_rel(got, want, what):
    """max |got - want| / max |want| per tensor -> the worst; asserts the bar for each."""
    worst = 0.0
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        assert g is not None and tuple(g.shape) == tuple(w.shape), (what, k)
        rel = float((g.double().cpu() - w).abs().max()) / float(w.abs().max())
        assert rel <= BAR, (what, k, rel, BAR)
        worst = max(worst, rel)
    return worst


@functools.lru_cache(maxsize=None)
def fixture():
    fx = T.f26()
    return fx, T.f26_weights(fx), T.f26_config(fx)


@functools.lru_cache(maxsize=None)
def oracle(case, views=None):
    """fp64 autograd through tests/fmt_ref.py on F26's weights and inputs -> (outputs, {("in", stage) | state-dict key: gradient}); computed
    once per case and shared (read-only)."""
    fx, sd, cfg = fixture()
    feats = {s: t[:, :views].double().requires_grad_(True) for s, t in T.inputs(fx, case).items()}
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    out = R.fmt(feats, sd64, cfg["layer_names"])
    cot = cotangents({s: out[s].shape for s in STAGES})
    sum((out[s] * cot[s].double()).sum() for s in STAGES).backward()
    grads = {("in", s): feats[s].grad for s in STAGES}
    grads.update({k: v.grad for k, v in sd64.items()})
    return {s: out[s].detach() for s in STAGES}, grads


def trainable(device="cpu", train=True):
    fx, sd, cfg = fixture()
    m = TrainableFMT_with_pathway(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.train(train).to(device)


def native_grads(m, feats):
    """forward + backward of the native module with the seeded cotangent -> (outputs, gradients keyed like oracle()'s)."""
    m.zero_grad(set_to_none=True)
    out = m(feats)
    cot = cotangents({s: out[s].shape for s in STAGES})
    sum((out[s] * cot[s].to(out[s].device)).sum() for s in STAGES).backward()
    grads = {("in", s): feats[s].grad for s in STAGES}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return out, grads


def check_module_case(case, device):
    fx, _, _ = fixture()
    m = trainable(device)
    feats = {s: t.clone().to(device).requires_grad_(True) for s, t in T.inputs(fx, case).items()}
    out, grads = native_grads(m, feats)
    want_out, want = oracle(case)
    assert len(want) == 70
    for s in STAGES:
        assert out[s].dtype == torch.float32 and out[s].is_contiguous()
        T.within_range(out[s].detach().cpu(), want_out[s], BAR, (case, s))
    return worst_rel(grads, want, "module case " + case)


# ---- pathway levels ------------------------------------------------------------------------------------------------------------------
LEVEL_SHAPES = [  # N, (h, w) of prev, (H, W) of the lateral
    (2, (2, 3), (4, 6)),          # exact x2
    (2, (3, 9), (5, 18)),         # F26 case b's ragged ratios
    (2, (5, 18), (10, 36)),
    (1, (10, 36), (20, 72)),
    (2, (5, 7), (3, 4)),          # a lateral smaller than prev
    (2, (1, 4), (3, 9)),          # h = 1
    (3, (3, 35), (5, 70)),        # wider than one 4 x 64 tile with a ragged edge, N > 1: several partials
]


def level_case(C, N, hw, HW, seed):
    g = torch.Generator().manual_seed(seed)
    prev, lat = torch.randn(N, 2 * C, *hw, generator=g), torch.randn(N, C, *HW, generator=g)
    w_red, w_sm = torch.randn(C, 2 * C, 1, 1, generator=g) / (2 * C) ** 0.5, torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5
    return prev, lat, w_red, w_sm, torch.randn(N, C, *HW, generator=g)


def level_oracle(k, prev, lat, w_red, w_sm, cot):
    leaves = [t.detach().double().requires_grad_(True) for t in (prev, lat, w_red, w_sm)]
    y, _ = R.level({"dim_reduction_%d.weight" % k: leaves[2], "smooth_%d.weight" % k: leaves[3]}, k, leaves[0], leaves[1])
    (y * cot.double()).sum().backward()
    return dict(zip(("prev", "lat", "w_reduce", "w_smooth"), (t.grad for t in leaves)))


def check_levels(device):
    worst = 0.0
    for k, C in ((1, 32), (2, 16), (3, 8)):
        for i, (N, hw, HW) in enumerate(LEVEL_SHAPES):
            prev, lat, w_red, w_sm, cot = level_case(C, N, hw, HW, 100 * k + i)
            want = level_oracle(k, prev, lat, w_red, w_sm, cot)
            leaves = [t.clone().to(device).requires_grad_(True) for t in (prev, lat, w_red, w_sm)]
            y = training.FmtPathLevelTrain.apply(*leaves)
            (y * cot.to(device)).sum().backward()
            got = dict(zip(("prev", "lat", "w_reduce", "w_smooth"), (t.grad for t in leaves)))
            worst = max(worst, worst_rel(got, want, ("level", C, N, hw, HW)))
    return worst


def test_level_backward_against_fp64(emu):
    worst = check_levels(emu)
    print("pathway level backward vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (worst, BAR))


def test_adjoint_identity(emu):
    """<U(W_r a), b> = <a, W_r^T U^T b>: the gather of mvs_fmt_path_bwd is the adjoint of the interpolation the forward evaluates."""
    for C, N, hw, HW in ((32, 2, (3, 9), (5, 18)), (16, 1, (5, 7), (3, 4)), (8, 2, (1, 4), (3, 9)), (8, 1, (4, 5), (9, 11))):
        a, lat, w_red, _, b = level_case(C, N, hw, HW, 7)
        w_red = w_red.reshape(C, 2 * C)
        lhs = ((ops.fmt_merge(a, lat, w_red).double() - lat.double()) * b.double()).sum()
        rhs = (a.double() * ops.fmt_path_bwd(b, a, w_red)[0].double()).sum()
        scale = float((ops.fmt_merge(a, lat, w_red).double() - lat.double()).abs().mul(b.double().abs()).sum())
        assert abs(float(lhs - rhs)) <= 1e-5 * scale, (C, hw, HW, float(lhs), float(rhs))


# ---- blocks --------------------------------------------------------------------------------------------------------------------------
def block_params(m, i):
    return [m.FMT.layers[i].get_parameter(k) for k in training.FMT_BLOCK_PARAMS]


def block_oracle(sd, i, x, cot, pe=None, ref=None, kv_div=1):
    """fp64 autograd of fmt_ref.block on planar x [N, 64, h, w] (view j reads ref[j // kv_div]) -> gradients keyed x / ref / parameter."""
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith("FMT.layers.%d." % i)}
    tok = lambda t: t.flatten(2).transpose(1, 2)
    x64 = x.detach().double().requires_grad_(True)
    ref64 = None if ref is None else ref.detach().double().requires_grad_(True)
    xin = x64 if pe is None else x64 + pe.double().reshape(1, 64, *x.shape[2:])
    ys = [R.block(sd64, i, tok(xin[j:j + 1]), None if ref is None else tok(ref64[j // kv_div:j // kv_div + 1])) for j in range(x.shape[0])]
    y = torch.cat(ys).transpose(1, 2).reshape(x.shape)
    (y * cot.double()).sum().backward()
    out = {"x": x64.grad}
    if ref is not None:
        out["ref"] = ref64.grad
    out.update({k[len("FMT.layers.%d." % i):]: v.grad for k, v in sd64.items()})
    return out


def check_blocks(device):
    fx, sd, _ = fixture()
    m = trainable(device)
    g = torch.Generator().manual_seed(11)
    h, w = 5, 7                                                   # n = 35: a ragged second 32-token tile
    worst = 0.0
    # a self block with the position table
    x, cot = torch.randn(2, 64, h, w, generator=g), torch.randn(2, 64, h, w, generator=g)
    pe = m.FMT.position_encoding(h, w, torch.device(device))
    xd = x.clone().to(device).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    (training.FmtBlockTrain.apply(xd, None, pe, 1, *block_params(m, 0)) * cot.to(device)).sum().backward()
    got = {"x": xd.grad}
    got.update({k: p.grad for k, p in zip(training.FMT_BLOCK_PARAMS, block_params(m, 0))})
    worst = max(worst, worst_rel(got, block_oracle(sd, 0, x, cot, pe=pe.cpu()), "self block"))
    # a cross block: four views, two per reference view
    x, ref, cot = (torch.randn(n, 64, h, w, generator=g) for n in (4, 2, 4))
    xd, rd = x.clone().to(device).requires_grad_(True), ref.clone().to(device).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    (training.FmtBlockTrain.apply(xd, rd, None, 2, *block_params(m, 1)) * cot.to(device)).sum().backward()
    got = {"x": xd.grad, "ref": rd.grad}
    got.update({k: p.grad for k, p in zip(training.FMT_BLOCK_PARAMS, block_params(m, 1))})
    worst = max(worst, worst_rel(got, block_oracle(sd, 1, x, cot, ref=ref, kv_div=2), "cross block"))
    return worst


def test_block_backward_against_fp64(emu):
    worst = check_blocks(emu)
    print("FMT block backward vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (worst, BAR))


# ---- whole module --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_module_backward_against_fp64(emu, case):
    worst = check_module_case(case, emu)
    print("fmt_forward_train vs fp64, case %s: worst |error| = %.3g x max|g64| over 70 gradients (bar %g)" % (case, worst, BAR))


def test_single_view(emu):
    """V = 1: only the reference view's self layers run; the cross layers' parameters get no gradient (None or exact zeros)."""
    fx, _, cfg = fixture()
    m = trainable()
    feats = {s: t[:, :1].clone().requires_grad_(True) for s, t in T.inputs(fx, "b").items()}
    _, grads = native_grads(m, feats)
    want = dict(oracle("b", 1)[1])
    cross = tuple("FMT.layers.%d." % i for i, n in enumerate(cfg["layer_names"]) if n == "cross")
    for k in [k for k in grads if isinstance(k, str) and k.startswith(cross)]:
        g = grads.pop(k)
        assert g is None or not bool(g.any()), k
        assert want.pop(k) is None
    worst_rel(grads, want, "V = 1")


def test_train_forward_is_the_eval_forward_bit_for_bit(emu):
    fx, sd, cfg = fixture()
    ev = T.module(fx)
    for mode in (True, False):
        m = trainable(train=mode)
        for case in ("a", "b"):
            feats = T.inputs(fx, case)
            with torch.no_grad():
                want = ev(feats)
            got = training.fmt_forward_train(m, {s: t.clone().requires_grad_(True) for s, t in feats.items()})
            via_module = m({s: t.clone().requires_grad_(mode is False) for s, t in feats.items()})
            for s in STAGES:
                assert got[s].requires_grad and torch.equal(got[s].detach(), want[s]), (mode, case, s)
                assert torch.equal(via_module[s].detach(), want[s]), (mode, case, s)
    with torch.no_grad():                                          # eval mode, nothing to differentiate: the inference path itself
        out = trainable(train=False)(T.inputs(fx, "b"))
    assert all(torch.equal(out[s], want[s]) and not out[s].requires_grad for s in STAGES)


def test_input_dtypes(emu):
    """A bf16 input is widened once and gets a bf16 gradient = the widened run's, rounded; an input that needs no gradient gets none."""
    fx, _, _ = fixture()
    m = trainable()
    base = T.inputs(fx, "b")
    base["stage3"] = base["stage3"].to(torch.bfloat16)
    wide = {s: t.detach().clone().float().requires_grad_(s != "stage2") for s, t in base.items()}
    mixed = {s: t.detach().clone().requires_grad_(s != "stage2") for s, t in base.items()}
    _, gw = native_grads(m, wide)
    out, gm = native_grads(m, mixed)
    assert all(out[s].dtype == torch.float32 for s in STAGES)
    assert gm[("in", "stage2")] is None and gw[("in", "stage2")] is None
    assert gm[("in", "stage3")].dtype == torch.bfloat16 and torch.equal(gm[("in", "stage3")], gw[("in", "stage3")].to(torch.bfloat16))
    for s in ("stage1", "stage4"):
        assert gm[("in", s)].dtype == torch.float32 and torch.equal(gm[("in", s)], gw[("in", s)])


def test_double_backward_is_refused(emu):
    fx, _, _ = fixture()
    m = trainable()
    feats = {s: t[:1, :1].clone().requires_grad_(True) for s, t in T.inputs(fx, "b").items()}
    out = m(feats)
    v = torch.ones_like(out["stage2"]).requires_grad_(True)              # a cotangent that itself asks for a gradient
    (g,) = torch.autograd.grad(out["stage2"], feats["stage1"], grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- contract ------------------------------------------------------------------------------------------------------------------------
def test_patch_fmt_trainable():
    for mode in (True, False):
        net = T._StandIn().train(mode)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        assert patch_fmt(net, trainable=True) is net
        assert type(net.FMT_module) is TrainableFMT_with_pathway and net.FMT_module.training is mode
        after = net.FMT_module.state_dict()
        assert len(after) == 66
        for k, v in after.items():
            assert torch.equal(v, before["FMT_module." + k]), k
    net = patch_fmt(T._StandIn().train())
    assert type(net.FMT_module) is FMT_with_pathway                     # the default still installs the form that refuses to train
    with pytest.raises(RuntimeError, match="reference's models/FMT.py"):
        net.FMT_module({"stage1": torch.zeros(1, 1, 64, 2, 3), "stage2": torch.zeros(1, 1, 32, 4, 6), "stage3": torch.zeros(1, 1, 16, 8, 12),
                        "stage4": torch.zeros(1, 1, 8, 16, 24)})
    import mvsformerplusplus_amd as pkg
    assert pkg.TrainableFMT_with_pathway is TrainableFMT_with_pathway and pkg.fmt_forward_train is training.fmt_forward_train


def test_same_refusals_and_a_larger_position_cache():
    _, _, cfg = fixture()
    with pytest.raises(NotImplementedError, match="attention_type"):
        TrainableFMT_with_pathway(**dict(cfg, attention_type="FLASH2"))
    with pytest.raises(NotImplementedError, match="base_channel"):
        TrainableFMT_with_pathway(**dict(cfg, base_channel=4))
    m = TrainableFMT_with_pathway(**cfg)
    with pytest.raises(ValueError, match="stage1..stage4"):
        m({"stage1": torch.zeros(1, 2, 64, 2, 3), "stage2": torch.zeros(1, 2, 16, 4, 6), "stage3": torch.zeros(1, 2, 16, 8, 12),
           "stage4": torch.zeros(1, 2, 8, 16, 24)})
    base = FMT_with_pathway(**cfg)
    for i in range(40):                                                # the shipped multi-scale training list has 25 sizes
        m.FMT.position_encoding(2, 3 + i, "cpu")
        base.FMT.position_encoding(2, 3 + i, "cpu")
    assert len(m.FMT._pe) == fmt.TRAIN_PE_CACHE_ENTRIES == 32 and len(base.FMT._pe) == fmt.PE_CACHE_ENTRIES == 8
    assert (2, 3 + 39, "cpu") in m.FMT._pe and (2, 3 + 8, "cpu") in m.FMT._pe and (2, 3 + 7, "cpu") not in m.FMT._pe


def test_entry_point_refusals(emu):
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.fmt_path_bwd(torch.zeros(1, 4, 4, 4), torch.zeros(1, 8, 2, 2), torch.zeros(4, 8))
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.fmt_smooth_wgrad(torch.zeros(1, 24, 4, 4), torch.zeros(1, 48, 2, 2), torch.zeros(1, 24, 4, 4), torch.zeros(24, 48))
    with pytest.raises(AssertionError):
        ops.fmt_path_bwd(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 2, 2), torch.zeros(8, 16))          # prev must have 2C channels
    with pytest.raises(ValueError, match="lateral's shape"):
        ops.fmt_smooth_wgrad(torch.zeros(1, 8, 4, 5), torch.zeros(1, 16, 2, 2), torch.zeros(1, 8, 4, 4), torch.zeros(8, 16))
    L = _lib.lib()
    assert L.mvs_fmt_path_bwd_workspace_bytes(1, 12, 4, 4) == 0 and L.mvs_fmt_smooth_wgrad_workspace_bytes(70000, 8, 4, 4) == 0
    assert L.mvs_fmt_path_bwd_workspace_bytes(3, 8, 16, 16) == 3 * 8 * 16 * 4           # one partial per 256 coarse pixels
    assert L.mvs_fmt_path_bwd_workspace_bytes(64, 32, 64, 64) == 256 * 32 * 64 * 4      # capped at 8192 / C partials


def test_host_tensors_are_refused(monkeypatch, emu_lib):
    """No CPU route in training either: with the device requirement in force a host tensor raises before any launch."""
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    assert _lib._REQUIRE_DEVICE
    fx, _, cfg = fixture()
    m = TrainableFMT_with_pathway(**cfg).train()
    feats = {s: t[:1, :1].clone().requires_grad_(True) for s, t in T.inputs(fx, "b").items()}
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        m(feats)
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        ops.fmt_path_bwd(torch.zeros(1, 8, 4, 4), torch.zeros(1, 16, 2, 2), torch.zeros(8, 16))
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        ops.fmt_smooth_wgrad(torch.zeros(1, 8, 4, 4), torch.zeros(1, 16, 2, 2), torch.zeros(1, 8, 4, 4), torch.zeros(8, 16))


# ---- fixture F32: the oracle's gradients are the reference's own --------------------------------------------------------------------
def test_restatement_gradients_pinned_to_f32():
    """tests/fmt_ref.py's fp64 gradients against the reference's own FMT_with_pathway in train mode (fp32, CPU; fixture F32): 1e-4 x
    max|g| per tensor - the reference is itself fp32.  Its train-mode outputs are F26's eval outputs, byte for byte."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "f32_fmt_train_*.npz")))
    f32 = {}
    for path in files:
        assert os.path.getsize(path) < 1024 * 1024
        f32.update({k: v for k, v in load_golden(os.path.basename(path)).items() if k != "__name__"})
    assert int(f32["cot.seed"]) == COT_SEED
    fx, _, _ = fixture()
    h = hashlib.sha256()
    for s in STAGES:
        h.update(fx["a/out_" + s].contiguous().numpy().tobytes())
    assert h.hexdigest() == f32["out.sha256"]
    _, grads = oracle("a")
    ref = {(("in", k[len("g/in/"):]) if k.startswith("g/in/") else k[len("g/"):]): v for k, v in f32.items() if k.startswith("g/")}
    assert len(ref) == 70 and sorted(map(str, ref)) == sorted(map(str, grads))
    worst = 0.0
    for k, w in ref.items():
        rel = float((grads[k] - w.double()).abs().max()) / float(w.abs().max())
        assert rel <= 1e-4, (k, rel)
        worst = max(worst, rel)
    assert min(float(g.abs().max()) for g in grads.values()) > 1.0          # no degenerate gradient among the 70
    print("fmt_ref fp64 gradients vs the reference's fp32 autograd (F32): worst %.3g x max|g|" % worst)
