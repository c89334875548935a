"""CPU: training of the FPN decoder (mvsformerplusplus_amd.training.fpn_decoder_forward_train, features.TrainableFPNDecoder, DESIGN.md
section 4.18) on the host emulator against fp64 autograd through the restatement tests/fpn_train_ref.py, which is itself pinned to
fixture F33 (the reference's own FPNDecoder in train mode, tests/golden/make_golden_fpn_train.py).

Bars.  Every non-trivial gradient tensor g (4 inputs, 18 parameters): max|g - g64| <= MODULE_BAR x max|g64|, MODULE_BAR = 2e-4 (the
project's bar for this arithmetic, tests/test_fpn.py, tests/test_fmt_train.py); plain fp32 PyTorch autograd of the same decoder sits at
1.1e-6 / 6.3e-6 / 1.3e-5 on the three shapes.  The four out_k.0.bias gradients are exactly zero (a bias in front of a batch-statistics
BatchNorm).  Train-mode outputs: test_fpn.within_range at 2e-4.  Running statistics: test_fpn.LAYER_BAR x max(1, max|ref|);
num_batches_tracked exact.  Measured for the native path on the emulator, worst tensor: whole decoder 1.4e-5 / 1.4e-5 / 1.5e-5 (cases a / b /
c), heads 9.4e-6, merges 5.4e-6, fused level 3 1.4e-5, the chain into the FMT 2.9e-5; on an MI355X 1.5e-5 / 1.7e-5 / 1.8e-5, 9.2e-6, 5.4e-6,
1.4e-5, 3.4e-5 (tests/test_fpn_train_gpu.py).  Outputs 6.0e-6 of their range, running statistics 2.1e-6."""
import functools
import glob
import hashlib
import os

import pytest
import torch

import fpn_train_ref as R
import test_fpn as T
from conftest import GOLDEN, load_golden
from mvsformerplusplus_amd import _lib, ops, training
from mvsformerplusplus_amd.features import FPNDecoder, TrainableFPNDecoder, patch_fpn

BAR = T.MODULE_BAR
INPUTS = ("conv01", "conv11", "conv21", "conv31")
ZERO_GRADS = tuple("out%d.0.bias" % k for k in range(4))
IN_SEED, COT_SEED = 330, 33                # fixture F33's
CASES = {"a": (2, 2, 3),                   # (N, h, w) of conv31; full resolution 16 x 24: one 4 x 64 tile column
         "b": (2, 3, 9),                   # 24 x 72: a ragged second tile column
         "c": (3, 5, 17),                  # 40 x 136: three tile columns, ragged, N > 1, several partials
         "f33": (2, 4, 6)}


def input_shapes(n, h, w):
    return [(n, 8, 8 * h, 8 * w), (n, 16, 4 * h, 4 * w), (n, 32, 2 * h, 2 * w), (n, 64, h, w)]


def inputs(case, seed=IN_SEED):
    """Standard normals drawn in the order conv01, conv11, conv21, conv31 (F33's recipe at any size)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in input_shapes(*(CASES[case] if isinstance(case, str) else case))]


def cotangents(outs, seed=COT_SEED):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) for o in outs]


@functools.lru_cache(maxsize=None)
def weights():
    return T.f25_weights(T.f25(), "dec.")


def worst_rel(got, want, what, bar=BAR):
    """max |got - want| / max |want| per tensor -> the worst; asserts the bar for each.  The out_k.0.bias entries must be exact zeros."""
    worst = 0.0
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        assert g is not None and tuple(g.shape) == tuple(w.shape), (what, k)
        if k in ZERO_GRADS:
            assert not bool(g.any()), (what, k)
            continue
        rel = float((g.double().cpu() - w).abs().max()) / float(w.abs().max())
        assert rel <= bar, (what, k, rel, bar)
        worst = max(worst, rel)
    return worst


@functools.lru_cache(maxsize=None)
def oracle(case):
    """fp64 autograd through tests/fpn_train_ref.py -> (outputs, {("in", name) | parameter key: gradient}, updated running statistics);
    computed once per case and shared (read-only)."""
    sd = weights()
    sd64 = {k: (v.double().requires_grad_(True) if k in R.PARAMS else v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    xs = [x.double().requires_grad_(True) for x in inputs(case)]
    running = {}
    outs = R.decoder(*xs, sd64, running=running)
    sum((o * c.double()).sum() for o, c in zip(outs, cotangents(outs))).backward()
    grads = {("in", n): x.grad for n, x in zip(INPUTS, xs)}
    grads.update({k: sd64[k].grad for k in R.PARAMS})
    return [o.detach() for o in outs], grads, running


def trainable(device="cpu", train=True):
    m = TrainableFPNDecoder([8, 16, 32, 64])
    m.load_state_dict(weights(), strict=True)
    return m.train(train).to(device)


def native_step(m, xs):
    """forward + backward of the native module with the seeded cotangent -> (outputs, gradients keyed like oracle()'s)."""
    m.zero_grad(set_to_none=True)
    outs = m(*xs)
    sum((o * c.to(o.device)).sum() for o, c in zip(outs, cotangents(outs))).backward()
    grads = {("in", n): x.grad for n, x in zip(INPUTS, xs)}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return outs, grads


def check_running(m, want, what):
    worst = 0.0
    buffers = dict(m.named_buffers())
    assert set(buffers) == set(want) and len(want) == 12
    for k, w in want.items():
        if k.endswith("num_batches_tracked"):
            assert int(buffers[k]) == int(w), (what, k)
        else:
            worst = max(worst, T.close(buffers[k].detach().cpu(), w, T.LAYER_BAR, (what, k)))
    return worst


def check_module_case(case, device):
    """One training step on `device` against the fp64 oracle -> (worst gradient ratio, worst output fraction, worst running-stat error)."""
    m = trainable(device)
    xs = [x.clone().to(device).requires_grad_(True) for x in inputs(case)]
    outs, grads = native_step(m, xs)
    want_out, want, want_run = oracle(case)
    assert len(want) == 26
    frac = 0.0
    for k, o in enumerate(outs):
        assert o.dtype == torch.float32 and o.is_contiguous()
        frac = max(frac, T.within_range(o.detach().cpu(), want_out[k], BAR, (case, "out%d" % k)))
    run = check_running(m, want_run, case)
    before = {k: v.clone() for k, v in m.named_buffers()}
    m(*[x.detach() for x in xs])                                             # a second step moves the statistics again
    for k, v in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1
        else:
            assert not torch.equal(v, before[k]), k
    return worst_rel(grads, want, "module case " + case), frac, run


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_module_backward_against_fp64(emu, case):
    worst, frac, run = check_module_case(case, emu)
    print("fpn_decoder_forward_train vs fp64, case %s: worst gradient |error| = %.3g x max|g64| over 22 tensors (bar %g); outputs %.3g of their "
          "range; running statistics %.3g" % (case, worst, BAR, frac, run))


# ---- single nodes --------------------------------------------------------------------------------------------------------------------
def _bn(c, device):
    bn = torch.nn.BatchNorm2d(c).to(device).train()
    g = torch.Generator().manual_seed(c)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


def _node_sd(name, w, b, gamma, beta, bn):
    return {name + ".0.weight": w, name + ".0.bias": b, name + ".1.weight": gamma, name + ".1.bias": beta,
            name + ".1.running_mean": bn.running_mean.detach().cpu().double(), name + ".1.running_var": bn.running_var.detach().cpu().double(),
            name + ".1.num_batches_tracked": bn.num_batches_tracked.detach().cpu().clone()}


def _leaves(ts, device=None):
    if device is None:
        return [t.detach().double().requires_grad_(True) for t in ts]
    return [t.clone().to(device).requires_grad_(True) for t in ts]


def check_heads(device):
    worst = 0.0
    for case in ("a", "b", "c"):
        n, h, w = CASES[case]
        for k, (cout, ks, scale) in enumerate(((64, 1, 1), (32, 3, 2), (16, 3, 4))):
            g = torch.Generator().manual_seed(10 * k + n + h)
            x = torch.randn(n, 64, scale * h, scale * w, generator=g)
            wt, b = torch.randn(cout, 64, ks, ks, generator=g) / (64 * ks * ks) ** 0.5, torch.randn(cout, generator=g)
            gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
            cot = torch.randn(n, cout, scale * h, scale * w, generator=g)
            bn = _bn(cout, device)
            names = ("x", "w", "b", "gamma", "beta")
            ref = _leaves((x, wt, b, gamma, beta))
            running = {}
            y64 = R.head(ref[0], _node_sd("h", *ref[1:], bn), "h", ks // 2, running)
            (y64 * cot.double()).sum().backward()
            got = _leaves((x, wt, b, gamma, beta), device)
            y = training.FpnHeadTrain.apply(got[0], bn, *got[1:])
            (y * cot.to(device)).sum().backward()
            T.within_range(y.detach().cpu(), y64.detach(), BAR, ("head", case, k))
            T.close(bn.running_mean.cpu(), running["h.1.running_mean"], T.LAYER_BAR, ("head running_mean", case, k))
            T.close(bn.running_var.cpu(), running["h.1.running_var"], T.LAYER_BAR, ("head running_var", case, k))
            assert not bool(got[2].grad.any())
            pairs = {nm: (a.grad, r.grad) for nm, a, r in zip(names, got, ref) if nm != "b"}
            worst = max(worst, worst_rel({k_: v[0] for k_, v in pairs.items()}, {k_: v[1] for k_, v in pairs.items()}, ("head", case, k)))
    return worst


def check_merges(device):
    worst = 0.0
    for case in ("a", "b", "c"):
        n, h, w = CASES[case]
        for k, (clat, scale) in ((1, (32, 1)), (2, (16, 2))):
            g = torch.Generator().manual_seed(20 * k + n + h)
            prev, lat = torch.randn(n, 64, scale * h, scale * w, generator=g), torch.randn(n, clat, 2 * scale * h, 2 * scale * w, generator=g)
            wi, bi = torch.randn(64, clat, 1, 1, generator=g) / clat ** 0.5, torch.randn(64, generator=g)
            cot = torch.randn(n, 64, 2 * scale * h, 2 * scale * w, generator=g)
            names = ("prev", "lat", "w_inner", "b_inner")
            ref = _leaves((prev, lat, wi, bi))
            y64 = R.merge(ref[0], ref[1], {"inner%d.weight" % k: ref[2], "inner%d.bias" % k: ref[3]}, k)
            (y64 * cot.double()).sum().backward()
            got = _leaves((prev, lat, wi, bi), device)
            y = training.FpnMergeTrain.apply(*got)
            (y * cot.to(device)).sum().backward()
            T.close(y.detach().cpu(), y64.detach(), T.LAYER_BAR, ("merge", case, k))
            worst = max(worst, worst_rel(dict(zip(names, (t.grad for t in got))), dict(zip(names, (t.grad for t in ref))), ("merge", case, k)))
    return worst


def level3_case(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    prev, lat = torch.randn(n, 64, 4 * h, 4 * w, generator=g), torch.randn(n, 8, 8 * h, 8 * w, generator=g)
    wi, bi = torch.randn(64, 8, 1, 1, generator=g) / 8 ** 0.5, torch.randn(64, generator=g)
    wt, b = torch.randn(8, 64, 3, 3, generator=g) / 576 ** 0.5, torch.randn(8, generator=g)
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    return (prev, lat, wi, bi, wt, b, gamma, beta), torch.randn(n, 8, 8 * h, 8 * w, generator=g)


LEVEL3_NAMES = ("prev", "lat", "w_inner", "b_inner", "w", "b", "gamma", "beta")


def check_level3(device):
    worst = 0.0
    for case in ("a", "b", "c"):
        n, h, w = CASES[case]
        ts, cot = level3_case(n, h, w, 30 + n + h)
        bn = _bn(8, device)
        ref = _leaves(ts)
        sd = _node_sd("h", *ref[4:], bn)
        sd.update({"inner3.weight": ref[2], "inner3.bias": ref[3]})
        y64 = R.head(R.merge(ref[0], ref[1], sd, 3), sd, "h", 1, {})
        (y64 * cot.double()).sum().backward()
        got = _leaves(ts, device)
        y = training.FpnLevel3Train.apply(got[0], got[1], bn, *got[2:])
        (y * cot.to(device)).sum().backward()
        T.within_range(y.detach().cpu(), y64.detach(), BAR, ("level 3", case))
        assert not bool(got[5].grad.any())
        pairs = {nm: (a.grad, r.grad) for nm, a, r in zip(LEVEL3_NAMES, got, ref) if nm != "b"}
        worst = max(worst, worst_rel({k: v[0] for k, v in pairs.items()}, {k: v[1] for k, v in pairs.items()}, ("level 3", case)))
    return worst


def test_head_nodes_against_fp64(emu):
    print("FpnHeadTrain vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_heads(emu), BAR))


def test_merge_nodes_against_fp64(emu):
    print("FpnMergeTrain vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_merges(emu), BAR))


def test_fused_level3_node_against_fp64(emu):
    print("FpnLevel3Train vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_level3(emu), BAR))


def test_upsample_adjoint_identity(emu):
    """<U a, b> = <a, U^T b>: mvs_fpn_up2_adjoint gathers with the weights the forward's merge evaluates."""
    for n, h, w in ((1, 1, 1), (2, 1, 4), (2, 3, 9), (1, 5, 33)):
        g = torch.Generator().manual_seed(h * w)
        a, b = torch.randn(n, 64, h, w, generator=g), torch.randn(n, 64, 2 * h, 2 * w, generator=g)
        ua = ops.fpn_merge(a, torch.zeros(n, 8, 2 * h, 2 * w), torch.zeros(64, 8), torch.zeros(64)).double()
        lhs, rhs = (ua * b.double()).sum(), (a.double() * ops.fpn_up2_adjoint(b).double()).sum()
        assert abs(float(lhs - rhs)) <= 1e-5 * float((ua.abs() * b.double().abs()).sum()), (n, h, w, float(lhs), float(rhs))


# ---- module contract -----------------------------------------------------------------------------------------------------------------
def test_eval_forward_is_the_inference_forward_bit_for_bit(emu):
    fx = T.f25()
    _, dec = T.modules(fx)
    m = trainable(train=False)
    xs = [fx["b/" + n] for n in INPUTS]
    with torch.no_grad():
        want, got = dec(*xs), m(*xs)
    for a, b in zip(got, want):
        assert torch.equal(a, b) and not a.requires_grad
    with pytest.raises(RuntimeError, match="frozen"):
        m(*[x.clone().requires_grad_(True) for x in xs])
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert sorted(before) == sorted(weights())
    for k, v in before.items():
        assert torch.equal(v, weights()[k]), k                      # strict load, eval forward leaves the buffers alone


def test_patch_fpn_trainable_decoder():
    for mode in (True, False):
        net = T._StandIn().train(mode)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        enc = net.encoder
        others = {n: getattr(net, n) for n in ("vit", "decoder_vit", "FMT_with_pathway", "fusions")}
        assert patch_fpn(net, trainable_decoder=True) is net
        assert type(net.decoder) is TrainableFPNDecoder and net.decoder.training is mode and net.encoder is enc
        for n, mod in others.items():
            assert getattr(net, n) is mod
        after = net.state_dict()
        assert sorted(after) == sorted(before)
        for k, v in before.items():
            assert torch.equal(after[k], v), k
    net = patch_fpn(T._StandIn().train())                                    # the default still installs the forms that refuse to train
    assert type(net.decoder) is FPNDecoder
    feats = [torch.zeros(1, 8, 16, 16), torch.zeros(1, 16, 8, 8), torch.zeros(1, 32, 4, 4), torch.zeros(1, 64, 2, 2)]
    with pytest.raises(RuntimeError, match="FPNDecoder"):
        net.decoder(*feats)
    with pytest.raises(RuntimeError, match="FPNDecoder"):
        FPNDecoder([8, 16, 32, 64])(*feats)
    import mvsformerplusplus_amd as pkg
    assert pkg.TrainableFPNDecoder is TrainableFPNDecoder and pkg.fpn_decoder_forward_train is training.fpn_decoder_forward_train


def test_input_dtypes(emu):
    """A bf16 input is widened once and gets a bf16 gradient = the widened run's, rounded; an input that needs no gradient gets none."""
    base = inputs("a")
    base[1] = base[1].to(torch.bfloat16)
    wide = [t.detach().clone().float().requires_grad_(i != 2) for i, t in enumerate(base)]
    mixed = [t.detach().clone().requires_grad_(i != 2) for i, t in enumerate(base)]
    _, gw = native_step(trainable(), wide)
    outs, gm = native_step(trainable(), mixed)
    assert all(o.dtype == torch.float32 for o in outs)
    assert gm[("in", "conv21")] is None and gw[("in", "conv21")] is None
    assert gm[("in", "conv11")].dtype == torch.bfloat16 and torch.equal(gm[("in", "conv11")], gw[("in", "conv11")].to(torch.bfloat16))
    for n in ("conv01", "conv31"):
        assert gm[("in", n)].dtype == torch.float32 and torch.equal(gm[("in", n)], gw[("in", n)])


def test_refusals(emu, monkeypatch):
    m = trainable()
    xs = [x.requires_grad_(True) for x in inputs("a")]
    outs = m(*xs)
    v = torch.ones_like(outs[1]).requires_grad_(True)                        # a cotangent that itself asks for a gradient
    (g,) = torch.autograd.grad(outs[1], xs[3], grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    with pytest.raises(ValueError, match="twice"):
        m(xs[0], xs[1], xs[2], torch.zeros(2, 64, 3, 3))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="SyncBatchNorm"):
        m(*xs)


def test_entry_point_refusals(emu):
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.fpn_train_conv(torch.zeros(1, 24, 4, 4), torch.zeros(24, 24, 3, 3))
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_wgrad(torch.zeros(1, 24, 4, 4), torch.zeros(1, 64, 4, 4), 3)
    with pytest.raises(_lib.MvsHipError, match="bad arguments"):
        ops.fpn_up2_adjoint(torch.zeros(1, 64, 0, 4))
    with pytest.raises(AssertionError):
        ops.fpn_up2_adjoint(torch.zeros(1, 64, 3, 4))
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_bn_swish_fwd(torch.zeros(1, 65, 2, 2), torch.ones(65), torch.zeros(65), 1e-5)
    assert ops.fpn_train_conv_is_built(32, 64, 3) and ops.fpn_train_conv_is_built(8, 8, 3) and not ops.fpn_train_conv_is_built(64, 8, 3)
    for ci, co, k, s in ((64, 8, 3, 1), (64, 64, 1, 1), (3, 8, 7, 1)):      # the inference list is what it was
        assert ops.fpn_conv_is_built(ci, co, k, s)
    assert not ops.fpn_conv_is_built(32, 64, 3, 1) and not ops.fpn_conv_is_built(8, 8, 3, 1)
    L = _lib.lib()
    assert L.mvs_fpn_wgrad_workspace_bytes(1, 64, 32, 3, 0, 4, 64) == 2 * 32 * 576 * 4          # one partial per 2 x 64 tile
    assert L.mvs_fpn_wgrad_workspace_bytes(64, 64, 32, 3, 0, 256, 256) == 113 * 32 * 576 * 4    # capped at 8 MiB of partials
    assert L.mvs_fpn_wgrad_workspace_bytes(1, 64, 32, 3, 1, 4, 64) == 0 and L.mvs_fpn_bn_workspace_bytes(1, 65, 4, 4) == 0


def test_host_tensors_are_refused(monkeypatch, emu_lib):
    """No CPU route in training either: with the device requirement in force a host tensor raises before any launch."""
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    assert _lib._REQUIRE_DEVICE
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        trainable()(*[x.requires_grad_(True) for x in inputs("a")])
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        ops.fpn_up2_adjoint(torch.zeros(1, 64, 4, 4))


# ---- chain: decoder -> FMT_with_pathway ---------------------------------------------------------------------------------------------
CHAIN = (3, 8, 12)                          # conv31 [3, 64, 8, 12]: B = 1, V = 3


@functools.lru_cache(maxsize=None)
def chain_oracle():
    import fmt_ref
    import test_fmt_train as FT
    _, fsd, cfg = FT.fixture()
    sd64 = {k: (v.double().requires_grad_(True) if k in R.PARAMS else v.double() if v.is_floating_point() else v) for k, v in weights().items()}
    xs = [x.double().requires_grad_(True) for x in inputs(CHAIN)]
    outs = R.decoder(*xs, sd64)
    out = fmt_ref.fmt({"stage%d" % (k + 1): o.unsqueeze(0) for k, o in enumerate(outs)}, {k: v.double() for k, v in fsd.items()}, cfg["layer_names"])
    cot = FT.cotangents({s: out[s].shape for s in FT.STAGES})
    sum((out[s] * cot[s].double()).sum() for s in FT.STAGES).backward()
    grads = {("in", n): x.grad for n, x in zip(INPUTS, xs)}
    grads.update({k: sd64[k].grad for k in R.PARAMS})
    return grads


def check_chain(device):
    import test_fmt_train as FT
    dec, fmt = trainable(device), FT.trainable(device)
    xs = [x.clone().to(device).requires_grad_(True) for x in inputs(CHAIN)]
    out = fmt({"stage%d" % (k + 1): o.unsqueeze(0) for k, o in enumerate(dec(*xs))})
    cot = FT.cotangents({s: out[s].shape for s in FT.STAGES})
    sum((out[s] * cot[s].to(device)).sum() for s in FT.STAGES).backward()
    grads = {("in", n): x.grad for n, x in zip(INPUTS, xs)}
    grads.update({k: p.grad for k, p in dec.named_parameters()})
    return worst_rel(grads, chain_oracle(), "decoder -> FMT chain")


def test_chain_into_fmt_against_fp64(emu):
    print("FPNDecoder -> FMT_with_pathway chain vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_chain(emu), BAR))


# ---- fixture F33: the oracle's gradients are the reference's own --------------------------------------------------------------------
def test_restatement_pinned_to_f33():
    """tests/fpn_train_ref.py's fp64 gradients and running statistics against the reference's own FPNDecoder in train mode (fp32, CPU;
    fixture F33).  Gradients: test_fmt_train's 2e-4 x max|g| per tensor; the four out_k.0.bias entries, where the reference's values are
    rounding noise around zero, |g| <= 1e-4 absolutely on both sides."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "f33_fpn_decoder_train_*.npz")))
    f33 = {}
    for path in files:
        assert os.path.getsize(path) < 1024 * 1024
        f33.update({k: v for k, v in load_golden(os.path.basename(path)).items() if k != "__name__"})
    assert int(f33["in.seed"]) == IN_SEED and int(f33["cot.seed"]) == COT_SEED and tuple(int(v) for v in f33["in.shape"]) == CASES["f33"]
    h = hashlib.sha256()
    for x in inputs("f33"):
        h.update(x.contiguous().numpy().tobytes())
    assert h.hexdigest() == f33["in.sha256"], "torch's CPU generator changed: regenerate F33 (tests/golden/make_golden_fpn_train.py)"
    _, grads, running = oracle("f33")
    ref = {(("in", k[len("g/in/"):]) if k.startswith("g/in/") else k[len("g/"):]): v for k, v in f33.items() if k.startswith("g/")}
    assert len(ref) == 26 and sorted(map(str, ref)) == sorted(map(str, grads))
    worst = 0.0
    for k, w in ref.items():
        if k in ZERO_GRADS:
            assert float(w.abs().max()) <= 1e-4 and float(grads[k].abs().max()) <= 1e-4, k
            continue
        rel = float((grads[k] - w.double()).abs().max()) / float(w.abs().max())
        assert rel <= 2e-4, (k, rel)
        worst = max(worst, rel)
    run = {k[len("run/"):]: v for k, v in f33.items() if k.startswith("run/")}
    assert len(run) == 12 and set(run) == set(running)
    for k, w in run.items():
        if k.endswith("num_batches_tracked"):
            assert int(w) == int(running[k])
        else:
            T.close(running[k], w, T.LAYER_BAR, k)
    print("fpn_train_ref fp64 gradients vs the reference's fp32 autograd (F33): worst %.3g x max|g|" % worst)
