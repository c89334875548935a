"""CPU: training of the FPN encoder (mvsformerplusplus_amd.training.fpn_encoder_forward_train, features.TrainableFPNEncoder, DESIGN.md
section 4.19) on the host emulator against fp64 autograd through the restatement tests/fpn_encoder_train_ref.py, which is itself pinned
to fixture F34 (the reference's own FPNEncoder in train mode, tests/golden/make_golden_fpn_encoder_train.py).

Bars.  Every gradient tensor g: max|g - g64| <= MODULE_BAR x max|g64|, MODULE_BAR = 2e-4 (the project's bar and the decoder's,
tests/test_fpn_train.py).  Train-mode outputs: test_fpn.within_range at 2e-4.  Running statistics: test_fpn.LAYER_BAR x max(1, max|ref|);
num_batches_tracked exact.

The LeakyReLU kink.  An fp32 run and the fp64 oracle may disagree on the sign of a pre-activation u = gamma xhat + beta that lies within
rounding of zero, and one such flip changes a weight gradient of a small case by percent.  So the linear kernels (weight and data
gradients) are tested WITHOUT the activation, against fp64 F.conv2d autograd on random dz and x, at the shapes that reach every index path;
and everything that contains the activation runs on inputs whose seeds are written below and for which the fp64 oracle's own
pre-activations satisfy min |u64| >= DELTA - asserted on the oracle, so that a bad seed fails loudly; nothing is ever excluded from a
comparison.  DELTA = 4 E with E = max |u_native - u64| over the 11 blocks of the module case, u_native from the same ops calls the
forward makes (measure_u_error): E = 1.3874e-4 on the emulator (per block it grows with depth, 1.9e-5 at conv00 to 1.4e-4 at conv31),
DELTA = 5.55e-4.  A flip needs an error above |u64|, and the decoder's device run sat within 1.3 x of its emulator run.  The seeds were
searched on the CPU with the fp64 oracle alone: the first seed from 0 that meets the condition.

The module case is [2, 3, 16, 16], not [2, 3, 16, 24]: at 16 x 24 E was 1.65e-4 and none of 6000 seeds reached 4 E (best min |u64|
3.9e-4 over 28 k pre-activations), so the shape was shrunk, never DELTA; [2, 3, 8, 16] is no way out, its 4 samples per channel at the last
level make BatchNorm amplify E to 1.4e-3.  At 16 x 16 (19 k pre-activations, 8 samples per channel at the last level) E depends on the
input (1.3e-4 .. 4.7e-4 over the candidates), so a seed is taken when min |u64| >= 4 E holds for E measured ON THAT SEED: of 240000 seeds
47 had min |u64| >= 5e-4 and two of those met it, 29275 (min |u64| 5.598e-4, E 1.3874e-4) and 77814.  Fixture F34 is generated at this
shape and seed.  Larger module shapes cannot meet the condition, which is why tiling is tested on the linear pieces.

Measured on the emulator, worst tensor x max|g64|: see the figures each test prints; on an MI355X: tests/test_fpn_encoder_train_gpu.py."""
import functools
import glob
import hashlib
import os

import pytest
import torch
import torch.nn.functional as F

import fpn_encoder_train_ref as R
import test_fpn as T
from conftest import GOLDEN, load_golden
from mvsformerplusplus_amd import _lib, ops, training
from mvsformerplusplus_amd.features import FPNEncoder, TrainableFPNDecoder, TrainableFPNEncoder, patch_fpn

BAR = T.MODULE_BAR
E_MEASURED = 1.3874e-4                        # max |u_native - u64| over the module case's 11 blocks on the emulator (measure_u_error)
DELTA = 4 * E_MEASURED
SHAPE = (2, 3, 16, 16)                       # the module case = fixture F34's
IN_SEED, COT_SEED = 29275, 34                # F34's; IN_SEED meets min |u64| >= DELTA over all 11 blocks (5.598e-4)
# (Cout, Cin, k, stride) of the encoder's eight distinct layers
LAYERS = ((8, 3, 7, 1), (8, 8, 5, 1), (16, 8, 5, 2), (16, 16, 3, 1), (32, 16, 5, 2), (32, 32, 3, 1), (64, 32, 3, 2), (64, 64, 3, 1))
# output sizes (N, OH, OW) of the linear pieces: two tile columns with the second ragged and rows ragged for TH = 4 and TH = 2; the smallest;
# and enough tiles for several partials per launch
LINEAR_SHAPES = ((2, 5, 72), (1, 1, 1), (2, 2, 3), (3, 12, 136))
# BatchNorm + LeakyReLU alone: (C, N, H, W) -> the first seed whose fp64 pre-activations keep min |u64| >= DELTA
BN_CASES = {(8, 2, 5, 72): 1, (64, 2, 2, 3): 1, (8, 1, 20, 55): 9}
# one block node per distinct layer at output [2, Cout, 3, 5] -> seed, same condition
BLOCK_SEEDS = dict(zip(LAYERS, (0, 0, 0, 1, 1, 0, 1, 0)))


def assert_clear_of_the_kink(us, what):
    """The stated condition on the inputs, on the fp64 oracle's own pre-activations."""
    for name, u in (us.items() if isinstance(us, dict) else [("u", us)]):
        m = float(u.abs().min())
        assert m >= DELTA, ("seed does not meet min |u64| >= DELTA: search another on the CPU", what, name, m, DELTA)


def rel(got, want, what, bar=BAR):
    assert got is not None and tuple(got.shape) == tuple(want.shape), (what, None if got is None else tuple(got.shape), tuple(want.shape))
    r = float((got.detach().double().cpu() - want).abs().max()) / float(want.abs().max())
    assert r <= bar, (what, r, bar)
    return r


# ---- linear pieces: no activation, no kink --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_case(layer, shape):
    """Random x, w, dz of one layer at one output size and fp64 F.conv2d autograd's d_w and d_x; computed once and shared (read-only)."""
    cout, cin, k, s = layer
    n, oh, ow = shape
    g = torch.Generator().manual_seed(1000 * cout + 100 * cin + 10 * k + oh)
    x = torch.randn(n, cin, oh * s, ow * s, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    dz = torch.randn(n, cout, oh, ow, generator=g)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (F.conv2d(x64, w64, None, s, k // 2) * dz.double()).sum().backward()
    return x, w, dz, w64.grad, x64.grad


def check_wgrads(device, shapes=LINEAR_SHAPES):
    worst = 0.0
    for layer in LAYERS:
        for shape in shapes:
            x, w, dz, dw64, _ = linear_case(layer, shape)
            got = ops.fpn_enc_wgrad(dz.to(device), x.to(device), layer[2], layer[3])
            worst = max(worst, rel(got, dw64, ("wgrad", layer, shape)))
    return worst


def check_dgrads(device, shapes=LINEAR_SHAPES):
    worst = 0.0
    for layer in LAYERS[1:]:                                                 # conv00's data gradient is never computed
        for shape in shapes:
            x, w, dz, _, dx64 = linear_case(layer, shape)
            got = ops.fpn_enc_dgrad(dz.to(device), w.to(device), layer[3])
            worst = max(worst, rel(got, dx64, ("dgrad", layer, shape)))
    return worst


def check_dgrad_adjoint(device):
    """<conv(a), b> = <a, dgrad(b)> for the three stride-2 layers, conv = the native forward convolution, to 1e-5 of sum |conv(a)| |b|."""
    from mvsformerplusplus_amd import packing
    for layer in LAYERS:
        cout, cin, k, s = layer
        if s != 2:
            continue
        for shape in ((2, 5, 72), (2, 2, 3)):
            a, w, b, _, _ = linear_case(layer, shape)
            ca = ops.fpn_conv(a.to(device), packing.pack_fpn_conv_weights(w, 2).to(device), None, cout, k, 2, ops.FPN_ACT_NONE).double().cpu()
            lhs = (ca * b.double()).sum()
            rhs = (a.double() * ops.fpn_enc_dgrad(b.to(device), w.to(device), 2).double().cpu()).sum()
            assert abs(float(lhs - rhs)) <= 1e-5 * float((ca.abs() * b.double().abs()).sum()), (layer, shape, float(lhs), float(rhs))


def test_weight_gradients_against_fp64(emu):
    print("fpn_enc_wgrad vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_wgrads(emu), BAR))


def test_data_gradients_against_fp64(emu):
    print("fpn_enc_dgrad vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_dgrads(emu), BAR))


def test_stride2_data_gradient_is_the_adjoint(emu):
    check_dgrad_adjoint(emu)


def test_parity_class_taps():
    """packing.fpn_enc_dgrad_class_taps: the four 3x3 tap sets scatter back to exactly the layer's taps, each used once."""
    from mvsformerplusplus_amd import packing
    for k in (3, 5):
        w = torch.arange(1, 2 * 3 * k * k + 1, dtype=torch.float32).reshape(2, 3, k, k)
        taps = packing.fpn_enc_dgrad_class_taps(w)
        assert taps.shape == (4, 3, 2, 3, 3)
        assert sorted(taps[taps != 0].tolist()) == sorted(w.flatten().tolist())
        # the class of output row 2 i + py reads dz row i + r - 1 with tap ky = py + k // 2 + 2 - 2 r
        for py in range(2):
            for r in range(3):
                ky = py + k // 2 + 2 - 2 * r
                want = w[:, :, ky, k // 2].t() if 0 <= ky < k else torch.zeros(3, 2)
                assert torch.equal(taps[2 * py + 0][:, :, r, 1], want), (k, py, r)


# ---- BatchNorm + LeakyReLU alone -------------------------------------------------------------------------------------------------------
def bn_case(shape, seed):
    c, n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, h, w, generator=g) * 2.0 + torch.randn(1, c, 1, 1, generator=g)
    return z, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g), torch.randn(n, c, h, w, generator=g)


def bn_oracle(shape, seed):
    z, gamma, beta, dy = bn_case(shape, seed)
    leaves = [t.double().requires_grad_(True) for t in (z, gamma, beta)]
    pre = []
    y, mean, var = R.bn_leaky(*leaves, pre)
    (y * dy.double()).sum().backward()
    return y.detach(), mean.detach(), var.detach(), [t.grad for t in leaves], pre[0]


def check_bn_leaky(device):
    worst = 0.0
    for shape, seed in BN_CASES.items():
        z, gamma, beta, dy = bn_case(shape, seed)
        y64, mean, var, (dz64, dg64, db64), u64 = bn_oracle(shape, seed)
        assert_clear_of_the_kink(u64, ("bn", shape, seed))
        c = shape[0]
        rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
        zd, gd, bd = z.to(device), gamma.to(device), beta.to(device)
        y, stats = ops.fpn_bn_leaky_fwd(zd, gd, bd, R.BN_EPS, rm, rv, R.MOMENTUM)
        assert torch.equal(torch.signbit(y.cpu()), torch.signbit(y64)), shape
        T.within_range(y.cpu(), y64, BAR, ("bn y", shape))
        T.close(stats[0].cpu(), mean, T.LAYER_BAR, ("bn mean", shape))
        T.close(stats[1].cpu(), var, T.LAYER_BAR, ("bn var", shape))
        m = z.numel() // c
        T.close(rm.cpu(), R.MOMENTUM * mean, T.LAYER_BAR, ("bn running_mean", shape))
        T.close(rv.cpu(), (1 - R.MOMENTUM) + R.MOMENTUM * var * (m / (m - 1)), T.LAYER_BAR, ("bn running_var", shape))
        dz, dg, db = ops.fpn_bn_leaky_bwd(dy.to(device), zd, stats, gd, bd)
        worst = max(worst, rel(dz, dz64, ("bn dz", shape)), rel(dg, dg64, ("bn dgamma", shape)), rel(db, db64, ("bn dbeta", shape)))
    return worst


def test_bn_leaky_against_fp64(emu):
    print("mvs_fpn_bn_leaky_fwd / _bwd vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_bn_leaky(emu), BAR))


# ---- one block node per distinct layer -------------------------------------------------------------------------------------------------
BLOCK_OUT = (2, 3, 5)                        # N, OH, OW


def block_case(layer, seed):
    cout, cin, k, s = layer
    n, oh, ow = BLOCK_OUT
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, oh * s, ow * s, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    return x, w, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), torch.randn(n, cout, oh, ow, generator=g)


def block_oracle(layer, seed):
    x, w, gamma, beta, cot = block_case(layer, seed)
    leaves = [t.double().requires_grad_(True) for t in (x, w, gamma, beta)]
    sd = {"b.conv.weight": leaves[1], "b.bn.weight": leaves[2], "b.bn.bias": leaves[3], "b.bn.running_mean": torch.zeros(layer[0]).double(),
          "b.bn.running_var": torch.ones(layer[0]).double(), "b.bn.num_batches_tracked": torch.tensor(0)}
    pre, running = {}, {}
    y = R.block(leaves[0], sd, "b", layer[2], layer[3], running, pre)
    (y * cot.double()).sum().backward()
    return y.detach(), [t.grad for t in leaves], running, pre["b"]


def check_blocks(device):
    worst = 0.0
    for layer, seed in BLOCK_SEEDS.items():
        cout, cin, k, s = layer
        y64, g64, running, u64 = block_oracle(layer, seed)
        assert_clear_of_the_kink(u64, ("block", layer, seed))
        x, w, gamma, beta, cot = block_case(layer, seed)
        bn = torch.nn.BatchNorm2d(cout).to(device).train()
        got = [t.clone().to(device).requires_grad_(i > 0 or cin != 3) for i, t in enumerate((x, w, gamma, beta))]   # conv00: no image gradient
        y = training.FpnEncBlockTrain.apply(got[0], bn, got[1], got[2], got[3], s)
        (y * cot.to(device)).sum().backward()
        assert torch.equal(torch.signbit(y.detach().cpu()), torch.signbit(y64)), layer
        T.within_range(y.detach().cpu(), y64, BAR, ("block", layer))
        T.close(bn.running_mean.cpu(), running["b.bn.running_mean"], T.LAYER_BAR, ("block running_mean", layer))
        T.close(bn.running_var.cpu(), running["b.bn.running_var"], T.LAYER_BAR, ("block running_var", layer))
        assert int(bn.num_batches_tracked) == 1
        for nm, a, r in zip(("x", "w", "gamma", "beta"), got, g64):
            if a.requires_grad:
                worst = max(worst, rel(a.grad, r, ("block", layer, nm)))
        assert got[0].requires_grad or got[0].grad is None
    return worst


def test_block_nodes_against_fp64(emu):
    print("FpnEncBlockTrain vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (check_blocks(emu), BAR))


# ---- whole module ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights():
    return T.f25_weights(T.f25(), "enc.")


def image(seed=None):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(IN_SEED if seed is None else seed))


def cotangents(outs, seed=COT_SEED):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) for o in outs]


def sd64_of(sd, params):
    return {k: (v.double().requires_grad_(True) if k in params else v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def oracle():
    """fp64 autograd through tests/fpn_encoder_train_ref.py -> (outputs, {parameter key: gradient}, updated running statistics, every
    block's pre-activation u64); computed once and shared (read-only)."""
    sd64 = sd64_of(weights(), R.PARAMS)
    running, pre = {}, {}
    outs = R.encoder(image(), sd64, running=running, pre=pre)
    sum((o * c.double()).sum() for o, c in zip(outs, cotangents(outs))).backward()
    return [o.detach() for o in outs], {k: sd64[k].grad for k in R.PARAMS}, running, pre


def trainable(device="cpu", train=True):
    m = TrainableFPNEncoder([8, 16, 32, 64])
    m.load_state_dict(weights(), strict=True)
    return m.train(train).to(device)


def native_step(m, x):
    m.zero_grad(set_to_none=True)
    outs = m(x)
    sum((o * c.to(o.device)).sum() for o, c in zip(outs, cotangents(outs))).backward()
    return outs, {k: p.grad for k, p in m.named_parameters()}


def measure_u_error(device):
    """E = max |u_native - u64| over the 11 blocks of the module case: u_native = gamma xhat + beta in fp32 from the pre-activation z and
    the statistics of the same ops calls the forward makes (DELTA = 4 E on the emulator, see the module docstring)."""
    from mvsformerplusplus_amd import packing
    sd, pre = weights(), oracle()[3]
    t, worst = image().to(device), 0.0
    for name, k, s in FPNEncoder.LAYERS:
        w, g, b = (sd[name + sfx].to(device) for sfx in (".conv.weight", ".bn.weight", ".bn.bias"))
        z = ops.fpn_conv(t, packing.pack_fpn_conv_weights(w, s).to(device), None, w.shape[0], k, s, ops.FPN_ACT_NONE)
        t, stats = ops.fpn_bn_leaky_fwd(z, g, b, R.BN_EPS)
        u = (z - stats[0].reshape(1, -1, 1, 1)) * stats[2].reshape(1, -1, 1, 1) * g.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1)
        worst = max(worst, float((u.double().cpu() - pre[name]).abs().max()))
        print("  %-12s max |u_native - u64| = %.3g" % (name, float((u.double().cpu() - pre[name]).abs().max())))
    return worst


def check_running(m, want, what):
    worst = 0.0
    buffers = dict(m.named_buffers())
    assert set(buffers) == set(want) and len(want) == 33
    for k, w in want.items():
        if k.endswith("num_batches_tracked"):
            assert int(buffers[k]) == int(w), (what, k)
        else:
            worst = max(worst, T.close(buffers[k].detach().cpu(), w, T.LAYER_BAR, (what, k)))
    return worst


def check_module(device):
    """One training step on `device` against the fp64 oracle -> (worst gradient ratio, worst output fraction, worst running-stat error)."""
    want_out, want, want_run, pre = oracle()
    assert_clear_of_the_kink(pre, "module case")
    assert len(pre) == 11 and len(want) == 33
    m = trainable(device)
    x = image().to(device)
    outs, grads = native_step(m, x)
    frac = 0.0
    for k, o in enumerate(outs):
        assert o.dtype == torch.float32 and o.is_contiguous() and o.requires_grad
        assert torch.equal(torch.signbit(o.detach().cpu()), torch.signbit(want_out[k])), R.OUTPUTS[k]
        frac = max(frac, T.within_range(o.detach().cpu(), want_out[k], BAR, R.OUTPUTS[k]))
    run = check_running(m, want_run, "module case")
    before = {k: v.clone() for k, v in m.named_buffers()}
    m(x)                                                                      # a second step moves the statistics again
    for k, v in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1
        else:
            assert not torch.equal(v, before[k]), k
    assert set(grads) == set(want)
    return max(rel(grads[k], want[k], ("module", k)) for k in want), frac, run


def test_module_backward_against_fp64(emu):
    worst, frac, run = check_module(emu)
    print("fpn_encoder_forward_train vs fp64: worst gradient |error| = %.3g x max|g64| over 33 tensors (bar %g); outputs %.3g of their range; "
          "running statistics %.3g" % (worst, BAR, frac, run))


def test_u_error_stays_within_the_margin(emu):
    """The margin behind DELTA: a flip needs an error above |u64| >= DELTA; the native pre-activations must lie within DELTA / 2 of the
    oracle's, which leaves a factor of two (E itself is DELTA / 4 on the emulator)."""
    e = measure_u_error(emu)
    print("max |u_native - u64| over the 11 blocks: %.3g (DELTA %.3g)" % (e, DELTA))
    assert e <= DELTA / 2, (e, DELTA)


# ---- chain: image -> encoder -> decoder -> FMT_with_pathway ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_oracle():
    import fmt_ref
    import fpn_train_ref as DR
    import test_fmt_train as FT
    import test_fpn_train as DT
    _, fsd, cfg = FT.fixture()
    sd64 = sd64_of(weights(), R.PARAMS)
    pre = {}
    feats = R.encoder(image(), sd64, pre=pre)
    outs = DR.decoder(*feats, {k: v.double() if v.is_floating_point() else v for k, v in DT.weights().items()})
    out = fmt_ref.fmt({"stage%d" % (k + 1): o.unsqueeze(0) for k, o in enumerate(outs)}, {k: v.double() for k, v in fsd.items()}, cfg["layer_names"])
    cot = FT.cotangents({s: out[s].shape for s in FT.STAGES})
    sum((out[s] * cot[s].double()).sum() for s in FT.STAGES).backward()
    return {k: sd64[k].grad for k in R.PARAMS}, pre


def check_chain(device):
    import test_fmt_train as FT
    import test_fpn_train as DT
    want, pre = chain_oracle()
    assert_clear_of_the_kink(pre, "chain")
    enc, dec, fmt = trainable(device), DT.trainable(device), FT.trainable(device)
    out = fmt({"stage%d" % (k + 1): o.unsqueeze(0) for k, o in enumerate(dec(*enc(image().to(device))))})
    cot = FT.cotangents({s: out[s].shape for s in FT.STAGES})
    sum((out[s] * cot[s].to(device)).sum() for s in FT.STAGES).backward()
    grads = {k: p.grad for k, p in enc.named_parameters()}
    assert set(grads) == set(want) and len(want) == 33
    return max(rel(grads[k], want[k], ("chain", k)) for k in want)


def test_chain_into_decoder_and_fmt_against_fp64(emu):
    print("image -> FPNEncoder -> FPNDecoder -> FMT_with_pathway vs fp64 (B = 1, V = 2): worst |error| = %.3g x max|g64| over the encoder's 33 "
          "parameters (bar %g)" % (check_chain(emu), BAR))


# ---- module contract -------------------------------------------------------------------------------------------------------------------
def test_eval_forward_is_the_inference_forward_bit_for_bit(emu):
    fx = T.f25()
    enc, _ = T.modules(fx)
    m = trainable(train=False)
    x = fx["b/x"]
    with torch.no_grad():
        want, got = enc(x), m(x)
    for a, b in zip(got, want):
        assert torch.equal(a, b) and not a.requires_grad
    with pytest.raises(RuntimeError, match="frozen"):
        m(x.clone().requires_grad_(True))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert sorted(before) == sorted(weights())
    for k, v in before.items():
        assert torch.equal(v, weights()[k]), k                      # strict load, eval forward leaves the buffers alone


def test_patch_fpn_flag_combinations():
    for enc_flag, dec_flag in ((False, False), (True, False), (False, True), (True, True)):
        for mode in (True, False):
            net = T._StandIn().train(mode)
            before = {k: v.clone() for k, v in net.state_dict().items()}
            enc, dec = net.encoder, net.decoder
            others = {n: getattr(net, n) for n in ("vit", "decoder_vit", "FMT_with_pathway", "fusions")}
            assert patch_fpn(net, trainable_decoder=dec_flag, trainable_encoder=enc_flag) is net
            if not enc_flag and not dec_flag:
                assert type(net.encoder) is FPNEncoder and type(net.decoder).__name__ == "FPNDecoder"
            else:
                assert (type(net.encoder) is TrainableFPNEncoder) if enc_flag else (net.encoder is enc)
                assert (type(net.decoder) is TrainableFPNDecoder) if dec_flag else (net.decoder is dec)
            assert net.encoder.training is mode and net.decoder.training is mode
            for n, mod in others.items():
                assert getattr(net, n) is mod
            after = net.state_dict()
            assert sorted(after) == sorted(before)
            for k, v in before.items():
                assert torch.equal(after[k], v), k
    import mvsformerplusplus_amd as pkg
    assert pkg.TrainableFPNEncoder is TrainableFPNEncoder and pkg.fpn_encoder_forward_train is training.fpn_encoder_forward_train


def test_input_dtypes(emu):
    """A bf16 / fp16 image is widened once: exactly what its fp32 widening gives - outputs and gradients for bf16, outputs for fp16."""
    x = image().to(torch.bfloat16)
    outs_n, g_n = native_step(trainable(), x)
    outs_w, g_w = native_step(trainable(), x.float())
    for a, b in zip(outs_n, outs_w):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    for k in g_w:
        assert g_n[k].dtype == torch.float32 and torch.equal(g_n[k], g_w[k]), k
    x = image().to(torch.float16)
    for a, b in zip(trainable()(x), trainable()(x.float())):
        assert a.dtype == torch.float32 and torch.equal(a, b)


def test_refusals(emu, monkeypatch):
    m = trainable()
    with pytest.raises(NotImplementedError, match="image's gradient"):
        m(image().requires_grad_(True))
    with pytest.raises(ValueError, match="multiples of 8"):
        m(torch.zeros(1, 3, 20, 16))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        m(torch.zeros(1, 4, 16, 16))
    outs = m(image())
    v = torch.ones_like(outs[1]).requires_grad_(True)                        # a cotangent that itself asks for a gradient
    (g,) = torch.autograd.grad(outs[1], m.conv11.conv.weight, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="SyncBatchNorm"):
        m(image())


def test_entry_point_refusals(emu):
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_enc_wgrad(torch.zeros(1, 24, 4, 4), torch.zeros(1, 24, 4, 4), 3)
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_enc_wgrad(torch.zeros(1, 16, 2, 2), torch.zeros(1, 8, 4, 4), 3, 2)          # downsample1 has k = 5
    with pytest.raises(ValueError, match="does not belong"):
        ops.fpn_enc_wgrad(torch.zeros(1, 16, 4, 4), torch.zeros(1, 8, 4, 4), 5, 2)
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_enc_dgrad(torch.zeros(1, 8, 4, 4), torch.zeros(8, 3, 7, 7))                 # conv00's is never computed
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_enc_dgrad(torch.zeros(1, 24, 4, 4), torch.zeros(24, 24, 3, 3), 2)
    with pytest.raises(_lib.MvsHipError, match="not built"):
        ops.fpn_bn_leaky_fwd(torch.zeros(1, 65, 2, 2), torch.ones(65), torch.zeros(65), 1e-5)
    L = _lib.lib()
    with pytest.raises(_lib.MvsHipError, match="even"):
        L.mvs_fpn_enc_dgrad(1, 1, 1, 1, 8, 16, 5, 3, 4, None)
    with pytest.raises(_lib.MvsHipError, match="built for"):
        L.mvs_fpn_enc_dgrad(1, 1, 1, 1, 8, 16, 3, 4, 4, None)
    for cout, cin, k, s in LAYERS[1:]:
        assert ops.fpn_enc_dgrad_is_built(cin, cout, k, s)
    assert not ops.fpn_enc_dgrad_is_built(3, 8, 7, 1) and not ops.fpn_enc_dgrad_is_built(8, 16, 5, 1) and not ops.fpn_enc_dgrad_is_built(8, 16, 3, 2)
    assert L.mvs_fpn_enc_wgrad_workspace_bytes(1, 32, 64, 3, 2, 4, 128) == 64 * 288 * 4     # one partial per 2 x 64 tile of dz
    assert L.mvs_fpn_enc_wgrad_workspace_bytes(1, 3, 8, 7, 1, 8, 128) == 4 * 8 * 147 * 4
    assert L.mvs_fpn_enc_wgrad_workspace_bytes(1, 3, 8, 7, 2, 8, 128) == 0 and L.mvs_fpn_enc_dgrad_weights_bytes(8, 16, 3) == 0


def test_host_tensors_are_refused(monkeypatch, emu_lib):
    """No CPU route in training either: with the device requirement in force a host tensor raises before any launch."""
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    assert _lib._REQUIRE_DEVICE
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        trainable()(image())
    with pytest.raises(_lib.MvsHipError, match="ROCm device"):
        ops.fpn_enc_wgrad(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), 5)


def test_gradients_are_the_same_bits_over_two_runs(emu):
    a, b = native_step(trainable(), image())[1], native_step(trainable(), image())[1]
    assert len(a) == 33
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- fixture F34: the oracle's gradients are the reference's own ----------------------------------------------------------------------
def test_restatement_pinned_to_f34():
    """tests/fpn_encoder_train_ref.py's fp64 outputs, gradients and running statistics against the reference's own FPNEncoder in train mode
    (fp32, CPU; fixture F34), at test_fpn_train.test_restatement_pinned_to_f33's bars: gradients 2e-4 x max|g| per tensor, running statistics
    test_fpn.LAYER_BAR, num_batches_tracked exact; the outputs within 2e-4 of their range.  F34's input is the module case's, so the
    reference's own fp32 run is clear of the kink by the same condition."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "f34_fpn_encoder_train_*.npz")))
    f34 = {}
    for path in files:
        assert os.path.getsize(path) < 1024 * 1024
        f34.update({k: v for k, v in load_golden(os.path.basename(path)).items() if k != "__name__"})
    assert int(f34["in.seed"]) == IN_SEED and int(f34["cot.seed"]) == COT_SEED and tuple(int(v) for v in f34["in.shape"]) == SHAPE
    assert hashlib.sha256(image().contiguous().numpy().tobytes()).hexdigest() == f34["in.sha256"], \
        "torch's CPU generator changed: regenerate F34 (tests/golden/make_golden_fpn_encoder_train.py)"
    outs, grads, running, pre = oracle()
    assert_clear_of_the_kink(pre, "F34")
    for n, o in zip(R.OUTPUTS, outs):
        T.within_range(f34["out/" + n], o, 2e-4, n)
    ref = {k[len("g/"):]: v for k, v in f34.items() if k.startswith("g/")}
    assert len(ref) == 33 and sorted(ref) == sorted(grads)
    worst = 0.0
    for k, w in ref.items():
        r = float((grads[k] - w.double()).abs().max()) / float(w.abs().max())
        assert r <= 2e-4, (k, r)
        worst = max(worst, r)
    run = {k[len("run/"):]: v for k, v in f34.items() if k.startswith("run/")}
    assert len(run) == 33 and set(run) == set(running)
    for k, w in run.items():
        if k.endswith("num_batches_tracked"):
            assert int(w) == int(running[k])
        else:
            T.close(running[k], w, T.LAYER_BAR, k)
    print("fpn_encoder_train_ref fp64 gradients vs the reference's fp32 autograd (F34): worst %.3g x max|g|" % worst)
