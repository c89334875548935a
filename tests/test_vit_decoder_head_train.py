"""CPU: the native train-mode head of the CrossVITDecoder (TrainableCrossVITDecoder(args, native_head=True), training.vitdec_head_train,
csrc/vitdec_head_train_kernels.hip) on the host emulator against fp64 on the host: F.conv2d / F.conv_transpose2d
with autograd for the entry points and the nodes, tests/vit_decoder_train_ref.py (pinned to fixture F35) for the module.

Bars (the project's, tests/test_vit_decoder_train.py; nothing derived from the code under test):
  * LAYER_BAR = 3e-5 x max(1, max|ref|) for one entry point and for the running statistics;
  * BAR = 2e-4 x max|g64| for every gradient of a node or of the module, 2e-4 of the oracle's range for the train-mode output;
  * the three conv biases in front of a batch-statistics BatchNorm: torch.equal(grad, zeros);
  * two calls, two runs of the head: torch.equal.
Shapes (NV, h, w): (1, 1, 1) - every window position but one off the map (convolutions only: a BatchNorm over one value is refused);
(2, 1, 3) - one-row maps, rows and views abut inside one 16-token block; (3, 4, 6), (4, 3, 5) - F27's cases a and b (72 and 60 tokens);
and the smallest map at which proj's weight gradient is cut into at least three slabs with a ragged last one (slab_shape()).

Measured on the emulator: the figures each test prints (pytest -s); on an MI355X: tests/test_vit_decoder_head_train_gpu.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import test_vit_decoder as T
import test_vit_decoder_train as C
import vit_decoder_train_ref as RT
from mvsformerplusplus_amd import ops, packing, training
from mvsformerplusplus_amd.vit_decoder import TrainableCrossVITDecoder, patch_vit_decoder

BAR = C.BAR
LAYER_BAR = C.LAYER_BAR
HEAD = packing.VITDEC_HEAD
CH = ((768, 256), (256, 128), (128, 64))                         # (Cin, Cout) of proj, upsampler0, upsampler1
EPS, MOMENTUM = 1e-5, 0.1


def slab_shape():
    """The smallest (NV, h, w), by token count, at which proj's weight gradient runs in at least three slabs with a ragged last one
    (slabs are whole 32-token chunks; the count is read off the workspace query), as test_vit_decoder_train.multi_slab_m()."""
    for m in range(1, 1024):
        if m % 32:
            for h in range(1, 9):
                if m % h == 0 and ops.vitdec_head_wgrad_slabs(ops.VITDEC_PROJ, 1, h, m // h) >= 3:
                    return (1, h, m // h)
    raise AssertionError("no map below 1024 tokens gives three slabs")


def shapes():
    return ((1, 1, 1), (2, 1, 3), (3, 4, 6), (4, 3, 5), slab_shape())


def tok(t):
    """planar [N, C, H, W] -> token-major [N H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def packed(rows, device):
    """token-major fp32 rows -> the packed-split tensor (host packer)"""
    return packing.pack_tokens_split(rows).view(torch.uint8).to(device)


def conv64(layer, x, w, b=None):
    return F.conv2d(x, w, b, padding=1) if layer == 0 else F.conv_transpose2d(x, w, b, stride=2, padding=1)


# ---- entry points ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_case(layer, NV, h, w):
    """Random planar x and weight of a head layer on the [NV, h, w] input map, a cotangent, and fp64 z, d_x, d_w; computed once, shared."""
    cin, cout = CH[layer]
    g = torch.Generator().manual_seed(1000 * layer + 100 * NV + 10 * h + w)
    x = torch.randn(NV, cin, h, w, generator=g)
    wshape = (cout, cin, 3, 3) if layer == 0 else (cin, cout, 4, 4)
    wgt = torch.randn(wshape, generator=g) / (9 * cin if layer == 0 else 4 * cin) ** 0.5
    x64, w64 = x.double().requires_grad_(True), wgt.double().requires_grad_(True)
    z64 = conv64(layer, x64, w64)
    dz = torch.randn(z64.shape, generator=g)
    (z64 * dz.double()).sum().backward()
    return x, wgt, dz, z64.detach(), x64.grad, w64.grad


def check_convs(device):
    """The three pre-activation convolutions, their data gradients and their weight gradients on every shape -> worst error of each."""
    worst = [0.0, 0.0, 0.0]
    for NV, h, w in shapes():
        for layer, name in enumerate(HEAD):
            x, wgt, dz, z64, dx64, dw64 = conv_case(layer, NV, h, w)
            what = (name, NV, h, w)
            pk = packing.pack_vitdec_head_train({name + ".0.weight": wgt.to(device)})[name]
            xp, dzp = packed(tok(x), device), packed(tok(dz), device)
            z = ops.vitdec_head_conv(xp, pk["w"], layer, NV, h, w)
            worst[0] = max(worst[0], C.close(z, tok(z64), ("z",) + what))
            assert torch.equal(z, ops.vitdec_head_conv(xp, pk["w"], layer, NV, h, w)), ("two calls differ: z",) + what
            dx = ops.vitdec_head_dgrad(dzp, pk["wT"], layer, NV, h, w)
            worst[1] = max(worst[1], C.close(dx, tok(dx64), ("d_x",) + what))
            assert torch.equal(dx, ops.vitdec_head_dgrad(dzp, pk["wT"], layer, NV, h, w)), ("two calls differ: d_x",) + what
            dzt, xt = tok(dz).to(device), tok(x).to(device)
            dw = ops.vitdec_head_wgrad(dzt, xt, layer, NV, h, w)
            worst[2] = max(worst[2], C.close(dw, dw64, ("d_w",) + what))
            assert torch.equal(dw, ops.vitdec_head_wgrad(dzt, xt, layer, NV, h, w)), ("two calls differ: d_w",) + what
    return worst


@functools.lru_cache(maxsize=None)
def bn_case(Cc, NV, h, w):
    """Random token-major z [NV h w, C], BatchNorm parameters and buffers, a cotangent; fp64: y, stats, running tensors, d_z, d_gamma, d_beta."""
    M = NV * h * w
    g = torch.Generator().manual_seed(Cc + 7 * M)
    z, dy = torch.randn(M, Cc, generator=g) * 2 + 0.5, torch.randn(M, Cc, generator=g)
    gamma, beta, bias = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    z64, g64, b64 = z.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean = z64.mean(0)
    var = ((z64 - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    y64 = F.silu((z64 - mean) * invstd * g64 + b64)
    (y64 * dy.double()).sum().backward()
    run_m = (1 - MOMENTUM) * rm.double() + MOMENTUM * (mean.detach() + bias.double())
    run_v = (1 - MOMENTUM) * rv.double() + MOMENTUM * var.detach() * (M / max(M - 1, 1))
    stats = torch.stack([mean.detach(), var.detach(), invstd.detach()])
    return z, dy, gamma, beta, bias, rm, rv, y64.detach(), stats, run_m, run_v, z64.grad, g64.grad, b64.grad


def check_bn(device):
    """BatchNorm + SiLU forward and backward at C = 256 / 128 / 64 in both output forms -> (worst forward, worst backward error)."""
    fwd = bwd = 0.0
    for NV, h, w in shapes()[1:]:
        for Cc in (256, 128, 64):
            z, dy, gamma, beta, bias, rm, rv, y64, st64, rm64, rv64, dz64, dg64, db64 = bn_case(Cc, NV, h, w)
            what = (Cc, NV, h, w)
            M = NV * h * w
            d = lambda t: t.to(device)

            def forward(**kw):
                r, v = d(rm.clone()), d(rv.clone())
                return ops.vitdec_head_bn_fwd(d(z), d(gamma), d(beta), EPS, d(bias), r, v, MOMENTUM, **kw) + (r, v)

            y, yp, stats, r, v = forward(want_packed=True)
            fwd = max(fwd, C.close(y, y64, ("y",) + what), C.close(stats, st64, ("stats",) + what),
                      C.close(r, rm64, ("running_mean",) + what), C.close(v, rv64, ("running_var",) + what))
            T.close(packing.unpack_tokens_split(yp.cpu(), M, Cc), y.cpu(), 2.0 ** -16, ("packed-split of the same rows",) + what)
            again = forward(want_packed=True)
            rows = lambda p, c=Cc, m=M: packing.unpack_tokens_split(p.cpu(), m, c)          # (the 16-row padding of a packed tensor is never written)
            assert torch.equal(rows(yp), rows(again[1])), ("two calls differ: packed",) + what
            assert all(torch.equal(p, q) for p, q in zip((y, stats, r, v), again[:1] + again[2:])), ("two calls differ",) + what
            ypl, none, stats_p, r_p, v_p = forward(planar=(NV, h, w))
            assert none is None and torch.equal(ypl, y.reshape(NV, h, w, Cc).permute(0, 3, 1, 2)), ("planar is not the token-major permuted",) + what
            assert torch.equal(stats_p, stats) and torch.equal(r_p, r) and torch.equal(v_p, v), what
            for form in ("rows", "planar"):
                cot = d(dy) if form == "rows" else d(dy).reshape(NV, h, w, Cc).permute(0, 3, 1, 2).contiguous()
                dz, dzp, dg, db = ops.vitdec_head_bn_bwd(cot, d(z), stats, d(gamma), d(beta))
                bwd = max(bwd, C.rel(dz, dz64, ("d_z", form) + what), C.rel(dg, dg64, ("d_gamma", form) + what), C.rel(db, db64, ("d_beta", form) + what))
                T.close(packing.unpack_tokens_split(dzp.cpu(), M, Cc), dz.cpu(), 2.0 ** -16, ("packed-split d_z", form) + what)
                again = ops.vitdec_head_bn_bwd(cot, d(z), stats, d(gamma), d(beta))
                assert torch.equal(rows(dzp), rows(again[1])), ("two calls differ: packed", form) + what
                assert all(torch.equal(p, q) for p, q in zip((dz, dg, db), again[:1] + again[2:])), ("two calls differ", form) + what
    return fwd, bwd


# ---- nodes -----------------------------------------------------------------------------------------------------------------------------
def trainable(device, mode=True, native_head=True, momentum=None):
    fx = T.f27()
    m = TrainableCrossVITDecoder(T.f27_args(fx), native_head=native_head)
    m.load_state_dict(T.f27_weights(fx), strict=True)
    if momentum is not None:
        for name in HEAD:
            getattr(m, name)[1].momentum = momentum
    return m.train(mode).to(device)


@functools.lru_cache(maxsize=None)
def node_case(layer):
    """F27 case a's captured input of a head layer (planar), a cotangent, fp64 autograd through conv + bias + train-mode BatchNorm + SiLU."""
    fx = T.f27()
    name = HEAD[layer]
    x = (fx["a/tokens"].reshape(3, 4, 6, 768).permute(0, 3, 1, 2), fx["a/proj"], fx["a/upsampler0"])[layer].contiguous()
    sd = T.f27_weights(fx)
    p64 = {k: sd["%s.%s" % (name, k)].double().requires_grad_(True) for k in ("0.weight", "0.bias", "1.weight", "1.bias")}
    x64 = x.double().requires_grad_(True)
    y64 = F.silu(F.batch_norm(conv64(layer, x64, p64["0.weight"], p64["0.bias"]), None, None, p64["1.weight"], p64["1.bias"], True, 0.0, EPS))
    cot = torch.randn(y64.shape, generator=torch.Generator().manual_seed(40 + layer))
    (y64 * cot.double()).sum().backward()
    return x, cot, y64.detach(), x64.grad, {k: v.grad for k, v in p64.items()}


def check_nodes(device):
    """Each head-layer node on F27 case a's captured layer input -> worst gradient error x max|g64|; forward at LAYER_BAR."""
    worst = 0.0
    m = trainable(device)
    for layer, name in enumerate(HEAD):
        x, cot, y64, dx64, g64 = node_case(layer)
        NV, _, H, W = x.shape
        seq = getattr(m, name)
        xg = tok(x).to(device).requires_grad_(True)
        last = layer == 2
        y, yp = training.VitdecHeadLayerTrain.apply(xg, None if layer == 0 else packed(tok(x), device), seq[1], layer, NV, H, W, last,
                                                    seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias)
        if last:
            assert yp is None and y.shape == y64.shape
            C.close(y, y64, (name, "forward"))
            (y * cot.to(device)).sum().backward()
        else:
            C.close(y, tok(y64), (name, "forward"))
            T.close(packing.unpack_tokens_split(yp.cpu(), y.shape[0], y.shape[1]), y.detach().cpu(), 2.0 ** -16, (name, "packed output"))
            (y * tok(cot).to(device)).sum().backward()
        worst = max(worst, C.rel(xg.grad, tok(dx64), (name, "d_x")), C.rel(seq[0].weight.grad, g64["0.weight"], (name, "d_w")),
                    C.rel(seq[1].weight.grad, g64["1.weight"], (name, "d_gamma")), C.rel(seq[1].bias.grad, g64["1.bias"], (name, "d_beta")))
        assert torch.equal(seq[0].bias.grad, torch.zeros_like(seq[0].bias)), (name, "the conv bias's gradient is exactly zero")
        assert float(g64["0.bias"].abs().max()) <= 1e-9 * float(g64["0.weight"].abs().max()), (name, "fp64 agrees that it is zero")
    return worst


# ---- whole module ----------------------------------------------------------------------------------------------------------------------
def check_module(device, cases=("a", "b")):
    """test_vit_decoder_train.check_module with native_head=True and the zero-bias rule -> per case (worst gradient error x max|g64|,
    output error as a fraction of the oracle's range, running statistics error)."""
    res = {}
    for case in cases:
        out64, run64, g64 = C.oracle(case)
        m = trainable(device)
        out, grads = C.native_step(m, case, device)
        assert out.dtype == torch.float32 and out.is_contiguous() and len(grads) == 93 and sorted(grads) == sorted(g64)
        frac = T.within_range(out.cpu(), out64, BAR, case)
        worst = 0.0
        for k, g in g64.items():
            if k in C.ZERO_BIASES:
                assert torch.equal(grads[k], torch.zeros_like(grads[k])), (case, k)
            else:
                worst = max(worst, C.rel(grads[k], g, (case, k)))
        runerr, seen = 0.0, 0
        for k, b in m.named_buffers():
            seen += 1
            if k.endswith("num_batches_tracked"):
                assert int(b) == int(run64[k]) == 1, k
            else:
                runerr = max(runerr, C.close(b, run64[k], (case, k)))
        assert seen == len(run64) == 9
        res[case] = (worst, frac, runerr)
    return res


def head_alone(device, NV, h, w, seed=5):
    """The three nodes on fixed tokens and a fixed cotangent, on a fresh module -> output, token gradient, 9 parameter gradients, 6 running
    tensors (19 tensors)."""
    m = trainable(device)
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randn(NV * h * w, 768, generator=g).to(device).requires_grad_(True)
    cot = torch.randn(NV, 64, 4 * h, 4 * w, generator=g).to(device)
    out = training.vitdec_head_train(m, tokens, NV, h, w)
    (out * cot).sum().backward()
    res = [out.detach(), tokens.grad]
    for name in HEAD:
        seq = getattr(m, name)
        res += [seq[0].weight.grad, seq[0].bias.grad, seq[1].weight.grad, seq[1].bias.grad, seq[1].running_mean, seq[1].running_var]
    assert len(res) == 2 + 3 * 6 and all(t is not None for t in res)
    return res


def check_head_bit_identity(device, NV, h, w):
    a, b = head_alone(device, NV, h, w), head_alone(device, NV, h, w)
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), ("two runs of the head differ", i, NV, h, w)
    return a


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def test_slab_shape(emu):
    """65 tokens: three 32-token chunks, the last one ragged, one slab each (54 x 2 tiles want five slabs and get the three there are)."""
    NV, h, w = slab_shape()
    assert NV * h * w == 65 and [ops.vitdec_head_wgrad_slabs(ops.VITDEC_PROJ, 1, 1, m) for m in (1, 32, 33, 64, 65)] == [1, 1, 2, 2, 3]
    assert ops.vitdec_head_wgrad_slabs(ops.VITDEC_UP0, 4, 16, 20) > 1 and ops.vitdec_head_wgrad_slabs(ops.VITDEC_UP1, 4, 32, 40) > 1
    assert ops.vitdec_head_wgrad_slabs(3, 1, 4, 4) == 0                 # no such layer


def test_window_gemms_against_fp64(emu):
    z, dx, dw = check_convs(emu)
    print("head convolutions vs fp64 on %s: pre-activation %.3g, data gradient %.3g, weight gradient %.3g x max(1, max|ref|) (bar %g)"
          % (shapes(), z, dx, dw, LAYER_BAR))


def test_token_batchnorm_against_fp64(emu):
    fwd, bwd = check_bn(emu)
    print("token-major BatchNorm + SiLU vs fp64: forward %.3g x max(1, max|ref|) (bar %g), backward %.3g x max|g64| (bar %g)" % (fwd, LAYER_BAR, bwd, BAR))


def test_device_packing_is_the_host_packing():
    """pack_vitdec_head_train's forward operands are the bits of pack_vitdec_conv / pack_vitdec_deconv for an identity BatchNorm; the data
    gradients' operands are pack_linear_bf16x3 of the flipped / window matrices."""
    sd = T.f27_weights(T.f27())
    live = packing.pack_vitdec_head_train({k: v for k, v in sd.items() if k.endswith(".0.weight")})
    ident = lambda c: {"weight": torch.ones(c), "bias": torch.zeros(c), "running_mean": torch.zeros(c), "running_var": torch.ones(c), "eps": 0.0}
    assert sorted(live) == sorted(HEAD)
    w = sd["proj.0.weight"]
    assert torch.equal(live["proj"]["w"], packing.pack_vitdec_conv(w, sd["proj.0.bias"], ident(256))[0])
    assert torch.equal(live["proj"]["wT"], packing.pack_linear_bf16x3(w.flip(2, 3).permute(1, 2, 3, 0).reshape(768, 2304).contiguous()))
    for name, (cin, cout) in zip(HEAD[1:], CH[1:]):
        w = sd[name + ".0.weight"]
        assert torch.equal(live[name]["w"], packing.pack_vitdec_deconv(w, sd[name + ".0.bias"], ident(cout))[0])
        m = torch.zeros(cin, 16 * cout)
        for ky in range(4):
            for kx in range(4):
                m[:, (4 * ky + kx) * cout:(4 * ky + kx + 1) * cout] = w[:, :, ky, kx]
        assert torch.equal(live[name]["wT"], packing.pack_linear_bf16x3(m))
    assert "wT" not in packing.pack_vitdec_head_train({"proj.0.weight": sd["proj.0.weight"]}, transposed=False)["proj"]


def test_head_nodes_against_fp64(emu):
    print("VitdecHeadLayerTrain (proj, upsampler0, upsampler1 on F27 case a's layer inputs) vs fp64 autograd: worst gradient |error| = %.3g x "
          "max|g64| (bar %g); conv bias gradients exactly zero" % (check_nodes(emu), BAR))


@pytest.mark.parametrize("case", ["a", "b"])
def test_module_against_fp64(emu, case):
    """Measured: case a 4.8e-5 x max|g64| on the emulator and 4.6e-5 on the MI355X; case b 1.66e-4 and 6.0e-5, its worst tensor the
    scalar prev_values.0 (a sum of 46 080 cancelling terms; 2.45e-4 on the emulator before the window GEMM summed K in two levels,
    DESIGN.md section 4.21)."""
    worst, frac, run = check_module(emu, (case,))[case]
    print("vitdec_forward_train with the native head, case %s vs fp64: worst gradient |error| = %.3g x max|g64| over 93 tensors (bar %g); "
          "output %.3g of its range; running statistics %.3g" % (case, worst, BAR, frac, run))


def test_head_is_bit_identical(emu):
    check_head_bit_identity(emu, 3, 4, 6)


def test_second_step_uses_the_updated_weights(emu):
    """The packing-cache trap, on the head: an in-place update of proj.0.weight and upsampler1.1.weight is seen by the next step."""
    m = trainable(emu)
    x = [torch.randn(1, 2, 6, 768, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    shape = [1, 2, 2, 3, 768]
    first = m(x, vit_shape=shape).detach()
    with torch.no_grad():
        m.proj[0].weight.mul_(0.5)
        m.upsampler1[1].weight.add_(0.25)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    second = m(x, vit_shape=shape).detach()
    fresh = TrainableCrossVITDecoder(T.f27_args(T.f27()), native_head=True)
    fresh.load_state_dict(state, strict=True)
    assert not torch.equal(first, second) and torch.equal(second, fresh.train()(x, vit_shape=shape).detach())
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in m.state_dict().items())


def test_momentum_and_eps_are_the_layers_own(emu):
    """momentum = 0.3: the running tensors against the oracle's formula with the oracle's batch statistics (case b)."""
    fx = T.f27()
    sd = T.f27_weights(fx)
    _, run64, _ = C.oracle("b")
    m = trainable(emu, momentum=0.3)
    m(T.inputs(fx, "b"), vit_shape=T.SHAPE_B)
    for name in HEAD:
        for stat in ("running_mean", "running_var"):
            k = "%s.1.%s" % (name, stat)
            batch = (run64[k].double() - (1 - RT.MOMENTUM) * sd[k].double()) / RT.MOMENTUM          # what the oracle's step took in
            C.close(m.state_dict()[k], 0.7 * sd[k].double() + 0.3 * batch, k)
    m2 = trainable(emu)
    m2.proj[1].eps = 0.5
    out = m2(T.inputs(fx, "b"), vit_shape=T.SHAPE_B)
    assert not torch.equal(out, trainable(emu)(T.inputs(fx, "b"), vit_shape=T.SHAPE_B))


class _Net(torch.nn.Module):
    pass


def test_contract(emu):
    fx = T.f27()
    sd = T.f27_weights(fx)
    m = trainable(emu)
    assert m.native_head is True and TrainableCrossVITDecoder(T.f27_args(fx)).native_head is False
    assert len(m.state_dict()) == 102 and sorted(m.state_dict()) == sorted(sd) and len(list(m.parameters())) == 93 and len(list(m.buffers())) == 9
    net = _Net()
    net.decoder_vit = trainable("cpu", native_head=False)
    assert patch_vit_decoder(net, trainable=True, native_head=True).decoder_vit.native_head is True
    assert patch_vit_decoder(net, trainable=True).decoder_vit.native_head is False
    with pytest.raises(ValueError, match="trainable"):
        patch_vit_decoder(net, native_head=True)
    # eval(): the parent's inference forward, bit for bit
    with torch.no_grad():
        assert torch.equal(trainable(emu, False)(T.inputs(fx, "b"), vit_shape=T.SHAPE_B), T.module(fx)(T.inputs(fx, "b"), vit_shape=T.SHAPE_B))
    # the refusals of the PyTorch-head path hold
    x = [torch.zeros(1, 1, 2, 768) for _ in range(3)]
    with pytest.raises(NotImplementedError, match="frozen"):
        m([x[0], x[1].clone().requires_grad_(True), x[2]], vit_shape=[1, 1, 1, 2, 768])
    # a head BatchNorm in eval mode while the module trains; nothing has moved
    m.upsampler0[1].eval()
    with pytest.raises(NotImplementedError, match="eval mode"):
        m(x, vit_shape=[1, 1, 1, 2, 768])
    assert int(m.proj[1].num_batches_tracked) == 0
    m.upsampler0[1].train()
    # one value per channel at proj, as PyTorch
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m([t[:, :, :1] for t in x], vit_shape=[1, 1, 1, 1, 768])
    assert int(m.proj[1].num_batches_tracked) == 0
    # V = 1 leaves the cross blocks without gradient; the output is planar fp32
    out = m([torch.randn(2, 1, 2, 768, generator=torch.Generator().manual_seed(i)) for i in range(3)], vit_shape=[2, 1, 1, 2, 768])
    assert out.shape == (2, 64, 4, 8) and out.dtype == torch.float32 and out.is_contiguous()
    out.square().sum().backward()
    for k, p in m.named_parameters():
        assert (p.grad is None) == k.startswith("cross_attn_blocks."), k


def test_default_is_the_pytorch_head(emu):
    """native_head=False: the module's own proj is called (the parent's path); native_head=True: it is not."""
    x = [torch.randn(1, 1, 2, 768, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    for native in (False, True):
        m = trainable(emu, native_head=native)
        calls = []
        handle = m.proj.register_forward_hook(lambda *a: calls.append(1))
        m(x, vit_shape=[1, 1, 1, 2, 768])
        handle.remove()
        assert len(calls) == (0 if native else 1), native
