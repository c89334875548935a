"""CPU: training of the CrossVITDecoder (mvsformerplusplus_amd.training.vitdec_forward_train, vit_decoder.TrainableCrossVITDecoder,
csrc/vitdec_train_kernels.hip) on the host emulator against fp64 autograd through the restatement
tests/vit_decoder_train_ref.py, which is itself pinned to fixture F35 (the reference's own CrossVITDecoder in train mode,
tests/golden/make_golden_vit_decoder_train.py).

Bars (the project's, nothing derived from the code under test):
  * LAYER_BAR = 3e-5 x max(1, max|ref|) for one entry point (tests/test_vit_decoder.py): mvs_vitdec_wgrad against fp64 dy^T x, every
    data-gradient GEMM against fp64 dy W, the running statistics;
  * BAR = MODULE_BAR = 2e-4 x max|g64| for every gradient tensor of a node or of the module, and 2e-4 of the oracle's range for the
    train-mode output.  The oracle with every GEMM operand rounded to hi + lo bf16 sits at most 3.9e-5 x max|g64| from fp64 on both module
    cases (the error model of the FORMAT), so the bar leaves about five times the expected error.
  * mvs_vitdec_ln_bwd has no GEMM in it: fp32 row arithmetic, held to LAYER_BAR x max(1, max|ref|) as well.
  * The three conv biases in front of a batch-statistics BatchNorm have a true gradient of exactly zero (the fp64 oracle gives 1e-14):
    they are held to BAR x max|g64| of the same layer's WEIGHT gradient.
The oracle pin: every quantity F35 stores within MODULE_BAR x max|g| (sums: the bounds that an elementwise error of that size implies).
Measured, oracle fp64 vs F35 (the reference's own fp32 run): gradients 6.15e-6 x max|g| (case a) / 8.04e-6 (case b), outputs 3.32e-6 / 1.92e-6
of max|out|, running statistics 4.42e-7 / 5.31e-7 of their maximum.

Measured on the emulator: see the figures each test prints (pytest -s); on an MI355X: tests/test_vit_decoder_train_gpu.py."""
import functools
import glob
import hashlib
import os

import pytest
import torch
import torch.nn.functional as F

import test_vit_decoder as T
import vit_decoder_ref as R
import vit_decoder_train_ref as RT
from conftest import GOLDEN, load_golden
from mvsformerplusplus_amd import _lib, ops, packing, training
from mvsformerplusplus_amd.vit_decoder import CrossVITDecoder, TrainableCrossVITDecoder, patch_vit_decoder

BAR = T.MODULE_BAR
LAYER_BAR = T.LAYER_BAR
COT_SEED = 35
CASES = (("a", T.SHAPE_A), ("b", T.SHAPE_B))
WGRAD_SHAPES = ((768, 768), (1536, 768), (3072, 768), (768, 3072))            # (N, K) of dw [N, K]: q / proj, [k; v], fc1, fc2
ZERO_BIASES = ("proj.0.bias", "upsampler0.0.bias", "upsampler1.0.bias")


def multi_slab_m():
    """The smallest M at which the slab rule cuts the 768 x 768 weight gradient into at least three slabs with a ragged last one (the
    slabs are whole 32-token chunks; ops.vitdec_wgrad_slabs reads the count off the workspace query)."""
    for m in range(1, 4096):
        if ops.vitdec_wgrad_slabs(m, 768, 768) >= 3 and m % 32:
            return m
    raise AssertionError("no M below 4096 gives three slabs")


def token_counts():
    return (30, 1, multi_slab_m())          # not a multiple of 16 and smaller than one tile; one token; several slabs, the last ragged


def close(got, want, what, bar=LAYER_BAR):
    assert got is not None and tuple(got.shape) == tuple(want.shape), (what, None if got is None else tuple(got.shape), tuple(want.shape))
    r = float((got.detach().double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
    assert r <= bar, (what, r, bar)
    return r


def rel(got, want, what, bar=BAR, scale=None):
    assert got is not None and tuple(got.shape) == tuple(want.shape), (what, None if got is None else tuple(got.shape), tuple(want.shape))
    r = float((got.detach().double().cpu() - want).abs().max()) / (float(want.abs().max()) if scale is None else scale)
    assert r <= bar, (what, r, bar)
    return r


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gemm_case(N, K, M):
    """Random dy [M, N], x [M, K], W [N, K] and fp64 dy^T x, column sums of dy, dy W; computed once and shared (read-only)."""
    g = torch.Generator().manual_seed(N + K + M)
    dy, x, w = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    return dy, x, w, dy.double().t() @ x.double(), dy.double().sum(0), dy.double() @ w.double()


def gemm_cases():
    ms = token_counts()
    return [(N, K, ms[0]) for N, K in WGRAD_SHAPES] + [(768, 768, m) for m in ms[1:]]


def check_wgrad(device):
    worst = 0.0
    for N, K, M in gemm_cases():
        dy, x, _, dw64, db64, _ = gemm_case(N, K, M)
        dw, db = ops.vitdec_wgrad(dy.to(device), x.to(device), want_bias=True)
        worst = max(worst, close(dw, dw64, ("wgrad", N, K, M)), close(db, db64, ("dbias", N, K, M)))
        dw2, db2 = ops.vitdec_wgrad(dy.to(device), x.to(device), want_bias=True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), ("two calls differ", N, K, M)
        assert torch.equal(ops.vitdec_wgrad(dy.to(device), x.to(device)), dw), ("without the bias", N, K, M)
    return worst


def check_dgrad(device):
    """dX = dY W on mvs_vitdec_linear_fwd with the transposed weight: 768 -> 768, 1536 -> 768, 3072 -> 768 and 768 -> 3072."""
    worst = 0.0
    for N, K, M in gemm_cases():
        dy, _, w, _, _, dx64 = gemm_case(N, K, M)
        got = ops.vitdec_dgrad(dy.to(device), packing.pack_linear_bf16x3(w.to(device).t()), K)
        worst = max(worst, close(got, dx64, ("dgrad", N, K, M)))
    return worst


@functools.lru_cache(maxsize=None)
def ln_case(M, eps):
    g = torch.Generator().manual_seed(7 * M + (1 if eps < 5e-6 else 0))
    x, dy = torch.randn(M, 768, generator=g) * 3 + 1, torch.randn(M, 768, generator=g)
    w, add = torch.randn(768, generator=g), torch.randn(M, 768, generator=g)
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), torch.zeros(768, dtype=torch.float64, requires_grad=True)
    (F.layer_norm(x64, (768,), w64, b64, eps) * dy.double()).sum().backward()
    return x, dy, w, add, x64.grad, w64.grad, b64.grad


def check_ln_bwd(device):
    worst = 0.0
    for M in token_counts():
        for eps in (1e-5, 1e-6):
            x, dy, w, add, dx64, dw64, db64 = ln_case(M, eps)
            for extra in (None, add):
                a = None if extra is None else extra.to(device)
                dx, dw, db = ops.vitdec_ln_bwd(dy.to(device), x.to(device), w.to(device), eps, add=a)
                want = dx64 if extra is None else dx64 + extra.double()
                worst = max(worst, close(dx, want, ("ln d_x", M, eps)), close(dw, dw64, ("ln d_w", M, eps)), close(db, db64, ("ln d_b", M, eps)))
                again = ops.vitdec_ln_bwd(dy.to(device), x.to(device), w.to(device), eps, add=a)
                assert all(torch.equal(p, q) for p, q in zip((dx, dw, db), again)), ("two calls differ", M, eps)
    return worst


# ---- nodes -----------------------------------------------------------------------------------------------------------------------------
def trainable(device, mode=True):
    fx = T.f27()
    m = TrainableCrossVITDecoder(T.f27_args(fx))
    m.load_state_dict(T.f27_weights(fx), strict=True)
    return m.train(mode).to(device)


@functools.lru_cache(maxsize=None)
def block_case(kind, i):
    """F27's captured input of block (kind, i) (case a), a cotangent, and fp64 autograd through the oracle's block."""
    fx = T.f27()
    L = "%s_attn_blocks.%d." % (kind, i)
    x = fx["a/ref/blk%d_in" % i] if kind == "self" else fx["a/src/blk%d_in" % i]
    ref = None if kind == "self" else ([fx["a/x0"][:, 0]] + [fx["a/ref/feat%d" % k] for k in (1, 2)])[i]
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(3 + i))
    sd64 = {k: v.double().requires_grad_(True) for k, v in T.f27_weights(fx).items() if k.startswith(L)}
    x64, r64 = x.double().requires_grad_(True), None if ref is None else ref.double().requires_grad_(True)
    (R.block(R._Ops(sd64), L, x64, r64) * cot.double()).sum().backward()
    grads = {k: sd64[L + k].grad for k in training.VITDEC_BLOCK_PARAMS}
    return x, ref, cot, x64.grad, None if ref is None else r64.grad, grads


@functools.lru_cache(maxsize=None)
def grouped_case():
    """Cross block 2 on two reference views with two source views each (kv_div = 2, 5 tokens): source view i reads reference i // 2,
    and d_ref sums over the pair.  Random tokens; fp64 autograd through the oracle's block with the pair's tokens side by side."""
    L = "cross_attn_blocks.2."
    g = torch.Generator().manual_seed(21)
    x, ref, cot = torch.randn(4, 5, 768, generator=g), torch.randn(2, 5, 768, generator=g), torch.randn(4, 5, 768, generator=g)
    sd64 = {k: v.double().requires_grad_(True) for k, v in T.f27_weights(T.f27()).items() if k.startswith(L)}
    x64, r64 = x.double().requires_grad_(True), ref.double().requires_grad_(True)
    y64 = R.block(R._Ops(sd64), L, x64.reshape(2, 10, 768), r64).reshape(4, 5, 768)
    (y64 * cot.double()).sum().backward()
    return x, ref, cot, x64.grad, r64.grad, {k: sd64[L + k].grad for k in training.VITDEC_BLOCK_PARAMS}


def check_blocks(device):
    fx = T.f27()
    m = trainable(device)
    inference = T.module(fx, device)
    p = inference._params(torch.device(device))
    worst = 0.0
    for kind, i, kv_div in (("self", 0, 1), ("cross", 1, 1), ("cross", 2, 2)):
        x, ref, cot, dx64, dr64, g64 = block_case(kind, i) if kv_div == 1 else grouped_case()
        blk = getattr(m, kind + "_attn_blocks")[i]
        params = [blk.get_parameter(k) for k in training.VITDEC_BLOCK_PARAMS]
        xg = x.to(device).requires_grad_(True)
        rg = None if ref is None else ref.to(device).requires_grad_(True)
        y = training.VitdecBlockTrain.apply(xg, rg, kv_div, *params)
        assert torch.equal(y.detach().cpu(), T.run_block(inference, p, kind, i, x, ref, device)), ("forward is not the inference path's", kind, i)
        (y * cot.to(device)).sum().backward()
        worst = max(worst, rel(xg.grad, dx64, (kind, i, "d_x")))
        if ref is not None:
            worst = max(worst, rel(rg.grad, dr64, (kind, i, "d_ref")))
        for k, prm in zip(training.VITDEC_BLOCK_PARAMS, params):
            worst = max(worst, rel(prm.grad, g64[k], (kind, i, k)))
    return worst


def check_mix(device):
    """norm_layers[0](prev_values[0] * prev + x_1) on the reference view of case a, the level's feature read in place from [B, V, n, 768]."""
    fx = T.f27()
    sd = T.f27_weights(fx)
    m = trainable(device)
    prev, x1 = fx["a/ref/blk0_out"], fx["a/x1"]
    cot = torch.randn(prev.shape, generator=torch.Generator().manual_seed(11))
    p64 = prev.double().requires_grad_(True)
    pv64, w64, b64 = (sd[k].double().requires_grad_(True) for k in ("prev_values.0", "norm_layers.0.weight", "norm_layers.0.bias"))
    y64 = F.layer_norm(pv64 * p64 + x1[:, 0].double(), (768,), w64, b64, 1e-6)
    (y64 * cot.double()).sum().backward()
    pg = prev.to(device).requires_grad_(True)
    y = training.VitdecMixTrain.apply(pg, x1.to(device)[:, :1], m.prev_values[0], m.norm_layers[0].weight, m.norm_layers[0].bias)
    close(y, y64.detach(), "mix forward")
    (y * cot.to(device)).sum().backward()
    return max(rel(pg.grad, p64.grad, "d_prev"), rel(m.prev_values[0].grad, pv64.grad, "d_prev_value", scale=float(pv64.grad.abs())),
               rel(m.norm_layers[0].weight.grad, w64.grad, "d_mix_w"), rel(m.norm_layers[0].bias.grad, b64.grad, "d_mix_b"))


# ---- whole module ----------------------------------------------------------------------------------------------------------------------
def is_buffer(key):
    return "running_" in key or "num_batches_tracked" in key


@functools.lru_cache(maxsize=None)
def oracle(case, dtype=torch.float64, split_operands=False):
    """The fp64 (or fp32 / two-term) oracle's train step of a case: output, updated buffers, the 93 gradients; computed once and shared."""
    fx = T.f27()
    shape = dict(CASES)[case]
    sd = {k: (v.clone() if is_buffer(k) else v.to(dtype).requires_grad_(True)) for k, v in T.f27_weights(fx).items()}
    run = {}
    out = RT.vit_decoder_train(T.inputs(fx, case), sd, shape, dtype=dtype, running=run, split_operands=split_operands)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(COT_SEED))
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), run, {k: v.grad for k, v in sd.items() if not is_buffer(k)}


def native_step(m, case, device):
    fx = T.f27()
    m.zero_grad(set_to_none=True)
    out = m(T.inputs(fx, case, device), vit_shape=dict(CASES)[case])
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(COT_SEED))
    (out * cot.to(device)).sum().backward()
    return out.detach(), {k: p.grad for k, p in m.named_parameters()}


def check_module(device, cases=("a", "b")):
    """-> per case (worst gradient error x max|g64|, output error as a fraction of the oracle's range, running statistics error)."""
    res = {}
    for case in cases:
        out64, run64, g64 = oracle(case)
        m = trainable(device)
        out, grads = native_step(m, case, device)
        assert out.dtype == torch.float32 and len(grads) == len(dict(m.named_parameters())) == 93 and sorted(grads) == sorted(g64)
        frac = T.within_range(out.cpu(), out64, BAR, case)
        worst = 0.0
        for k, g in g64.items():
            scale = float(g64[k[:-4] + "weight"].abs().max()) if k in ZERO_BIASES else None
            worst = max(worst, rel(grads[k], g, (case, k), scale=scale))
        runerr = 0.0
        for k, b in m.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(b) == int(run64[k]) == 1, k
            else:
                runerr = max(runerr, close(b, run64[k], (case, k)))
        assert len(run64) == 9
        res[case] = (worst, frac, runerr)
    return res


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def f35():
    fx = {}
    files = sorted(glob.glob(os.path.join(GOLDEN, "f35_vitdec_train_*.npz")))
    assert files, "fixture F35 is missing (tests/golden/make_golden_vit_decoder_train.py)"
    for path in files:
        fx.update({k: v for k, v in load_golden(os.path.basename(path)).items() if k != "__name__"})
    return fx


def test_oracle_pinned_to_f35():
    """The fp64 oracle against everything F35 stores (the reference's own train-mode fp32 run): outputs, the nine buffers, the 93
    gradients (whole, or sample + sum + sum of squares), within MODULE_BAR x max|.|.  Measured: see the module docstring."""
    fx = f35()
    f27 = T.f27()
    assert int(fx["cot.seed"]) == COT_SEED
    for case, shape in CASES:
        h = hashlib.sha256()
        for t in T.inputs(f27, case):
            h.update(t.contiguous().numpy().tobytes())
        assert h.hexdigest() == fx[case + "/in.sha256"], "F35 was generated from other inputs than F27's"
        out64, run64, g64 = oracle(case)
        eo = rel(fx[case + "/out"], out64, (case, "out"))
        er = 0.0
        for k, v in run64.items():
            got = fx["%s/run/%s" % (case, k)]
            if k.endswith("num_batches_tracked"):
                assert int(got) == int(v) == 1, k
            else:
                er = max(er, rel(got, v, (case, k)))
        eg, seen = 0.0, 0
        for k, g in g64.items():
            scale = float(g64[k[:-4] + "weight"].abs().max()) if k in ZERO_BIASES else float(g.abs().max())
            if g.numel() <= 16384:
                eg = max(eg, rel(torch.as_tensor(fx["%s/g/%s" % (case, k)]), g, (case, k), scale=scale))       # (a 0-d array loads as a scalar)
            else:
                sample = g.flatten()[::g.numel() // 4096 + 1]
                eg = max(eg, rel(fx["%s/gx/%s" % (case, k)], sample, (case, k, "sample"), scale=scale))
                # an elementwise error of e = BAR max|g| moves the sum by at most numel e and the sum of squares by at most e (2 sum|g| + numel e)
                e = BAR * scale
                s, ss = (float(t) for t in fx["%s/gs/%s" % (case, k)])
                assert abs(s - float(g.sum())) <= g.numel() * e, (case, k, "sum")
                assert abs(ss - float((g * g).sum())) <= e * (2 * float(g.abs().sum()) + g.numel() * e), (case, k, "sum of squares")
            seen += 1
        assert seen == 93
        print("fp64 oracle vs F35 case %s: gradients %.3g x max|g| (bar %g), output %.3g x max|out|, running statistics %.3g" % (case, eg, BAR, eo, er))


def test_wgrad_against_fp64(emu):
    print("vitdec_wgrad vs fp64 (M = %s): worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (token_counts(), check_wgrad(emu), LAYER_BAR))


def test_slab_rule(emu):
    """Whole 32-token chunks, enough slabs for 512 workgroups over the tiles, never more slabs than chunks: the 36-tile 768 x 768 case
    fills the chip at M = 1300 (14 slabs x 36 tiles = 504 workgroups on 256 compute units)."""
    assert multi_slab_m() == 65
    assert [ops.vitdec_wgrad_slabs(m, 768, 768) for m in (1, 32, 33, 64, 65, 1300)] == [1, 1, 2, 2, 3, 14]
    assert ops.vitdec_wgrad_slabs(1300, 3072, 768) == 4 and ops.vitdec_wgrad_slabs(12800, 768, 768) == 15
    assert ops.vitdec_wgrad_slabs(30, 768, 64) == 0                    # not built: the wrapper's workspace query says so
    with pytest.raises(_lib.MvsHipError, match="built for"):
        ops.vitdec_wgrad(torch.zeros(4, 768), torch.zeros(4, 64))
    with pytest.raises(ValueError, match="built for"):
        ops.vitdec_pack(torch.zeros(4, 64))


def test_ln_bwd_against_fp64(emu):
    print("vitdec_ln_bwd vs fp64 autograd: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (check_ln_bwd(emu), LAYER_BAR))


def test_data_gradient_gemms_against_fp64(emu):
    print("data-gradient GEMMs vs fp64: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (check_dgrad(emu), LAYER_BAR))


def test_device_packing_is_the_host_packing():
    """pack_vitdec_block_train gives the bits of pack_vitdec_block, and its transposed operands are pack_linear_bf16x3(W^T)."""
    sd = {k[len("cross_attn_blocks.1."):]: v for k, v in T.f27_weights(T.f27()).items() if k.startswith("cross_attn_blocks.1.")}
    host, live = packing.pack_vitdec_block(sd), packing.pack_vitdec_block_train(sd)
    for k, v in host.items():
        assert torch.equal(v, live[k]), k
    assert torch.equal(live["fc1T"], packing.pack_linear_bf16x3(sd["mlp.fc1.weight"].t().contiguous()))
    assert torch.equal(live["kvT"], packing.pack_linear_bf16x3(torch.cat([sd["attn.k_proj.weight"], sd["attn.v_proj.weight"]], 0).t().contiguous()))
    assert "fc1T" not in packing.pack_vitdec_block_train(sd, transposed=False)


def test_block_nodes_against_fp64(emu):
    print("VitdecBlockTrain (self 0, cross 1, cross 2 on 2 x 2 views) vs fp64 autograd: forward = the inference bits; worst gradient |error| = %.3g x max|g64| (bar %g)"
          % (check_blocks(emu), BAR))


def test_mix_node_against_fp64(emu):
    print("VitdecMixTrain vs fp64 autograd: worst gradient |error| = %.3g x max|g64| (bar %g)" % (check_mix(emu), BAR))


@pytest.mark.parametrize("case", ["a", "b"])
def test_module_against_fp64(emu, case):
    worst, frac, run = check_module(emu, (case,))[case]
    print("vitdec_forward_train case %s vs fp64: worst gradient |error| = %.3g x max|g64| over 93 tensors (bar %g); output %.3g of its range; "
          "running statistics %.3g" % (case, worst, BAR, frac, run))


class _Net(torch.nn.Module):
    pass


def test_contract(emu):
    fx = T.f27()
    sd = T.f27_weights(fx)
    assert len(sd) == 102
    for mode in (True, False):
        net = _Net()
        net.decoder_vit = trainable("cpu", mode)
        old = net.decoder_vit
        assert patch_vit_decoder(net, trainable=True) is net
        new = net.decoder_vit
        assert type(new) is TrainableCrossVITDecoder and new is not old and new.training == mode
        assert sorted(new.state_dict()) == sorted(sd) and all(torch.equal(new.state_dict()[k], v) for k, v in sd.items())
        assert next(new.parameters()).device == next(old.parameters()).device
        assert type(patch_vit_decoder(net).decoder_vit) is CrossVITDecoder                # the default call: the inference form
    # eval(): the parent's inference forward, bit for bit
    m = trainable(emu, False)
    with torch.no_grad():
        assert torch.equal(m(T.inputs(fx, "b"), vit_shape=T.SHAPE_B), T.module(fx)(T.inputs(fx, "b"), vit_shape=T.SHAPE_B))
    # the backbone is frozen: no gradient into the ViT features
    m.train()
    x = [torch.zeros(1, 1, 2, 768) for _ in range(3)]
    with pytest.raises(NotImplementedError, match="frozen"):
        m([x[0], x[1].clone().requires_grad_(True), x[2]], vit_shape=[1, 1, 1, 2, 768])
    with pytest.raises(ValueError, match="three"):
        m(x[:2], vit_shape=[1, 1, 1, 2, 768])


def test_one_view_leaves_the_cross_blocks_without_gradient(emu):
    m = trainable(emu)
    x = [torch.randn(2, 1, 2, 768, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    out = m(x, vit_shape=[2, 1, 1, 2, 768])
    assert out.shape == (2, 64, 4, 8)
    out.square().sum().backward()
    for k, p in m.named_parameters():
        assert (p.grad is None) == k.startswith("cross_attn_blocks."), k


def test_second_step_uses_the_updated_weights(emu):
    """The packing-cache trap: weights are packed from the live parameters at every call, so an optimiser's in-place update is seen."""
    m = trainable(emu)
    x = [torch.randn(1, 1, 2, 768, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    shape = [1, 1, 1, 2, 768]
    first = m(x, vit_shape=shape).detach()
    with torch.no_grad():
        for p in m.self_attn_blocks[0].parameters():
            p.mul_(0.5)
    second = m(x, vit_shape=shape).detach()
    fresh = TrainableCrossVITDecoder(T.f27_args(T.f27()))
    fresh.load_state_dict(m.state_dict(), strict=True)
    assert not torch.equal(first, second) and torch.equal(second, fresh.train()(x, vit_shape=shape).detach())
