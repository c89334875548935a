"""The class-fused contraction of the (1,2,2) transposed convolutions 64 -> 32 and 32 -> 16 (csrc/conv_bf16x3_kernels.hip, BfDeconvF)
against the per-class loop.  Both forms live in one library; MVS_DECONV_CLASS_FUSED, read at every dispatch, forces the walk ("1") or
the loop ("0") - unset, the dispatch takes its measured choice per instantiation.  Every class sums the same K = 32 groups in the same order in both, so the outputs must be EQUAL bit for bit
(torch.equal): both layer shapes, the four activation / weight formats (fp32 and split tensors on the split-bf16 MFMAs, fp16 with two
weight terms, fp16 with one), with and without skip, ReLU on and off (the linear form of the training path), D in {3, 4, 8}, H and W
ragged against the tile and smaller than one tile.

The one-term format (MVS_PREC_F16) reads only w_hi in BOTH forms: its output equals the two-term format's on weights whose packed
lo half is zeroed, and the lo half the packer hands to such a layer is not zero (so the format does change values).

`-m gpu` runs the cases on the MI355X; the emulator twin (tests/hipemu) runs a reduced set of the same cases on the CPU."""
import pytest
import torch

from mvsformerplusplus_amd import _lib, ops, packing

SWITCH = "MVS_DECONV_CLASS_FUSED"
LAYERS = ((64, 32), (32, 16))
# (D, H, W): H, W not multiples of the 2 x 16 / 4 x 16 input tiles, and smaller than one tile
SHAPES = ((3, 6, 20), (4, 5, 33), (8, 7, 17), (4, 1, 5), (3, 3, 9), (8, 2, 16))
SHAPES_QUICK = ((3, 5, 20), (4, 1, 5), (8, 3, 17))
FORMATS = ("bf16x3", "split", "f16x2", "f16")


def _inputs(fmt, ci, co, shape, gen, batch=2):
    D, H, W = shape
    x = torch.randn(batch, D, H, W, ci, generator=gen)
    skip = torch.randn(batch, D, 2 * H, 2 * W, co, generator=gen)
    w = torch.randn(ci, co, 3, 3, 3, generator=gen) * 0.1
    bias = torch.randn(64, generator=gen)
    if fmt in ("f16x2", "f16"):
        wp = packing.f16x2(packing.pack_deconv_weights_bf16x3, w, 1)
        return x.half(), skip.half(), wp, bias, _lib.PREC_F16X2 if fmt == "f16x2" else _lib.PREC_F16
    wp = packing.pack_deconv_weights_bf16x3(w, 1)
    if fmt == "split":
        return ops.to_split(x), ops.to_split(skip), wp, bias, _lib.PREC_BF16X3_SPLIT
    return x, skip, wp, bias, _lib.PREC_BF16X3


def _both(monkeypatch, fn):
    """fn() through the class-fused walk and through the per-class loop"""
    monkeypatch.setenv(SWITCH, "1")
    fused = fn().cpu()
    monkeypatch.setenv(SWITCH, "0")
    loop = fn().cpu()
    monkeypatch.delenv(SWITCH, raising=False)
    return fused, loop


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def case_fused_equals_loop(device, monkeypatch, shapes, formats=FORMATS):
    gen = torch.Generator().manual_seed(77)
    n = 0
    for ci, co in LAYERS:
        for fmt in formats:
            for shape in shapes:
                x, skip, wp, bias, prec = _inputs(fmt, ci, co, shape, gen)
                xd, sd_, wd, bd = x.to(device), skip.to(device), wp.to(device), bias.to(device)
                for sk in (None, sd_):
                    fused, loop = _both(monkeypatch, lambda: ops.deconv3d_bn_relu_add(xd, wd, bd, co, 1, sk, prec))
                    assert fused.shape == (x.shape[0], shape[0], 2 * shape[1], 2 * shape[2], co)
                    assert bool(torch.isfinite(fused.float()).all()) and float(fused.float().abs().max()) > 0.1, (ci, co, fmt, shape)
                    assert torch.equal(_bits(fused), _bits(loop)), ("relu", ci, co, fmt, shape, sk is not None,
                                                                    float((fused.float() - loop.float()).abs().max()))
                    n += 1
                if fmt == "bf16x3":      # relu = 0: the linear layer of the training path (fp32 tensors, no skip, zero bias)
                    zb = torch.zeros(64, device=device)
                    fused, loop = _both(monkeypatch, lambda: ops.deconv3d_linear(xd, wd, zb, co, 1, prec))
                    assert float(fused.min()) < -0.1, "the linear form keeps negative values"
                    assert torch.equal(_bits(fused), _bits(loop)), ("linear", ci, co, shape, float((fused - loop).abs().max()))
                    n += 1
    return n


def case_switch_selects(device, monkeypatch):
    """Every setting of the switch gives the same bits (unset and empty: the dispatch's own choice), and a layer outside the walk (stride
    (2,2,2)) runs with it set either way."""
    gen = torch.Generator().manual_seed(5)
    x, skip, wp, bias, prec = _inputs("f16x2", 32, 16, (3, 4, 18), gen)
    args = [t.to(device) for t in (x, wp, bias)]
    monkeypatch.delenv(SWITCH, raising=False)
    ref = ops.deconv3d_bn_relu_add(args[0], args[1], args[2], 16, 1, None, prec).cpu()
    for val in ("0", "", "1"):
        monkeypatch.setenv(SWITCH, val)
        assert torch.equal(_bits(ops.deconv3d_bn_relu_add(args[0], args[1], args[2], 16, 1, None, prec).cpu()), _bits(ref)), val
    w2 = packing.f16x2(packing.pack_deconv_weights_bf16x3, torch.randn(32, 16, 3, 3, 3, generator=gen) * 0.1, 2).to(device)
    monkeypatch.setenv(SWITCH, "1")
    a = ops.deconv3d_bn_relu_add(args[0], w2, args[2], 16, 2, None, prec).cpu()
    monkeypatch.setenv(SWITCH, "0")
    b = ops.deconv3d_bn_relu_add(args[0], w2, args[2], 16, 2, None, prec).cpu()
    assert torch.equal(_bits(a), _bits(b))
    monkeypatch.delenv(SWITCH, raising=False)


def case_one_term_is_hi_only(device, monkeypatch):
    """MVS_PREC_F16 on the one-tile transposed kernels = the two-term kernel on weights without their lo half, in both forms and for
    the stride-(2,2,2) launches of the same kernel; the packed lo half is not zero, so dropping it is a change of arithmetic."""
    gen = torch.Generator().manual_seed(9)
    for ci, co, sd in ((64, 32, 1), (32, 16, 1), (64, 32, 2), (32, 16, 2)):
        x = torch.randn(1, 3, 5, 19, ci, generator=gen).half().to(device)
        skip = torch.randn(1, 3 * sd, 10, 38, co, generator=gen).half().to(device)
        w = torch.randn(ci, co, 3, 3, 3, generator=gen) * 0.1
        wp = packing.f16x2(packing.pack_deconv_weights_bf16x3, w, sd)
        halves = wp.clone().view(torch.int16).reshape(-1, 2, 512)          # [step x mb][hi | lo][lane x 8]
        assert int((halves[:, 1] != 0).sum()) > halves[:, 1].numel() // 2, "the packer writes a non-zero lo half"
        halves[:, 1] = 0
        wp_hi = halves.reshape(-1).view(wp.dtype)
        bias = torch.randn(64, generator=gen).to(device)
        for off in ("1", "0"):
            monkeypatch.setenv(SWITCH, off)
            one = ops.deconv3d_bn_relu_add(x, wp.to(device), bias, co, sd, skip, _lib.PREC_F16).cpu()
            two_hi = ops.deconv3d_bn_relu_add(x, wp_hi.to(device), bias, co, sd, skip, _lib.PREC_F16X2).cpu()
            two = ops.deconv3d_bn_relu_add(x, wp.to(device), bias, co, sd, skip, _lib.PREC_F16X2).cpu()
            assert torch.equal(_bits(one), _bits(two_hi)), (ci, co, sd, off)
            # fp16 weights carry 11 bits: the dropped term is 2^-11-class relative to the products
            assert float((one.float() - two.float()).abs().max()) <= 2e-3 * max(1.0, float(two.float().abs().max())), (ci, co, sd, off)
    monkeypatch.delenv(SWITCH, raising=False)


# ---- the MI355X -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def _real_library():
    import os
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    assert os.path.exists(_lib.LIB_PATH), "libmvs_hip.so missing: python -m mvsformerplusplus_amd.build"
    _lib.lib()
    assert _lib._REQUIRE_DEVICE
    yield


@pytest.mark.gpu
def test_fused_equals_loop(_real_library, monkeypatch):
    assert case_fused_equals_loop("cuda", monkeypatch, SHAPES) == 2 * len(FORMATS) * len(SHAPES) * 2 + 2 * len(SHAPES)


@pytest.mark.gpu
def test_fused_equals_loop_stage_shapes(_real_library, monkeypatch):
    """volumes with many tiles (every block of a full grid, several tiles along each axis)"""
    gen = torch.Generator().manual_seed(3)
    for (ci, co), shape in (((64, 32), (8, 36, 48)), ((32, 16), (8, 72, 96))):
        for fmt in ("f16x2", "f16"):
            x, skip, wp, bias, prec = _inputs(fmt, ci, co, shape, gen, batch=1)
            xd, sd_, wd, bd = x.cuda(), skip.cuda(), wp.cuda(), bias.cuda()
            fused, loop = _both(monkeypatch, lambda: ops.deconv3d_bn_relu_add(xd, wd, bd, co, 1, sd_, prec))
            assert torch.equal(_bits(fused), _bits(loop)), (ci, co, fmt)


@pytest.mark.gpu
def test_switch_selects(_real_library, monkeypatch):
    case_switch_selects("cuda", monkeypatch)


@pytest.mark.gpu
def test_one_term_is_hi_only(_real_library, monkeypatch):
    case_one_term_is_hi_only("cuda", monkeypatch)


# ---- the emulator twin (CPU) ----------------------------------------------------------------------------------------------
def test_emu_fused_equals_loop(emu, monkeypatch):
    assert case_fused_equals_loop(emu, monkeypatch, SHAPES_QUICK) > 0


def test_emu_switch_selects(emu, monkeypatch):
    case_switch_selects(emu, monkeypatch)


def test_emu_one_term_is_hi_only(emu, monkeypatch):
    case_one_term_is_hi_only(emu, monkeypatch)
