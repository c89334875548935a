"""Parity cases shared by tests/test_emu_parity.py (kernel sources run through the host emulator, CPU) and
tests/test_gpu_parity.py (-m gpu: the real libmvs_hip.so on an MI355X).  Every case drives the product API
(mvsformerplusplus_amd.*) on `device` and compares with the oracle / golden vectors on the CPU.

Tolerances: depth within 1e-3 relative L1 is the north-star bar (BASELINE.json); the checks below are far tighter
(fp32 MFMA is an exact fmaf chain, so differences are summation-order noise) and are written next to each assert.
"""
import os

import torch

from conftest import golden_weights, load_golden, rel_l1
from mvsformerplusplus_amd import _lib, module as M, ops, packing, synth
from mvsformerplusplus_amd.cost_volume import StageNet
from mvsformerplusplus_amd.warping import homo_warping_3D_with_mask
from oracle import ref_path as O

ARGS = {"base_ch": [8, 8, 8, 8], "depth_type": ["ce"] * 4, "fusion_type": "cnn", "cost_reg_type": ["Normal"] * 4}


# ---- precision parametrisation (round 4): `prec` None = the PRODUCT DEFAULT (the "stagemix" policy: fp32-equivalent coarse
# stages, "f16mix" fine stages - fp16 regulariser activations); "bf16x3" = the fp32-equivalent mode.  Every bound below is written as tol(prec, <fp32-equivalent bound>, <fp16 bound>); the
# fp16 bounds are ~3x what the emulator (bit-faithful for these kernels) measures on the fixture, and always far inside the 1e-3 depth bar.
def eff(prec):
    from conftest import PRODUCT_DEFAULT_PRECISION
    return prec or PRODUCT_DEFAULT_PRECISION


def is_f16(prec):
    """Does `prec` (None = the product default) store any regulariser activations as fp16?  The default policy "stagemix" does on the fine
    stages (the coarse ones run bf16x3): it is held to the fp16 bounds, which the all-fp16 formats meet too."""
    return eff(prec) in _lib.F16_FORMATS + ("stagemix",)


def tol(prec, exact, f16):
    return f16 if is_f16(prec) else exact


def with_prec(args, prec):
    return dict(args, conv_precision=prec) if prec else dict(args)


def dev(t, device):
    return t.to(device) if torch.is_tensor(t) else t


def cpu(t):
    return t.detach().cpu()


# ---------------------------------------------------------------- a2/a3
def case_warp_golden(device, tag):
    fx = load_golden("f1_warp_%s.npz" % tag)
    for dv, wk, mk in (("dv2", "warped2", "mask2"), ("dv4", "warped4", "mask4")):
        w, m = homo_warping_3D_with_mask(dev(fx["src_fea"], device), dev(fx["src_proj"], device), dev(fx["ref_proj"], device),
                                         dev(fx[dv], device))
        w, m = cpu(w), cpu(m)
        # mask flips only where a coordinate sits within rounding of the frame border
        assert (m != fx[mk]).float().mean() <= 2e-3
        assert (w - fx[wk]).abs().max() <= 2e-4, "warped features differ from the reference"
        assert (w - fx[wk]).abs().mean() <= 2e-6


def case_warp_siblings(device):
    """homo_warping_3D (no mask, warping.py:152-189) and the forward of diff_homo_warping_3D_with_mask (:112-149) against the same F1
    vectors - the reference computes the three from one formula."""
    from mvsformerplusplus_amd.warping import diff_homo_warping_3D_with_mask, homo_warping_3D
    fx = load_golden("f1_warp_b.npz")
    args = [dev(fx[k], device) for k in ("src_fea", "src_proj", "ref_proj", "dv4")]
    w = cpu(homo_warping_3D(*args))
    assert (w - fx["warped4"]).abs().max() <= 2e-4
    w2, m2 = diff_homo_warping_3D_with_mask(*args)
    assert torch.equal(cpu(w2), w) and (cpu(m2) != fx["mask4"]).float().mean() <= 2e-3
    try:
        diff_homo_warping_3D_with_mask(args[0], args[1], args[2], args[3].clone().requires_grad_(True))
    except NotImplementedError:
        pass
    else:
        raise AssertionError("the forward-only form must refuse hypotheses that require grad")


def case_warp_dtypes(device):
    fx = load_golden("f1_warp_a.npz")
    for dt, tol in ((torch.bfloat16, 1e-6), (torch.float16, 1e-6)):
        src = fx["src_fea"].to(dt)
        w, _ = homo_warping_3D_with_mask(dev(src, device), dev(fx["src_proj"], device), dev(fx["ref_proj"], device), dev(fx["dv4"], device))
        wo, _ = O.homo_warping_3D_with_mask(src.float(), fx["src_proj"], fx["ref_proj"], fx["dv4"])
        assert (cpu(w) - wo).abs().max() <= 2e-4        # the kernel upcasts the same low-precision values exactly


# ---------------------------------------------------------------- a7-a9
def _load_regnet(net, sd, device):
    net.load_state_dict(sd, strict=True)
    return net.eval().to(device)


def case_regnet_golden(device, name, prec=None):
    fx = load_golden(name)
    sd = golden_weights(fx)
    net = M.CostRegNet3D(8, 8) if "3d" in name else M.CostRegNet(8, 8)
    net = _load_regnet(net, sd, device)
    if prec:
        net.conv_precision = prec
    assert net.conv_precision == (prec or M.DEFAULT_PRECISION)          # a bare regulariser module: the layer-level default ("f16mix")
    with torch.no_grad():
        y = cpu(net(dev(fx["x"], device)))
    assert y.shape == fx["y"].shape
    scale = float(fx["y"].abs().max())
    err = float((y - fx["y"]).abs().max()) / max(1.0, scale)
    # fp16: the input volume and ten layers of activations carry 2^-12 relative rounding each (standalone regulariser: NCDHW fp32 in)
    assert err <= tol(prec, 2e-4, 1.5e-3), "regulariser logits differ from the reference: %g" % err
    return err


def case_precisions(device):
    """Both contraction modes of the MFMA convolutions against the reference's regulariser output:
    fp32 (v_mfma_f32_16x16x4_f32, an exact fmaf chain) and bf16x3 (3-term split bf16, ~2^-16 per product)."""
    for name in ("f3_costregnet.npz", "f3_costregnet3d_d8.npz"):
        fx = load_golden(name)
        sd = golden_weights(fx)
        errs = {}
        for prec in ("fp32", "bf16x3"):
            net = M.CostRegNet3D(8, 8) if "3d" in name else M.CostRegNet(8, 8)
            net = _load_regnet(net, sd, device)
            net.conv_precision = prec
            with torch.no_grad():
                y = cpu(net(dev(fx["x"], device)))
            errs[prec] = float((y - fx["y"]).norm() / fx["y"].norm())
        assert errs["fp32"] <= 2e-6, errs            # summation-order noise only
        assert errs["bf16x3"] <= 5e-5, errs          # 2^-16-class product error, 10 layers deep
    fx = load_golden("f2_stage_s1.npz")
    for prec, tol in (("fp32", 5e-6), ("bf16x3", 2e-5)):
        net = make_stage(fx, fx["hyp"].shape[1], 1, device)
        net.conv_precision = prec
        with torch.no_grad():
            out = net(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), float(fx["tmp"]))
        assert rel_l1(cpu(out["depth"]), fx["depth"]) <= tol, prec
    try:
        net.conv_precision = "fp8"
        with torch.no_grad():
            net(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), 5.0)
    except ValueError:
        pass
    else:
        raise AssertionError("unknown precision names must be rejected")


def case_single_layers(device, prec=None):
    """Conv3d / Deconv3d wrappers one layer at a time against torch's own conv (fp32 reference of the same op).  Product default (fp16
    activations): input and output each carry one fp16 rounding (2^-12 relative of the value, here a few 1e-4 of the output range)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    lt = tol(prec, 1e-4, 1.5e-3)
    for cin, cout, stride, shape in ((8, 16, (2, 2, 2), (8, 8, 24)), (8, 16, (1, 2, 2), (4, 8, 40)), (16, 16, 1, (5, 6, 20)),
                                     (32, 64, (1, 2, 2), (3, 8, 16)), (64, 64, 1, (2, 5, 17))):
        layer = M.Conv3d(cin, cout, stride=stride, padding=1)
        man = synth.state_dict_manifest(layer.state_dict())
        layer.load_state_dict(synth.seeded_state_dict(man, 5))
        layer = layer.eval().to(device)
        if prec:
            layer.conv_precision = prec
        x = torch.randn(2, cin, *shape, generator=g)
        ref = F.relu(F.batch_norm(F.conv3d(x, layer.conv.weight.cpu(), None, stride=stride, padding=1), layer.bn.running_mean.cpu(),
                                  layer.bn.running_var.cpu(), layer.bn.weight.cpu(), layer.bn.bias.cpu(), False, 0.1, 1e-5))
        with torch.no_grad():
            y = cpu(layer(dev(x, device)))
        assert y.shape == ref.shape
        assert (y - ref).abs().max() <= lt * max(1.0, float(ref.abs().max())), (cin, cout, stride)
    for cin, cout, sd, shape in ((64, 32, 2, (2, 3, 5)), (32, 16, 2, (3, 4, 18)), (16, 8, 2, (4, 5, 16)),
                                 (64, 32, 1, (3, 2, 5)), (16, 8, 1, (4, 6, 17))):
        layer = M.Deconv3d(cin, cout, stride=(sd, 2, 2), padding=1, output_padding=(sd - 1, 1, 1))
        man = synth.state_dict_manifest(layer.state_dict())
        layer.load_state_dict(synth.seeded_state_dict(man, 6))
        layer = layer.eval().to(device)
        if prec:
            layer.conv_precision = prec
        x = torch.randn(1, cin, *shape, generator=g)
        ref = F.relu(F.batch_norm(F.conv_transpose3d(x, layer.conv.weight.cpu(), None, stride=(sd, 2, 2), padding=1,
                                                     output_padding=(sd - 1, 1, 1)), layer.bn.running_mean.cpu(),
                                  layer.bn.running_var.cpu(), layer.bn.weight.cpu(), layer.bn.bias.cpu(), False, 0.1, 1e-5))
        with torch.no_grad():
            y = cpu(layer(dev(x, device)))
        assert y.shape == ref.shape
        assert (y - ref).abs().max() <= lt * max(1.0, float(ref.abs().max())), (cin, cout, sd)


# ---------------------------------------------------------------- a7-a9 outside the tuned tables (shape-generic exact-fp32 kernel)
def case_generic_conv_layers(device):
    """Conv3d / Deconv3d wrappers on layer shapes NO tuned kernel exists for (other channel counts, 1x1x1 / 3x1x1 / 5x3x3 / even kernels,
    padding 0, stride 3, no BatchNorm / no ReLU forms) against torch's own fp32 convolution: the shape-generic kernel is exact fp32, the
    bound is summation-order noise."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(21)
    convs = ((4, 8, 3, 2, 1, (6, 7, 9), {}), (12, 6, 3, (1, 2, 2), 1, (3, 8, 10), {}), (5, 3, 1, 1, 0, (2, 5, 7), {}),
             (8, 1, 3, 1, 1, (4, 5, 6), {"bn": False, "relu": False}), (3, 10, (3, 1, 1), 1, (1, 0, 0), (5, 4, 6), {"relu": False}),
             (6, 7, (5, 3, 3), (1, 3, 2), (2, 0, 1), (7, 9, 8), {}), (16, 16, 2, 2, 0, (4, 6, 8), {"bn": False}),
             (128, 8, 3, 1, 1, (2, 3, 5), {}), (8, 16, 3, 2, 0, (5, 7, 9), {"bn": False}))
    for cin, cout, k, st, pad, shape, kw in convs:
        layer = M.Conv3d(cin, cout, kernel_size=k, stride=st, padding=pad, **kw)
        layer.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(layer.state_dict()), 5))
        layer = layer.eval().to(device)
        assert not layer.is_tuned(), (cin, cout, k, st, pad)
        x = torch.randn(2, cin, *shape, generator=g)
        ref = F.conv3d(x, layer.conv.weight.cpu(), None if layer.conv.bias is None else layer.conv.bias.cpu(), stride=st, padding=pad)
        if layer.bn is not None:
            ref = F.batch_norm(ref, layer.bn.running_mean.cpu(), layer.bn.running_var.cpu(), layer.bn.weight.cpu(), layer.bn.bias.cpu(), False, 0.1, 1e-5)
        if layer.relu:
            ref = F.relu(ref)
        with torch.no_grad():
            y = cpu(layer(dev(x, device)))
        assert y.shape == ref.shape, (y.shape, ref.shape)
        assert (y - ref).abs().max() <= 2e-5 * max(1.0, float(ref.abs().max())), (cin, cout, k, st, pad, float((y - ref).abs().max()))
    deconvs = ((8, 4, 3, 2, 1, 1, (3, 4, 5), {}), (6, 10, 3, (1, 2, 2), 1, (0, 1, 1), (3, 4, 6), {}), (4, 4, 2, 2, 0, 0, (3, 3, 4), {"bn": False, "relu": False}),
               (5, 2, (3, 3, 1), (2, 3, 1), (1, 0, 0), (1, 2, 0), (3, 4, 5), {"relu": False}), (16, 8, 3, 2, 1, 0, (3, 4, 5), {}),
               (16, 8, 3, 2, 1, 1, (3, 4, 5), {"bn": False}))
    for cin, cout, k, st, pad, op, shape, kw in deconvs:
        layer = M.Deconv3d(cin, cout, kernel_size=k, stride=st, padding=pad, output_padding=op, **kw)
        layer.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(layer.state_dict()), 6))
        layer = layer.eval().to(device)
        assert not layer.is_tuned(), (cin, cout, k, st, pad, op)
        x = torch.randn(2, cin, *shape, generator=g)
        ref = F.conv_transpose3d(x, layer.conv.weight.cpu(), None if layer.conv.bias is None else layer.conv.bias.cpu(), stride=st, padding=pad,
                                 output_padding=op)
        if layer.bn is not None:
            ref = F.batch_norm(ref, layer.bn.running_mean.cpu(), layer.bn.running_var.cpu(), layer.bn.weight.cpu(), layer.bn.bias.cpu(), False, 0.1, 1e-5)
        if layer.relu:
            ref = F.relu(ref)
        with torch.no_grad():
            y = cpu(layer(dev(x, device)))
        assert y.shape == ref.shape, (y.shape, ref.shape)
        assert (y - ref).abs().max() <= 2e-5 * max(1.0, float(ref.abs().max())), (cin, cout, k, st, pad, op, float((y - ref).abs().max()))
    # the C ABI refuses output sizes that do not follow from the layer arithmetic, and skip tensors of another shape
    x = dev(torch.randn(1, 3, 4, 4, 4, generator=g), device)
    w = dev(torch.randn(27, 4, 5, generator=g), device)
    for bad in (lambda: ops.conv3d_generic(x.permute(0, 2, 3, 4, 1).contiguous(), w, None, 5, (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # Cin mismatch
                lambda: ops.conv3d_generic(x, w[:, :3].contiguous()[:, :, :4].contiguous(), None, 4, (3, 3, 3), (1, 1, 1), (1, 1, 1),
                                           skip_cl=x)):                                                                           # skip shape
        try:
            bad()
        except _lib.MvsHipError:
            pass
        else:
            raise AssertionError("a mismatching weight / skip tensor must be refused")
    xc = dev(torch.randn(1, 4, 4, 4, 3, generator=g), device)
    y = torch.empty(1, 9, 9, 9, 5, device=xc.device)
    try:                                                               # the bound library raises on a status other than MVS_OK
        _lib.lib().mvs_conv3d_generic_fwd(_lib.ptr(xc), _lib.ptr(dev(torch.randn(27, 3, 5, generator=g), device)), None, None, _lib.ptr(y), 1, 3, 5, 4, 4, 4,
                                          9, 9, 9, 3, 3, 3, 2, 2, 2, 1, 1, 1, 1, 0, None)
        err = ""
    except _lib.MvsHipError as e:
        err = str(e)
    assert err.startswith("mvs_conv3d_generic_fwd failed (code 1)"), \
        "output size 9 of a stride-2 k3 p1 transposed layer on 4 inputs (valid: 7, 8) must be MVS_ERR_ARG; got '%s'" % err


def case_generic_conv_fuzz(device, n_cases=60, seed=0):
    """Seeded random layer shapes through ops.conv3d_generic (both forms, with / without bias, ReLU, skip) against torch's fp32 convolutions:
    kernel 1..4 per axis, stride 1..3, padding 0..2, output padding < stride, 1..20 channels, ragged sizes."""
    import random
    import torch.nn.functional as F
    rnd = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    done = 0
    while done < n_cases:
        transposed = rnd.random() < 0.5
        k = tuple(rnd.randint(1, 4) for _ in range(3))
        st = tuple(rnd.randint(1, 3) for _ in range(3))
        pad = tuple(rnd.randint(0, min(2, k[i] - 1) if transposed else 2) for i in range(3))
        op = tuple(rnd.randint(0, st[i] - 1) for i in range(3)) if transposed else (0, 0, 0)
        cin, cout, B = rnd.randint(1, 20), rnd.choice([1, 2, 3, 4, 5, 8, 9, 16, 17]), rnd.randint(1, 2)
        size = tuple(rnd.randint(1, 7) for _ in range(3))
        if not transposed and any(size[i] + 2 * pad[i] < k[i] for i in range(3)):
            continue
        x = torch.randn(B, cin, *size, generator=g)
        bias = torch.randn(cout, generator=g) if rnd.random() < 0.6 else None
        relu = rnd.random() < 0.5
        if transposed:
            if any((size[i] - 1) * st[i] - 2 * pad[i] + k[i] + op[i] < 1 for i in range(3)):
                continue                                       # no output voxel along an axis: torch refuses the layer too
            w = torch.randn(cin, cout, *k, generator=g) * 0.3
            ref = F.conv_transpose3d(x, w, bias, stride=st, padding=pad, output_padding=op)
            wt = packing.pack_generic_deconv_weights(w)
        else:
            w = torch.randn(cout, cin, *k, generator=g) * 0.3
            ref = F.conv3d(x, w, bias, stride=st, padding=pad)
            wt = packing.pack_generic_conv_weights(w)
        if ref.numel() == 0:
            continue
        if relu:
            ref = F.relu(ref)
        skip = torch.randn(ref.shape, generator=g) if rnd.random() < 0.4 else None
        if skip is not None:
            ref = ref + skip
        cl = lambda t: None if t is None else dev(t.permute(0, 2, 3, 4, 1).contiguous(), device)
        y = ops.conv3d_generic(cl(x), dev(wt, device), None if bias is None else dev(bias, device), cout, k, st, pad, relu, cl(skip), transposed, op)
        y = cpu(y).permute(0, 4, 1, 2, 3)
        assert y.shape == ref.shape, (transposed, k, st, pad, op, y.shape, ref.shape)
        err = float((y - ref).abs().max())
        assert err <= 3e-5 * max(1.0, float(ref.abs().max())), (transposed, k, st, pad, op, cin, cout, size, err)
        done += 1


def case_regnet_generic_golden(device):
    """Fixture F16 from the reference: regularisers whose in_channels differ from base_channels (`inner` 1x1x1 convolution,
    module.py:385-388 / 481-484), other base widths, last_layer=False and log_var=True - all on the shape-generic kernel."""
    fx = load_golden("f16_regnet_inner.npz")
    made = {"crn_4_8": lambda: M.CostRegNet(4, 8), "crn_12_4": lambda: M.CostRegNet(12, 4), "crn_8_8_nolast": lambda: M.CostRegNet(8, 8, last_layer=False),
            "crn3d_12_8": lambda: M.CostRegNet3D(12, 8), "crn3d_6_6": lambda: M.CostRegNet3D(6, 6), "crn3d_8_8_logvar": lambda: M.CostRegNet3D(8, 8, log_var=True)}
    errs = {}
    for tag, make in made.items():
        net = make()
        net.load_state_dict(golden_weights(fx, prefix=tag + ".w."), strict=True)      # reference state-dict names (incl. inner.weight / .bias), strict
        net = net.eval().to(device)
        assert net.is_generic, tag
        with torch.no_grad():
            y = cpu(net(dev(fx[tag + ".x"], device)))
        want = fx[tag + ".y"]
        assert y.shape == want.shape, (tag, y.shape, want.shape)
        errs[tag] = float((y - want).abs().max()) / max(1.0, float(want.abs().max()))
        assert errs[tag] <= 2e-5, "generic regulariser %s differs from the reference: %g" % (tag, errs[tag])
    # a volume whose size the U-Net's skip adds do not fit is refused with the reference's constraint spelled out
    net = M.CostRegNet(4, 4).eval().to(device)
    try:
        with torch.no_grad():
            net(dev(torch.zeros(1, 4, 8, 12, 16), device))
    except ValueError as e:
        assert "divisible by 8" in str(e)
    else:
        raise AssertionError("H = 12 cannot pass three stride-2 levels")
    return errs


def case_position_encoding_golden(device):
    """Fixture F19 from the reference: get_position_3d with and without normalisation, PositionEncoding3D as a tensor of its own."""
    from mvsformerplusplus_amd import PositionEncoding3D, get_position_3d
    fx = load_golden("f19_position_encoding.npz")
    B, D, H, W = fx["hyp"].shape
    K, hyp = dev(fx["K"], device), dev(fx["hyp"], device)
    pos, hmin, hmax, wmin, wmax = get_position_3d(B, H, W, K, hyp, 425.0, 935.0, None, None, None, None, normalize=True)
    assert torch.allclose(cpu(pos), fx["position3d"], rtol=1e-4, atol=2e-6)
    assert torch.allclose(torch.stack([cpu(hmin), cpu(hmax), cpu(wmin), cpu(wmax)]), fx["ranges"], rtol=1e-5)
    raw, a, b, c, d = get_position_3d(B, H, W, K, hyp, 425.0, 935.0, None, 1.0, None, None, normalize=False)
    assert (a, b, c, d) == (None, 1.0, None, None), "normalize=False hands the range arguments back untouched (position_encoding.py:150,163)"
    assert torch.allclose(cpu(raw), fx["position3d_raw"], rtol=1e-5, atol=1e-4)
    for C, rescale in ((8, 4.0), (6, 2.5)):
        pe = cpu(PositionEncoding3D(dev(fx["position3d"], device), C, rescale=rescale))
        assert pe.shape == fx["pe_c%d" % C].shape
        assert (pe - fx["pe_c%d" % C]).abs().max() <= 2e-6, (C, float((pe - fx["pe_c%d" % C]).abs().max()))
    try:
        PositionEncoding3D(dev(fx["position3d"], device), 5)
    except _lib.MvsHipError:
        pass
    else:
        raise AssertionError("an odd channel count must be refused")


def case_costregnet2d_golden(device):
    """Fixture F18 from the reference: CostRegNet2D (module.py:411-450) at base 8 and 4 - (1,3,3) strided / transposed layers on the
    shape-generic kernel, strict state-dict load."""
    fx = load_golden("f18_costregnet2d.npz")
    errs = {}
    for tag, base in (("b8", 8), ("b4", 4)):
        net = M.CostRegNet2D(base, base)
        net.load_state_dict(golden_weights(fx, prefix=tag + ".w."), strict=True)
        net = net.eval().to(device)
        assert net.is_generic
        with torch.no_grad():
            y = cpu(net(dev(fx[tag + ".x"], device)))
        want = fx[tag + ".y"]
        assert y.shape == want.shape
        errs[tag] = float((y - want).abs().max()) / max(1.0, float(want.abs().max()))
        assert errs[tag] <= 2e-5, (tag, errs[tag])
    return errs


def case_stage_other_groups_golden(device, tag, prec=None):
    """Fixture F15 from the reference: StageNet with base_ch != 8 (cost_volume.py:29-49) - the direct gather with G groups, an fp32 volume
    [B,D,H,W,G], the CostRegNet(G, G) / CostRegNet3D(G, G) of the reference's own widths on the shape-generic kernel.  conv_precision only
    selects the visibility CNN's format here (its fp16 form shifts the volume by ~1e-4)."""
    fx = load_golden("f15_stage_%s.npz" % tag)
    D, G = fx["hyp"].shape[1], int(fx["base_ch"])
    args = with_prec(dict(ARGS, base_ch=[G] * 4), prec)
    net = StageNet(args, D, int(fx["stage_idx"]))
    net.load_state_dict(golden_weights(fx), strict=True)
    net = net.eval().to(device)
    assert net._generic_regulariser() and not net._f16_activations() and not net._split_activations()
    with torch.no_grad():
        out = net(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), float(fx["tmp"]))
    assert set(out) == {"depth", "prob_volume", "photometric_confidence", "depth_values", "prob_volume_pre"}
    errs = (rel_l1(cpu(out["depth"]), fx["depth"]), float((cpu(out["prob_volume_pre"]) - fx["prob_volume_pre"]).abs().max()),
            float((cpu(out["prob_volume"]) - fx["prob_volume"]).abs().max()),
            float((cpu(out["photometric_confidence"]) - fx["photometric_confidence"]).abs().max()))
    assert errs[0] <= tol(prec, 2e-5, 2e-4), "stage depth vs reference (bar: 1e-3): %g" % errs[0]
    assert errs[1] <= tol(prec, 5e-4, 1e-2), errs
    assert errs[2] <= tol(prec, 1e-4, 2e-3) and errs[3] <= tol(prec, 1e-4, 2e-3), errs
    return errs


def case_cascade_other_groups_vs_oracle(device, G=4, prec=None):
    """A whole 4-stage cascade with base_ch = G != 8 against the oracle (64 x 128, V = 3): hypothesis scheduling, both U-Net kinds and
    the confidence average downstream of the generic stages."""
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    args = with_prec({"base_ch": [G] * 4, "depth_type": ["ce"] * 4, "fusion_type": "cnn", "cost_reg_type": ["Normal"] * 4, "ndepths": [32, 16, 8, 4],
                      "depth_interals_ratio": [4.0, 2.67, 1.5, 1.0], "inverse_depth": True}, prec)
    head = CascadeDepthHead(dict(args))
    for i, st in enumerate(head.fusions):
        st.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(st.state_dict()), 40 + i), strict=True)
    head = head.eval()
    feats, projs, dv = synth.make_cascade_inputs(64, 128, 3, seed=5, rot_deg=1.0)
    sds = [dict(st.state_dict()) for st in head.fusions]
    with torch.no_grad():
        ref = O.cascade_forward(feats, projs, dv, sds, ndepths=args["ndepths"], depth_interals_ratio=args["depth_interals_ratio"], base_ch=args["base_ch"])
        head = head.to(device)
        out = head({k: dev(v, device) for k, v in feats.items()}, {k: dev(v, device) for k, v in projs.items()}, dev(dv, device))
    e = rel_l1(cpu(out["refined_depth"]), ref["refined_depth"])
    c = float((cpu(out["photometric_confidence"]) - ref["photometric_confidence"]).abs().max())
    assert e <= tol(prec, 5e-5, 5e-4), "refined depth vs oracle (bar 1e-3): %g" % e
    assert c <= tol(prec, 2e-3, 5e-2), c
    return e, c


# ---------------------------------------------------------------- a1-a12 one stage
def make_stage(fx, ndepth, stage_idx, device, depth_type="ce", prec=None):
    args = with_prec(ARGS, prec)
    args["depth_type"] = [depth_type] * 4
    net = StageNet(args, ndepth, stage_idx)
    net.load_state_dict(golden_weights(fx), strict=True)      # reference state-dict names, strict
    return net.eval().to(device)


def case_stage_golden(device, tag, prec=None):
    fx = load_golden("f2_stage_%s.npz" % tag)
    D = fx["hyp"].shape[1]
    net = make_stage(fx, D, int(fx["stage_idx"]), device, prec=prec)
    assert net.precision_policy == eff(prec) and net.conv_precision == M.resolve_stage_precision(eff(prec), D)[0]
    with torch.no_grad():
        out = net(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), float(fx["tmp"]))
    assert set(out) == {"depth", "prob_volume", "photometric_confidence", "depth_values", "prob_volume_pre"}
    errs = (rel_l1(cpu(out["depth"]), fx["depth"]), float((cpu(out["prob_volume_pre"]) - fx["prob_volume_pre"]).abs().max()),
            float((cpu(out["prob_volume"]) - fx["prob_volume"]).abs().max()),
            float((cpu(out["photometric_confidence"]) - fx["photometric_confidence"]).abs().max()))
    assert errs[0] <= tol(prec, 2e-5, 2e-4), "stage depth vs reference (bar: 1e-3): %g" % errs[0]       # fp16: measured 5e-5 .. 6e-5
    assert errs[1] <= tol(prec, 5e-4, 1e-2), errs                                                         # logits: 1.3e-3 .. 3.3e-3
    assert errs[2] <= tol(prec, 1e-4, 2e-3), errs                                                         # probabilities: 1e-4 .. 6e-4
    assert errs[3] <= tol(prec, 1e-4, 2e-3), errs
    return errs


def case_stage_bd_hypotheses(device, prec=None):
    """depth_values of shape [B, D] (one set of fronto-parallel planes for every pixel) against fixture F14 from the reference; the output
    dict hands the caller's [B, D] tensor back under 'depth_values' like the reference does."""
    fx = load_golden("f14_stage_bd_hyp.npz")
    net = make_stage(fx, fx["hyp"].shape[1], 3, device, prec=prec)
    hyp = dev(fx["hyp"], device)
    assert hyp.dim() == 2
    with torch.no_grad():
        out = net(dev(fx["features"], device), dev(fx["proj"], device), hyp, 1.0)
    assert out["depth_values"].shape == hyp.shape
    e = (rel_l1(cpu(out["depth"]), fx["depth"]), float((cpu(out["prob_volume"]) - fx["prob_volume"]).abs().max()),
         float((cpu(out["photometric_confidence"]) - fx["photometric_confidence"]).abs().max()))
    assert e[0] <= tol(prec, 2e-5, 2e-4), e
    assert e[1] <= tol(prec, 1e-4, 2e-3) and e[2] <= tol(prec, 1e-4, 2e-3), e
    return e


def case_stage_pieces(device):
    """Intermediate tensors of one stage (entropy, visibility, cost volume) against the oracle's intermediates."""
    fx = load_golden("f2_stage_s1.npz")
    sd = golden_weights(fx)
    feats, proj, hyp = fx["features"], fx["proj"], fx["hyp"]
    ref = O.stage_forward(feats, proj, hyp, 5.0, sd, G=8, return_intermediates=True)
    net = make_stage(fx, hyp.shape[1], 1, device)
    f, code = ops._feat(dev(feats, device))
    hom = ops.compose_homography(dev(proj, device))
    ent = ops.warp_corr_entropy(f, code, hom, dev(hyp, device), 8)
    assert (cpu(ent) - ref["entropy"].squeeze(2)).abs().max() <= 2e-5
    for prec in ("fp32", "bf16x3"):
        net.conv_precision = prec
        vis = ops.vis_weight(ent, net._vis_params(f.device), _lib.PRECISIONS[prec])
        # fp32: summation order only; bf16x3: 2^-16-class product error through three conv layers (measured 2e-5 max on MI355X)
        assert (cpu(vis) - ref["vis_weight"].squeeze(2)).abs().max() <= (2e-5 if prec == "fp32" else 1e-4), prec
    net.conv_precision = "fp32"
    vis = ops.vis_weight(ent, net._vis_params(f.device), _lib.PRECISIONS["fp32"])
    vol, _ = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8)
    assert (cpu(vol).permute(0, 4, 1, 2, 3) - ref["volume_mean"]).abs().max() <= 2e-5
    # partial (view-sharded) form: two halves summed and normalised == the fused single pass
    v1, s1 = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8, normalise=False, view_begin=1, view_end=2)
    v2, s2 = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8, normalise=False, view_begin=2, view_end=3)
    both = ops.volume_normalise_(v1 + v2, s1 + s2)
    assert (cpu(both) - cpu(vol)).abs().max() <= 1e-6


def case_stage_modes(device, prec=None):
    """The 'ce' head in its train-time form (argmax; the stage runs its TRAINING path, which keeps fp32 activations on the bf16x3 kernels
    whatever conv_precision says) and the 'reg' head (expectation + confidence window) at inference, fixtures F6."""
    fx = load_golden("f6_stage_train_ce.npz")
    net = make_stage(fx, 8, 2, device, prec=prec)
    net.training = True                                   # BN layers stay in eval mode, like the fixture
    with torch.no_grad():
        out = net(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), 5.0)
    e0 = float((cpu(out["depth"]) != fx["depth"]).float().mean())
    e1 = float((cpu(out["prob_volume"]) - fx["prob_volume"]).abs().max())
    assert e0 <= 0.005, e0                                # argmax may flip on exact near-ties only
    assert e1 <= 1e-4, e1
    fx = load_golden("f6_stage_reg.npz")
    net = make_stage(fx, 8, 2, device, depth_type="reg", prec=prec)
    with torch.no_grad():
        out = net(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), 1.0)
    e2 = rel_l1(cpu(out["depth"]), fx["depth"])
    e3 = float((cpu(out["photometric_confidence"]) - fx["photometric_confidence"]).abs().max())
    assert e2 <= tol(prec, 2e-5, 2e-4), e2                # fp16: measured 4.6e-5
    assert e3 <= tol(prec, 1e-4, 1e-3), e3                # 2.6e-4
    return e0, e1, e2, e3


def case_stage_lowp_features(device, prec=None):
    """bf16 / fp16 feature inputs are upcast per element in-kernel (reference: cost_volume.py:67,81,84)."""
    fx = load_golden("f2_stage_s3.npz")
    sd = golden_weights(fx)
    net = make_stage(fx, 4, 3, device, prec=prec)
    errs = []
    for dt in (torch.bfloat16, torch.float16):
        f = fx["features"].to(dt)
        ref = O.stage_forward(f.float(), fx["proj"], fx["hyp"], 1.0, sd, G=8)
        with torch.no_grad():
            out = net(dev(f, device), dev(fx["proj"], device), dev(fx["hyp"], device), 1.0)
        errs.append(rel_l1(cpu(out["depth"]), ref["depth"]))
        assert errs[-1] <= tol(prec, 2e-5, 2e-4), errs      # fp16: measured 4.8e-5
        if dt == torch.float16:
            # the same features handed over as fp16 octet tiles (the emitter's fp16 hand-off): in the fp16 gather forms the taps are read straight
            # from the tiles (gather_lds.h, the direct form (`gl_direct_v`) - no window) - the same values in the same order: every output bit for bit
            with torch.no_grad():
                out_t = net(ops.pack_features(dev(f, device)), dev(fx["proj"], device), dev(fx["hyp"], device), 1.0)
            same = all(torch.equal(cpu(out[k]), cpu(out_t[k])) for k in ("depth", "photometric_confidence", "prob_volume"))
            if net.gather_precision == "f16":
                assert same, "fp16 tiles (direct gather) must reproduce planar fp16 features (fp16 windows) bit for bit"
            else:
                assert rel_l1(cpu(out_t["depth"]), cpu(out["depth"])) <= 1e-6
    return errs


# ---------------------------------------------------------------- a10-a15 small functions
def case_auto_policy(device, quick=False):
    """conv_precision="auto" (opt-in, round 5): CascadeDepthHead picks the uniform "f16mix" format while depth_max / depth_min stays below half the
    ratio at which the inverse-depth schedule degenerates ((ndepths[0] - 1) / ratio[1] + 1 = 12.6), the default policy's exact coarse stages
    otherwise - per call, from the depth_values it is handed (cached per tensor).  Bit-identical to the explicitly configured head either way."""
    def head_of(policy):
        h, _ = _seeded_head(device, conv_precision=policy)
        return h
    auto = head_of("auto")
    assert [f.precision_policy for f in auto.fusions] == ["auto"] * 4 and auto.fusions[0].conv_precision == "bf16x3"     # unresolved: the safe form
    for inputs, want in ((dict(), "f16mix"), (dict(numdepth=64, depth_min=0.5, depth_interval=9.5 / 63, baseline=0.03), "stagemix"),
                         (dict(numdepth=64, depth_min=0.5, depth_interval=2.5 / 63, baseline=0.03), "f16mix"))[:2 if quick else 3]:
        feats, projs, dv = synth.make_cascade_inputs(64, 64, 3, seed=3, rot_deg=1.0, **inputs)
        fd, pd, dd = {k: dev(v, device) for k, v in feats.items()}, {k: dev(v, device) for k, v in projs.items()}, dev(dv, device)
        with torch.no_grad():
            out = auto(fd, pd, dd)
            assert [f.precision_policy for f in auto.fusions] == [want] * 4, (inputs, [f.precision_policy for f in auto.fusions])
            ref = head_of(want)(fd, pd, dd)
            again = out if quick else auto(fd, pd, dd)       # cached decision: no second read of the range
        for k in ("refined_depth", "photometric_confidence"):
            assert torch.equal(cpu(out[k]), cpu(ref[k])) and torch.equal(cpu(out[k]), cpu(again[k])), (want, k)
    # a StageNet on its own (the reference's loop hands it hypotheses, not the range) resolves "auto" like the default policy
    st = StageNet(dict(ARGS, conv_precision="auto"), 32, 0)
    assert (st.conv_precision, st.gather_precision) == ("bf16x3", "f32")


def case_feature_heads(device):
    """SURVEY section 8f #4, producer side (round 5): TiledFeatureHead - the feature side's last 3x3 convolution emitting the octet-tiled
    hand-off layout from its epilogue - against fixture F20 (inputs / outputs of the reference's own FMT_with_pathway.smooth_k and
    FPNDecoder.out_k, captured with hooks): fp32 tiles to 2e-5 of the output range (split-bf16 MFMA = fp32-equivalent), bf16 tiles = the
    reference output rounded once to bf16 (what its autocast hands over, test.py:250) up to one bf16 ulp; filling a [B,V,C/8,H,W,8]
    buffer view by view == all views at once; the emitted tiles feed StageNet like packed features; unsupported widths are refused."""
    import torch.nn as nn
    from mvsformerplusplus_amd import TiledFeatureHead
    fx = load_golden("f20_feature_heads.npz")
    for k in (1, 2, 3):
        x, y = fx["fmt%d_x" % k], fx["fmt%d_y" % k]
        B, V, C, H, W = y.shape
        conv = nn.Conv2d(C, C, 3, padding=1, bias=False)
        conv.weight.data.copy_(fx["fmt%d_w" % k])
        scale = max(1.0, float(y.abs().max()))
        head32 = TiledFeatureHead(conv, dtype=torch.float32).to(device)
        got = cpu(head32(dev(x, device)).unpack())
        assert got.shape == y.shape and (got - y).abs().max() <= 2e-5 * scale, ("fmt", k, float((got - y).abs().max()))
        head = TiledFeatureHead(conv).to(device)                                   # bf16 tiles, the default hand-off dtype
        pk = head(dev(x, device))
        assert pk.dtype == torch.bfloat16 and pk.data.shape == (B, V, C // 8, H, W, 8)
        want = y.to(torch.bfloat16).float()
        d = (cpu(pk.unpack()).float() - want).abs()
        assert d.max() <= 2.0 ** -7 * scale and float((d > 0).float().mean()) <= 0.02, ("fmt bf16", k)      # rare one-ulp flips at rounding ties
        buf = head.new_buffer(B, V, H, W, device)
        for v in range(V):                                                          # the reference's per-view loop (FMT.py:231-233), in place
            head(dev(x[:, v], device), out=buf, view=v)
        assert torch.equal(cpu(buf.data), cpu(pk.data)), "view-by-view fill must equal the all-views launch"
        h16 = TiledFeatureHead(conv, dtype=torch.float16).to(device)
        assert (cpu(h16(dev(x.half(), device)).unpack()).float() - O.feature_head(x.half().float().flatten(0, 1), fx["fmt%d_w" % k]).view_as(y)).abs().max() <= 2e-3 * scale
        # FPN head: Conv2d(64, C) + BatchNorm2d (folded) + Swish
        xs, ys = fx["fpn%d_x" % k], fx["fpn%d_y" % k]
        co = ys.shape[1]
        seq = nn.Sequential(nn.Conv2d(64, co, 3, padding=1), nn.BatchNorm2d(co, eps=float(fx["fpn%d_bn_eps" % k])), nn.SiLU()).eval()
        seq[0].weight.data.copy_(fx["fpn%d_w" % k]); seq[0].bias.data.copy_(fx["fpn%d_b" % k])
        for n in ("weight", "bias", "running_mean", "running_var"):
            getattr(seq[1], n).data.copy_(fx["fpn%d_bn_%s" % (k, n)])
        hf = TiledFeatureHead.from_sequential(seq, dtype=torch.float32).to(device)
        got = cpu(hf(dev(xs, device)).unpack())[:, 0]
        assert (got - ys).abs().max() <= 3e-5 * max(1.0, float(ys.abs().max())), ("fpn", k, float((got - ys).abs().max()))
    # consumer side: the emitted stage-4 tiles go through a StageNet exactly like features packed by mvs_pack_features
    #   (own input of a size the U-Net takes - F20's maps are 20 rows tall; the expected features come from the oracle's feature_head)
    B, V, C, H, W = 1, 3, 8, 16, 72
    x = torch.randn(B, V, C, H, W, generator=torch.Generator().manual_seed(8))
    conv = nn.Conv2d(C, C, 3, padding=1, bias=False)
    conv.weight.data.copy_(fx["fmt3_w"])
    y = O.feature_head(x.flatten(0, 1), fx["fmt3_w"]).view(B, V, C, H, W)
    emitted = TiledFeatureHead(conv).to(device)(dev(x, device))
    packed = ops.pack_features(dev(y, device), dtype=torch.bfloat16)
    st = StageNet(dict(ARGS), 4, 3)
    st.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(st.state_dict()), 9), strict=True)
    st = st.eval().to(device)
    cams = synth.make_cameras(V, H * 4, W * 4, baseline=30.0, seed=1, batch=B)
    cams[:, :, 1, :2, :] /= 4
    hyp = (torch.linspace(800, 500, 4)[None, :, None, None] * torch.ones(B, 4, H, W)).contiguous()
    with torch.no_grad():
        o1 = st(emitted, dev(cams, device), dev(hyp, device), 1.0)
        o2 = st(packed, dev(cams, device), dev(hyp, device), 1.0)
    assert rel_l1(cpu(o1["depth"]), cpu(o2["depth"])) <= 2e-4, "emitted tiles vs packed reference features through a stage"
    bad = nn.Conv2d(24, 24, 3, padding=1, bias=False)
    try:
        TiledFeatureHead(bad).to(device)(dev(torch.zeros(1, 24, 8, 8), device))
        raise AssertionError("an unsupported head width must be refused")
    except RuntimeError as e:
        assert "built for" in str(e), str(e)


def case_fused_small_launches(device):
    """Round 5: the cascade's folded launches are BIT-identical to the stand-alone kernels they replace -
    mvs_cascade_prologue_fwd == 4 x mvs_compose_homography + mvs_init_range_fwd; mvs_softmax_regress_confavg_fwd == mvs_softmax_regress_fwd
    + mvs_confidence_average; and CascadeDepthHead (fused path) == the same stages called one by one the way the reference's own cascade loop
    (DINOv2_mvsformer_model.py:120-179, through patch_model) calls them."""
    g = torch.Generator().manual_seed(5)
    B, V = 2, 4
    projs = []
    for s in range(4):
        cams = synth.make_cameras(V, 64, 96, baseline=30.0 + s, rot_deg=1.5, seed=s, batch=B)
        cams[:, :, 1, :2, :] *= 2.0 ** (s - 3)
        projs.append(dev(cams, device))
    for inverse in (True, False):
        dv = dev(torch.linspace(425.0, 931.0, 192)[None].repeat(B, 1) * torch.tensor([[1.0], [1.1]]), device)
        homs, hyp = ops.cascade_prologue(projs, dv, 32, 8, 12, inverse=inverse)
        for s in range(4):
            assert torch.equal(cpu(homs[s]), cpu(ops.compose_homography(projs[s]))), ("prologue homographies", s)
        assert torch.equal(cpu(hyp), cpu(ops.init_range(dv, 32, 8, 12, inverse=inverse))), "prologue hypotheses"
    homs, none = ops.cascade_prologue(projs[:2])                     # homographies only
    assert none is None and torch.equal(cpu(homs[1]), cpu(ops.compose_homography(projs[1])))
    for D, (H, W) in ((4, (16, 24)), (8, (16, 24)), (6, (8, 16))):     # 6: the run-time-D head variant
        logits = dev(torch.randn(B, D, H, W, generator=g) * 3.0, device)
        hyp = dev(500.0 + 100.0 * torch.rand(B, D, H, W, generator=g), device)
        prev = [dev(torch.rand(B, H >> k, W >> k, generator=g), device) for k in (3, 2, 1)]
        for mode, conf_n in ((_lib.HEAD_CE_EVAL, 0), (_lib.HEAD_REG, 2)):
            d0, c0, p0 = ops.softmax_regress(logits, hyp, 5.0, mode, conf_n, True)
            d1, c1, p1, avg = ops.softmax_regress(logits, hyp, 5.0, mode, conf_n, True, conf_prev=prev)
            assert torch.equal(cpu(d0), cpu(d1)) and torch.equal(cpu(c0), cpu(c1)) and torch.equal(cpu(p0), cpu(p1))
            assert torch.equal(cpu(avg), cpu(ops.confidence_average(prev + [c0], H, W))), ("fused confidence average", D, mode)
        d1, c1, _, avg = ops.softmax_regress(logits, hyp, 1.0, _lib.HEAD_CE_EVAL, 0, False, conf_prev=[])      # a one-stage cascade
        assert torch.equal(cpu(avg), cpu(c1))
    # head + the next stage's schedule in one launch == head, then schedule_inverse_range: tiles with ragged edges, several D, odd sizes
    for D, Dn, (H, W), ratio in ((32, 16, (16, 40), 2.67), (8, 4, (9, 70), 1.0), (6, 5, (20, 33), 1.5), (16, 8, (8, 32), 1.5)):
        logits = dev(torch.randn(B, D, H, W, generator=g) * 3.0, device)
        hyp = dev((torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.02 * torch.rand(B, D, H, W, generator=g))).contiguous(), device)
        for mode, conf_n, wp in ((_lib.HEAD_CE_EVAL, 0, True), (_lib.HEAD_REG, 2, False)):
            d0, c0, p0 = ops.softmax_regress(logits, hyp, 5.0, mode, conf_n, wp)
            d1, c1, p1, nh = ops.softmax_regress_schedule(logits, hyp, 5.0, mode, conf_n, wp, Dn, ratio)
            assert torch.equal(cpu(d0), cpu(d1)) and torch.equal(cpu(c0), cpu(c1)) and (p0 is None or torch.equal(cpu(p0), cpu(p1))), ("fused head", D, H, W)
            want = cpu(ops.schedule_inverse_range(d0, hyp, Dn, ratio, 2 * H, 2 * W))
            assert nh.shape == want.shape and rel_l1(cpu(nh), want) <= 1e-7 and (cpu(nh) - want).abs().max() <= 2e-6 * float(want.abs().max()), ("fused schedule", D, H, W)
    # the whole cascade: fused driver vs the stage-by-stage calls of the reference's loop
    head, args = _seeded_head(device)
    feats, projm, dvs = synth.make_cascade_inputs(64, 128, 3, seed=4, rot_deg=1.0)
    feats, projm, dvs = {k: dev(v, device) for k, v in feats.items()}, {k: dev(v, device) for k, v in projm.items()}, dev(dvs, device)
    with torch.no_grad():
        out = head(feats, projm, dvs)
        so, confs = None, []
        for s in range(4):
            key = "stage%d" % (s + 1)
            H, W = feats[key].shape[-2:]
            hyp = (M.init_inverse_range(dvs, args["ndepths"][0], dvs.device, dvs.dtype, H, W) if s == 0 else
                   M.schedule_inverse_range(so["depth"], so["depth_values"], args["ndepths"][s], args["depth_interals_ratio"][s], H, W))
            so = head.fusions[s](feats[key], projm[key], hyp, tmp=[5.0, 5.0, 5.0, 1.0][s])
            assert set(so) == {"depth", "prob_volume", "photometric_confidence", "depth_values", "prob_volume_pre"}
            assert set(out[key]) == set(so), "the fused driver must return the reference's five keys per stage"
            # stage 1 has no fused input: bit-equal.  Later stages consume next_hyp, which the header (mvs_hip.h, mvs_softmax_regress_schedule_fwd)
            # only promises up to FMA contraction (<= 2e-6 of its range, asserted above): the same bar here
            assert torch.equal(cpu(so["depth"]), cpu(out[key]["depth"])) or (s > 0 and rel_l1(cpu(out[key]["depth"]), cpu(so["depth"])) <= 1e-6), \
                ("stage depth, fused vs stage-by-stage", s)
            confs.append(so["photometric_confidence"])
        assert torch.equal(cpu(out["photometric_confidence"]), cpu(ops.confidence_average(confs, *feats["stage4"].shape[-2:])))


def case_small_fns(device):
    fx = load_golden("f5_small_fns.npz")
    for D, n in ((32, 4), (16, 3), (8, 2)):
        p, dv = dev(fx["p%d" % D], device), dev(fx["dv%d" % D], device)
        assert torch.allclose(cpu(M.depth_regression(p, dv)), fx["dreg%d" % D], rtol=1e-5, atol=0)
        assert torch.allclose(cpu(M.conf_regression(p, n=n)), fx["conf%d_n%d" % (D, n)], rtol=1e-5, atol=1e-6)
    dv = dev(fx["depth_values"], device)
    assert torch.allclose(cpu(M.init_range(dv, 8, dv.device, dv.dtype, 5, 6)), fx["init_range"], rtol=1e-6, atol=0)
    assert torch.allclose(cpu(M.init_inverse_range(dv, 8, dv.device, dv.dtype, 5, 6)), fx["init_inverse_range"], rtol=1e-6, atol=0)
    got = M.schedule_inverse_range(dev(fx["prev_depth"], device), dev(fx["prev_hyp"], device), 4, 2.67, 10, 12)
    assert torch.allclose(cpu(got), fx["schedule_inverse_range"], rtol=2e-6, atol=0)
    got = M.schedule_range(dev(fx["prev_depth"], device), 4, dev(fx["schedule_range_itv"], device), 10, 12)
    assert torch.allclose(cpu(got), fx["schedule_range"], rtol=2e-6, atol=0)


def case_range_variants(device):
    """Fixture F17 from the reference: per-pixel initial ranges, schedule_inverse_range(shift=True), per-pixel depth intervals."""
    fx = load_golden("f17_range_variants.npz")
    px = dev(fx["pixel_ranges"], device)
    assert torch.allclose(cpu(M.init_range(px, 8, px.device, px.dtype, 5, 6)), fx["init_range_pixel"], rtol=1e-6, atol=0)
    assert torch.allclose(cpu(M.init_inverse_range(px, 8, px.device, px.dtype, 5, 6)), fx["init_inverse_range_pixel"], rtol=1e-6, atol=0)
    pd, ph = dev(fx["prev_depth"], device), dev(fx["prev_hyp"], device)
    got = cpu(M.schedule_inverse_range(pd, ph, 4, 1.0, 10, 12, shift=True))
    assert torch.allclose(got, fx["schedule_inverse_range_shift"], rtol=5e-6, atol=0)
    plain = cpu(M.schedule_inverse_range(pd, ph, 4, 1.0, 10, 12))
    assert float((got - plain).abs().max()) > 1.0, "shift=True must change the hypotheses of this fixture"
    got = M.schedule_range(pd, 4, dev(fx["schedule_range_itv_pixel"], device), 10, 12)
    assert torch.allclose(cpu(got), fx["schedule_range_pixel"], rtol=2e-6, atol=0)
    for bad in (lambda: M.init_range(px[:, :, :, 0], 8, px.device, px.dtype, 5, 6), lambda: M.init_range(px, 8, px.device, px.dtype, 6, 5)):
        try:
            bad()
        except (ValueError, _lib.MvsHipError):
            pass
        else:
            raise AssertionError("a range tensor of the wrong rank / map size must be refused")


def case_generic_shapes(device):
    """Ragged sizes and the run-time-shape kernel variants: HW not a multiple of 64, C/G outside the templated set,
    D without a register-resident head, empty view ranges rejected."""
    g = torch.Generator().manual_seed(3)
    B, V, C, G, D, H, W = 2, 3, 12, 4, 5, 9, 13
    cams = synth.make_cameras(V, H * 8, W * 8, baseline=40.0, rot_deg=3.0, seed=1, batch=B)
    cams[:, :, 1, :2, :] /= 8
    feats = torch.randn(B, V, C, H, W, generator=g)
    hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.05 * torch.rand(B, D, H, W, generator=g))).contiguous()
    ref_p = O.compose_proj(cams[:, 0])
    f, code = ops._feat(dev(feats, device))
    hom = ops.compose_homography(dev(cams, device))
    ent = cpu(ops.warp_corr_entropy(f, code, hom, dev(hyp, device), G))
    vis = torch.rand(B, V - 1, H, W, generator=g)
    vol, _ = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), dev(vis, device), G)
    vsum, acc = 0.0, 0.0
    for v in range(1, V):
        warped, _ = O.homo_warping_3D_with_mask(feats[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
        ip = O.group_correlation(feats[:, 0], warped, G)
        assert (ent[:, v - 1] - O.entropy_of_similarity(ip)[:, 0]).abs().max() <= 2e-5
        acc = acc + ip * vis[:, v - 1][:, None, None]
        vsum = vsum + vis[:, v - 1]
    expect = acc / (vsum[:, None, None] + 1e-6)
    assert (cpu(vol).permute(0, 4, 1, 2, 3) - expect).abs().max() <= 2e-5
    # run-time-D head (D = 5 has no register variant) on given logits
    logits = torch.randn(B, D, H, W, generator=g) * 3
    depth, conf, pv = ops.softmax_regress(dev(logits, device), dev(hyp, device), 5.0, _lib.HEAD_CE_EVAL)
    assert torch.allclose(cpu(depth), O.depth_regression(torch.softmax(logits * 5.0, 1), hyp), rtol=1e-5)
    assert torch.allclose(cpu(pv), torch.softmax(logits, 1), rtol=1e-5, atol=1e-7)
    assert torch.allclose(cpu(conf), torch.softmax(logits, 1).max(1)[0], rtol=1e-5)
    try:
        ops.warp_corr_entropy(f, code, hom, dev(hyp, device), G, view_begin=2, view_end=2)
    except _lib.MvsHipError:
        pass
    else:
        raise AssertionError("an empty source-view range must be rejected")
    try:
        ops.warp_corr_entropy(f, code, hom, dev(hyp, device), 5)      # G does not divide C
    except _lib.MvsHipError:
        pass
    else:
        raise AssertionError("G must divide C (cost_volume.py:87)")


def case_vis_cnn(device):
    """Row-streaming visibility CNN against the oracle on sizes that exercise several 60-column strips, several row segments,
    ragged right / bottom edges and images smaller than one strip."""
    g = torch.Generator().manual_seed(21)
    st = StageNet(dict(ARGS), 8, 2)
    st.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(st.state_dict()), 9), strict=True)
    st = st.eval()
    sd = {k: v.detach().clone() for k, v in st.state_dict().items()}
    st = st.to(device)
    for (N, H, W) in ((3, 37, 130), (2, 70, 61), (1, 9, 24), (2, 64, 120)):
        ent = torch.rand(1, N, H, W, generator=g) * 2.0
        ref = torch.stack([O.vis_weight(ent[:, n:n + 1], sd) for n in range(N)], 1)[:, :, 0]      # [1, N, H, W]
        # f16x2: fp16 rings (2^-11) through two layers + the sigmoid; f16 / f16mix: the same with ONE fp16 weight term
        for prec, tol in (("bf16x3", 1e-4), ("fp32", 2e-5), ("f16x2", 3e-3), ("f16", 4e-3), ("f16mix", 4e-3)):
            st.conv_precision = prec
            vis = ops.vis_weight(dev(ent, device), st._vis_params(torch.device(device) if isinstance(device, str) else device), _lib.PRECISIONS[prec])
            assert vis.shape == ent.shape
            err = float((cpu(vis) - ref).abs().max())
            assert err <= tol, (N, H, W, prec, err)


def case_gather_variants(device, quick=False):
    """LDS-staged gather passes against the oracle over every channel-octet count (C = 8..64), depth-chunk geometry
    (D = 4, 8, 16, 32, 48: 1 / 2 / 4 work-items per pixel, looping for D > 16), ragged tiles (W not a multiple of the tile
    width), bf16 features, out-of-frame taps, and the block-uniform fallback for windows larger than the LDS capacity
    (per-pixel hypotheses that jump across the whole range make the tap bounding box cover > 1024 source positions)."""
    g = torch.Generator().manual_seed(11)
    cases = [(8, 4, 12, 24, False, torch.float32), (16, 8, 10, 40, False, torch.float32), (32, 16, 9, 24, False, torch.float32),
             (64, 32, 8, 16, False, torch.float32), (8, 48, 6, 24, False, torch.float32), (16, 6, 36, 48, True, torch.float32),
             (8, 4, 36, 64, True, torch.bfloat16)]
    if quick:
        cases = cases[:2] + cases[5:6]
    for C, D, H, W, wild, dt in cases:
        B, V, G = 1, 3, 8
        cams = synth.make_cameras(V, H * 8, W * 8, baseline=60.0, rot_deg=2.0, seed=C + D, batch=B)
        cams[:, :, 1, :2, :] /= 8
        feats = torch.randn(B, V, C, H, W, generator=g).to(dt)
        if wild:      # every pixel draws its own hypotheses from the whole range: taps of one tile scatter over the image
            hyp = 430.0 + 500.0 * torch.rand(B, D, H, W, generator=g)
        else:
            hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.03 * torch.rand(B, D, H, W, generator=g))).contiguous()
        ref_p = O.compose_proj(cams[:, 0])
        f, code = ops._feat(dev(feats, device))
        hom = ops.compose_homography(dev(cams, device))
        ent = cpu(ops.warp_corr_entropy(f, code, hom, dev(hyp, device), G))
        vis = torch.rand(B, V - 1, H, W, generator=g)
        vol, _ = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), dev(vis, device), G)
        vsum, acc = 0.0, 0.0
        ff = feats.float()
        for v in range(1, V):
            warped, _ = O.homo_warping_3D_with_mask(ff[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
            ip = O.group_correlation(ff[:, 0], warped, G)
            assert (ent[:, v - 1] - O.entropy_of_similarity(ip)[:, 0]).abs().max() <= 5e-5, (C, D, "entropy")
            acc = acc + ip * vis[:, v - 1][:, None, None]
            vsum = vsum + vis[:, v - 1]
        expect = acc / (vsum[:, None, None] + 1e-6)
        scale = max(1.0, float(expect.abs().max()))
        assert (cpu(vol).permute(0, 4, 1, 2, 3) - expect).abs().max() <= 5e-5 * scale, (C, D, "volume")
        # streaming pass 2 of the fp16 formats: pass 1 keeps the per-view group correlations as fp16, corr_aggregate streams them
        hd = dev(hyp, device)
        assert ops.gather_keeps_correlations(f, G, hd), (C, D, "the keeping pass exists for every LDS-staged shape")
        if True:
            for fk in (f, ops.pack_features(f)):
                # the fp16 formats' gather (MVS_GATHER_F16): the SOURCE features are rounded to fp16 once, nothing else changes
                ent_k, corr = ops.warp_corr_entropy_keep(fk, ops._feat(fk)[1], hom, hd, G)
                ent_w = ops.warp_corr_entropy(fk, ops._feat(fk)[1], hom, hd, G, f16_window=True)
                assert (cpu(ent_k) - cpu(ent_w)).abs().max() <= 2e-5, (C, D, "fp16-window entropy pass == keeping pass")
                acc16, f16src = 0.0, ff.half().float()
                for v in range(1, V):
                    warped, _ = O.homo_warping_3D_with_mask(f16src[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
                    ip = O.group_correlation(ff[:, 0], warped, G)
                    assert (cpu(ent_k)[:, v - 1] - O.entropy_of_similarity(ip)[:, 0]).abs().max() <= 5e-5, (C, D, v, "entropy, fp16 source features")
                    got = cpu(corr[:, v - 1]).float().permute(0, 4, 1, 2, 3)
                    assert (got - ip).abs().max() <= 6e-4 * max(1.0, float(ip.abs().max())), (C, D, v, "kept correlations")   # one fp16 rounding
                    acc16 = acc16 + ip * vis[:, v - 1][:, None, None]
                expect16 = acc16 / (vsum[:, None, None] + 1e-6)
                assert (expect16 - expect).abs().max() <= 1e-3 * scale, (C, D, "effect of the rounded source features")
                vol_k = cpu(ops.corr_aggregate(corr, dev(vis, device))).float().permute(0, 4, 1, 2, 3)
                assert (vol_k - expect16).abs().max() <= 1.2e-3 * scale, (C, D, "streamed volume")                           # two fp16 roundings
                # ... and in the other regulariser formats (a bf16x3 / transformer stage under the "stagemix" policy): fp32 and split bf16
                vol_f = cpu(ops.corr_aggregate(corr, dev(vis, device), f16=False)).permute(0, 4, 1, 2, 3)
                assert vol_f.dtype == torch.float32 and (vol_f - expect16).abs().max() <= 6e-4 * scale, (C, D, "streamed volume, fp32 out")
                vol_s = cpu(ops.from_split(ops.corr_aggregate(corr, dev(vis, device), split=True))).permute(0, 4, 1, 2, 3)
                assert (vol_s - vol_f).abs().max() <= 2e-5 * scale, (C, D, "streamed volume, split out")
                vol16 = cpu(ops.warp_corr_aggregate(fk, ops._feat(fk)[1], hom, hd, dev(vis, device), G, f16=True)[0]).float().permute(0, 4, 1, 2, 3)
                assert (vol_k - vol16).abs().max() <= 1.2e-3 * scale, (C, D, "streamed vs gathered fp16 volume")
                if dt == torch.float32 and fk is not f:
                    # fp16 octet tiles (the producer-side emitter's other hand-off dtype): the fp16 window is staged by a pure 16-byte copy
                    # (gather_lds.h) - the same bits as planar fp16 features, whose staging converts fp16 -> fp32 -> fp16
                    fh = dev(feats.half(), device)
                    e_p, c_p = ops.warp_corr_entropy_keep(fh, ops._feat(fh)[1], hom, hd, G)
                    ft16 = ops.pack_features(fh)
                    e_t, c_t = ops.warp_corr_entropy_keep(ft16, ops._feat(ft16)[1], hom, hd, G)
                    assert ft16.dtype == torch.float16 and torch.equal(cpu(e_p), cpu(e_t)) and torch.equal(cpu(c_p), cpu(c_t)), (C, D, "fp16 tiles: copy staging")
                    v_p = ops.warp_corr_aggregate(fh, ops._feat(fh)[1], hom, hd, dev(vis, device), G, f16=True)[0]
                    v_t = ops.warp_corr_aggregate(ft16, ops._feat(ft16)[1], hom, hd, dev(vis, device), G, f16=True)[0]
                    assert torch.equal(cpu(v_p), cpu(v_t)), (C, D, "fp16 tiles: copy staging, pass 2")
                    w_p = ops.warp_corr_entropy(fh, ops._feat(fh)[1], hom, hd, G, f16_window=True)
                    w_t = ops.warp_corr_entropy(ft16, ops._feat(ft16)[1], hom, hd, G, f16_window=True)
                    assert torch.equal(cpu(w_p), cpu(w_t)), (C, D, "fp16 tiles: plain pass 1")
                if D <= 4:
                    continue
                # round 5: the EXACT keeping pass (MVS_CORR_F32: fp32 windows, fp32 kept correlations - the coarse stages of the default
                # policy): entropy == the plain pass 1, kept correlations == the oracle's, streamed volume == the second gather's
                ent_x, corr_x = ops.warp_corr_entropy_keep(fk, ops._feat(fk)[1], hom, hd, G, exact=True)
                assert corr_x.dtype == torch.float32 and (cpu(ent_x) - ent).abs().max() <= 2e-6, (C, D, "exact keeping pass: entropy")
                for v in range(1, V):
                    warped, _ = O.homo_warping_3D_with_mask(ff[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
                    ip = O.group_correlation(ff[:, 0], warped, G)
                    assert (cpu(corr_x[:, v - 1]).permute(0, 4, 1, 2, 3) - ip).abs().max() <= 5e-5 * max(1.0, float(ip.abs().max())), (C, D, v, "exact kept correlations")
                vol_x = cpu(ops.corr_aggregate(corr_x, dev(vis, device), f16=False)).permute(0, 4, 1, 2, 3)
                assert (vol_x - cpu(vol).permute(0, 4, 1, 2, 3)).abs().max() <= 4e-6 * scale, (C, D, "exact streamed volume == second gather")
                vol_xs = cpu(ops.from_split(ops.corr_aggregate(corr_x, dev(vis, device), split=True))).permute(0, 4, 1, 2, 3)
                assert (vol_xs - vol_x).abs().max() <= 2e-5 * scale, (C, D, "exact streamed volume, split out")
        if D <= 4:
            try:
                ops.warp_corr_entropy_keep(f, code, hom, hd, G, exact=True)
                raise AssertionError("D <= 4 must be refused by the EXACT keeping pass")
            except RuntimeError as e:
                assert "D > 4" in str(e), str(e)
        # hand-off layout: the same features octet-tiled give the same numbers, in fp32 and - packed
        # down to bf16 - the numbers of bf16 planar features
        for pdt in (None, torch.bfloat16):
            if pdt is not None and dt != torch.float32:
                continue
            pk = ops.pack_features(f, pdt)
            assert tuple(pk.shape) == tuple(f.shape) and pk.data.shape[-1] == 8
            if pdt is None:
                assert torch.equal(cpu(pk.unpack()), cpu(f)), "pack_features must be a pure re-layout"
                ent_p, vol_p = ent, cpu(vol)
            else:
                fb, cb = ops._feat(dev(feats.to(pdt), device))
                assert torch.equal(cpu(pk.unpack()), cpu(fb)), "fp32 -> bf16 packing must round like .to(bfloat16)"
                ent_p = cpu(ops.warp_corr_entropy(fb, cb, hom, dev(hyp, device), G))
                vol_p = cpu(ops.warp_corr_aggregate(fb, cb, hom, dev(hyp, device), dev(vis, device), G)[0])
            ent_t = cpu(ops.warp_corr_entropy(pk, ops._feat(pk)[1], hom, dev(hyp, device), G))
            vol_t = cpu(ops.warp_corr_aggregate(pk, ops._feat(pk)[1], hom, dev(hyp, device), dev(vis, device), G)[0])
            assert (ent_t - ent_p).abs().max() <= 1e-6 and (vol_t - vol_p).abs().max() <= 1e-6 * scale, (C, D, "tiled layout", pdt)
        # partial (view-sharded) form == fused form
        v1, s1 = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), dev(vis, device), G, normalise=False, view_begin=1, view_end=2)
        v2, s2 = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), dev(vis, device), G, normalise=False, view_begin=2, view_end=3)
        both = ops.volume_normalise_(v1 + v2, s1 + s2)
        assert (cpu(both) - cpu(vol)).abs().max() <= 2e-6 * scale, (C, D, "partial sums")


def case_gather_windows(device):
    """Gather passes against the oracle on a wide-baseline rig with per-pixel hypothesis jitter: source windows from a few dozen to
    several hundred positions in one launch, tiles whose taps all fall outside the source image, border-clamped 2x2 blocks."""
    g = torch.Generator().manual_seed(5)
    for C, D, H, W, amp in ((8, 4, 24, 64, 0.3), (16, 8, 24, 64, 0.1)):
        B, V, G = 1, 3, 8
        cams = synth.make_cameras(V, H * 8, W * 8, baseline=300.0, rot_deg=2.0, seed=C + D, batch=B)
        cams[:, :, 1, :2, :] /= 8
        feats = torch.randn(B, V, C, H, W, generator=g)
        hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + amp * torch.rand(B, D, H, W, generator=g))).contiguous()
        hom = ops.compose_homography(dev(cams, device))
        f, code = ops._feat(dev(feats, device))
        ent = cpu(ops.warp_corr_entropy(f, code, hom, dev(hyp, device), G))
        vis = torch.rand(B, V - 1, H, W, generator=g)
        vol = cpu(ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), dev(vis, device), G)[0])
        ref_p = O.compose_proj(cams[:, 0])
        acc, vsum = 0.0, 0.0
        for v in range(1, V):
            warped, _ = O.homo_warping_3D_with_mask(feats[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
            ip = O.group_correlation(feats[:, 0], warped, G)
            assert (ent[:, v - 1] - O.entropy_of_similarity(ip)[:, 0]).abs().max() <= 5e-5, (C, D, "entropy")
            acc = acc + ip * vis[:, v - 1][:, None, None]
            vsum = vsum + vis[:, v - 1]
        expect = acc / (vsum[:, None, None] + 1e-6)
        assert (vol.permute(0, 4, 1, 2, 3) - expect).abs().max() <= 5e-5 * max(1.0, float(expect.abs().max())), (C, D, "volume")


def case_split_format(device):
    """The split activation format of the inference U-Net (MVS_PREC_BF16X3_SPLIT: per voxel C/8 octets of [hi x8 | lo x8] bf16):
    every convolution / transposed convolution (with and without skip, both strides, the fused and the 3x3x3 head, the whole
    U-Nets) fed with to_split(x) gives from_split(y) equal to the fp32-format path up to the split's 2^-17-class rounding, the
    aggregate pass writes exactly to_split(volume), and mvs_volume_normalise converts in place."""
    from mvsformerplusplus_amd import _lib
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 3, 5, 7, 32, generator=g) * torch.logspace(-6, 3, 32)
    s = ops.to_split(x)
    assert s.shape == x.shape and s.dtype == torch.float32
    assert (ops.from_split(s) - x).abs().max() <= 2.0 ** -16 * x.abs().max()
    P1, P3 = _lib.PREC_BF16X3, _lib.PREC_BF16X3_SPLIT
    for ci, co, stride in ((8, 16, (2, 2, 2)), (8, 16, (1, 2, 2)), (16, 16, (1, 1, 1)), (16, 32, (2, 2, 2)), (16, 32, (1, 2, 2)), (32, 32, (1, 1, 1)),
                           (32, 64, (2, 2, 2)), (32, 64, (1, 2, 2)), (64, 64, (1, 1, 1))):
        xx = torch.randn(2, 6, 10, 20, ci, generator=g)                     # ragged tiles: 10 x 20 is not a multiple of 4 x 16
        w = torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1
        wp = dev(packing.pack_conv_weights_bf16x3(w, packing.conv_chunk(ci, stride)), device)
        b = dev(torch.randn(64, generator=g), device)
        y1 = cpu(ops.conv3d_bn_relu(dev(xx, device), wp, b, co, 3, stride, True, P1))
        y3 = ops.from_split(cpu(ops.conv3d_bn_relu(dev(ops.to_split(xx), device), wp, b, co, 3, stride, True, P3)))
        assert (y1 - y3).abs().max() <= 2e-5 * max(1.0, float(y1.abs().max())), ("conv", ci, co, stride)
    for ci, co, sd in ((64, 32, 2), (32, 16, 2), (16, 8, 2), (64, 32, 1), (32, 16, 1), (16, 8, 1)):
        xx = torch.randn(2, 3, 6, 20, ci, generator=g)
        w = torch.randn(ci, co, 3, 3, 3, generator=g) * 0.1
        wp = dev(packing.pack_deconv_weights_bf16x3(w, sd), device)
        b = dev(torch.randn(64, generator=g), device)
        skip = torch.randn(2, 3 * sd, 12, 40, co, generator=g)
        for sk in (None, skip):
            y1 = cpu(ops.deconv3d_bn_relu_add(dev(xx, device), wp, b, co, sd, None if sk is None else dev(sk, device), P1))
            y3 = ops.from_split(cpu(ops.deconv3d_bn_relu_add(dev(ops.to_split(xx), device), wp, b, co, sd, None if sk is None else dev(ops.to_split(sk), device), P3)))
            assert (y1 - y3).abs().max() <= 2e-5 * max(1.0, float(y1.abs().max())), ("deconv", ci, co, sd, sk is not None)
    # whole U-Nets incl. heads (CostRegNet: 3x3x3 head on the split features; CostRegNet3D: head fused into the last layer)
    for cls, shape in ((M.CostRegNet, (1, 16, 16, 24)), (M.CostRegNet3D, (1, 4, 16, 24))):
        reg = cls(8, 8)
        reg.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(reg.state_dict()), 5))
        reg = reg.eval().to(device)
        vol = torch.randn(shape[0], *shape[1:], 8, generator=g) * 0.3
        ws, bs, prob_w, prob_b = reg.packed_all(torch.device(device) if isinstance(device, str) else device, "bf16x3")
        if reg.prob_ksize == 1:
            l1 = cpu(ops.regnet_logits(reg.kind, dev(vol, device), ws, bs, prob_w, prob_b, P1))
            l3 = cpu(ops.regnet_logits(reg.kind, dev(ops.to_split(vol), device), ws, bs, prob_w, prob_b, P3))
        else:
            l1 = cpu(ops.conv3d_logits(ops.regnet(reg.kind, dev(vol, device), ws, bs, P1), prob_w, prob_b, P1))
            l3 = cpu(ops.conv3d_logits(ops.regnet(reg.kind, dev(ops.to_split(vol), device), ws, bs, P3), prob_w, prob_b, P3))
        assert (l1 - l3).abs().max() <= 5e-5 * max(1.0, float(l1.abs().max())), cls.__name__
    # the aggregate pass and the normaliser write the format themselves
    B, V, C, D, H, W = 1, 3, 16, 8, 12, 24
    cams = synth.make_cameras(V, H * 8, W * 8, baseline=60.0, rot_deg=2.0, seed=3, batch=B)
    cams[:, :, 1, :2, :] /= 8
    feats = torch.randn(B, V, C, H, W, generator=g)
    hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.03 * torch.rand(B, D, H, W, generator=g))).contiguous()
    f, code = ops._feat(dev(feats, device))
    hom = ops.compose_homography(dev(cams, device))
    vis = dev(torch.rand(B, V - 1, H, W, generator=g), device)
    v32 = cpu(ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8)[0])
    vs = cpu(ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8, split=True)[0])
    assert torch.equal(vs.view(torch.int32), ops.to_split(v32).view(torch.int32)), "aggregate: split volume"
    part, vsum = ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8, normalise=False)
    vn = cpu(ops.volume_normalise_(part.clone(), vsum, split=True))
    assert torch.equal(vn.view(torch.int32), ops.to_split(cpu(ops.volume_normalise_(part.clone(), vsum))).view(torch.int32)), "normalise: split volume"


def case_f16_layers(device):
    """MVS_PREC_F16X2 (fp16 activations, fp16 hi + lo weights, two MFMA terms): every convolution of the U-Nets against torch's float64
    conv on the SAME fp16-rounded input - what remains is the fp32 accumulation order and the rounding of the fp16 result (2^-11)."""
    import torch.nn.functional as F
    from mvsformerplusplus_amd import _lib
    g = torch.Generator().manual_seed(41)
    P4 = _lib.PREC_F16X2
    for ci, co, stride in F16_CONVS:
        xx = (torch.randn(2, 6, 10, 20, ci, generator=g)).half()
        w = torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1
        bias = torch.randn(64, generator=g)
        wp = dev(packing.f16x2(packing.pack_conv_weights_bf16x3, w, packing.conv_chunk(ci, stride)), device)
        ref = F.relu(F.conv3d(xx.permute(0, 4, 1, 2, 3).double(), w.double(), bias[:co].double(), stride=stride, padding=1)).permute(0, 2, 3, 4, 1)
        y = cpu(ops.conv3d_bn_relu(dev(xx, device), wp, dev(bias, device), co, 3, stride, True, P4))
        assert y.dtype == torch.float16 and y.shape == ref.shape
        assert (y.double() - ref).abs().max() <= 1.5e-3 * max(1.0, float(ref.abs().max())), ("conv", ci, co, stride, float((y.double() - ref).abs().max()))
    for ci, co, sd in ((64, 32, 2), (32, 16, 2), (16, 8, 2), (64, 32, 1), (32, 16, 1), (16, 8, 1)):
        xx = torch.randn(2, 3, 6, 20, ci, generator=g).half()
        w = torch.randn(ci, co, 3, 3, 3, generator=g) * 0.1
        bias = torch.randn(64, generator=g)
        wp = dev(packing.f16x2(packing.pack_deconv_weights_bf16x3, w, sd), device)
        skip = torch.randn(2, 3 * sd, 12, 40, co, generator=g).half()
        for sk in (None, skip):
            ref = F.relu(F.conv_transpose3d(xx.permute(0, 4, 1, 2, 3).double(), w.double(), bias[:co].double(), stride=(sd, 2, 2), padding=1,
                                            output_padding=(sd - 1, 1, 1))).permute(0, 2, 3, 4, 1)
            if sk is not None:
                ref = ref + sk.double()
            y = cpu(ops.deconv3d_bn_relu_add(dev(xx, device), wp, dev(bias, device), co, sd, None if sk is None else dev(sk, device), P4))
            assert y.dtype == torch.float16
            assert (y.double() - ref).abs().max() <= 1.5e-3 * max(1.0, float(ref.abs().max())), ("deconv", ci, co, sd, sk is not None)
    # Cin = 8 layers (persistent kernels) and the two heads
    for stride in ((2, 2, 2), (1, 2, 2)):
        xx = torch.randn(2, 6, 10, 24, 8, generator=g).half()
        w = torch.randn(16, 8, 3, 3, 3, generator=g) * 0.1
        bias = torch.randn(64, generator=g)
        wp = dev(packing.f16x2(packing.pack_conv_weights_bf16x3, w, packing.conv_chunk(8, stride)), device)
        ref = F.relu(F.conv3d(xx.permute(0, 4, 1, 2, 3).double(), w.double(), bias[:16].double(), stride=stride, padding=1)).permute(0, 2, 3, 4, 1)
        y = cpu(ops.conv3d_bn_relu(dev(xx, device), wp, dev(bias, device), 16, 3, stride, True, P4))
        assert (y.double() - ref).abs().max() <= 1.5e-3 * max(1.0, float(ref.abs().max())), ("conv 8->16", stride)


def case_f16_saturation(device):
    """fp16 stores saturate instead of overflowing: a layer whose outputs exceed 65504 writes +-65504 (finite), and the aggregate pass
    clamps the cost volume it writes (features scaled until the correlations leave the fp16 range)."""
    import warnings
    from mvsformerplusplus_amd import _lib, cost_volume
    g = torch.Generator().manual_seed(3)
    ops.f16_saturation_count(reset=True)
    # a layer inside the range leaves the counter alone
    xs = torch.rand(1, 4, 8, 16, 16, generator=g).half()
    w = torch.ones(16, 16, 3, 3, 3) * 2.0
    wp = dev(packing.f16x2(packing.pack_conv_weights_bf16x3, w, packing.conv_chunk(16, (1, 1, 1))), device)
    ops.conv3d_bn_relu(dev(xs, device), wp, dev(torch.zeros(64), device), 16, 3, (1, 1, 1), True, _lib.PREC_F16X2)
    assert ops.f16_saturation_count() == 0, "no value left the fp16 range, the counter must stay 0"
    xx = (torch.rand(1, 4, 8, 16, 16, generator=g) * 200.0 + 100.0).half()                  # every output ~ 27 * 16 * 2 * 200 >> 65504
    y = cpu(ops.conv3d_bn_relu(dev(xx, device), wp, dev(torch.zeros(64), device), 16, 3, (1, 1, 1), True, _lib.PREC_F16X2))
    assert torch.isfinite(y).all() and float(y.max()) == 65504.0
    n_conv = ops.f16_saturation_count()
    assert n_conv > 0, "the clamped stores must be counted (mvs_f16_saturation_count)"
    with warnings.catch_warnings(record=True) as rec:                                       # ... and surfaced as a warning, which also clears the counter
        warnings.simplefilter("always")
        assert cost_volume.check_f16_saturation(device if device != "cpu" else None) == n_conv
    assert any("conv_precision='bf16x3'" in str(r.message) for r in rec)
    assert ops.f16_saturation_count() == 0
    B, V, C, D, H, W = 1, 3, 8, 4, 8, 32
    cams = synth.make_cameras(V, H * 8, W * 8, baseline=30.0, seed=1, batch=B)
    cams[:, :, 1, :2, :] /= 8
    feats = torch.randn(B, V, C, H, W, generator=g) * 400.0
    hyp = (torch.linspace(800, 500, D)[None, :, None, None] * torch.ones(B, D, H, W)).contiguous()
    f, code = ops._feat(dev(feats, device))
    hom = ops.compose_homography(dev(cams, device))
    vis = dev(torch.ones(B, V - 1, H, W), device)
    v32 = cpu(ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8)[0])
    v16 = cpu(ops.warp_corr_aggregate(f, code, hom, dev(hyp, device), vis, 8, f16=True)[0])
    assert float(v32.abs().max()) > 65504.0, "the case must leave the fp16 range"
    assert v16.dtype == torch.float16 and torch.isfinite(v16).all()
    # the fp16 volume's gather stages the SOURCE features as fp16 (MVS_GATHER_F16): same numbers as the fp32 gather of once-rounded sources
    fr = feats.clone()
    fr[:, 1:] = fr[:, 1:].half().float()
    v32r = cpu(ops.warp_corr_aggregate(dev(fr, device), code, hom, dev(hyp, device), vis, 8)[0])
    want = v32r.clamp(-65504.0, 65504.0).half().float()
    assert ((v16.float() - want).abs() <= 1e-3 * want.abs() + 1e-3).all() and float(v16.float().abs().max()) == 65504.0      # 1 ulp: fma contraction differs
    n_agg = ops.f16_saturation_count(reset=True)
    assert n_agg > 0, "the aggregate pass's clamped cost-volume writes must be counted"
    assert torch.equal(cpu(ops.volume_to_f16(dev(v32, device))), v32.clamp(-65504.0, 65504.0).half())
    assert ops.f16_saturation_count(reset=True) > 0, "mvs_volume_to_f16's clamped writes must be counted"


def case_f16_cascade(device):
    """conv_precision = "f16x2" end to end (fp16 cost volume from the aggregate pass, fp16 U-Net tensors, both heads) against the
    reference-generated cascade golden F4 and, per stage, the golden stage outputs: the north-star bar is 1e-3 relative L1 on depth;
    measured ~5e-5 on plain inputs (scripts/study_activation_precision.py predicts 5.5e-5 plain, 4.2e-4 on the x30 stress set)."""
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    fx = load_golden("f4_cascade.npz")
    args = {"base_ch": [8] * 4, "depth_type": ["ce"] * 4, "ndepths": [32, 16, 8, 4], "depth_interals_ratio": [4.0, 2.67, 1.5, 1.0], "inverse_depth": True,
            "conv_precision": "f16x2"}
    head = CascadeDepthHead(args)
    for s in range(4):
        head.fusions[s].load_state_dict(golden_weights(fx, "w%d." % (s + 1)), strict=True)
        assert head.fusions[s].conv_precision == "f16x2"
    head = head.eval().to(device)
    feats = {"stage%d" % s: dev(fx["features%d" % s], device) for s in range(1, 5)}
    projs = {"stage%d" % s: dev(fx["proj%d" % s], device) for s in range(1, 5)}
    with torch.no_grad():
        out = head(feats, projs, dev(fx["depth_values"], device))
    r = rel_l1(cpu(out["refined_depth"]), fx["refined_depth"])
    assert r <= 3e-4, "f16x2 cascade: refined depth rel-L1 %g vs the reference's golden" % r
    # the A/B switch fuse_prob_head = False (standalone fp32 head on the fp16 features) gives the same stage result up to the
    # fp16 rounding of the 8-channel features the fused head never stores
    for st in head.fusions:
        st.fuse_prob_head = False
    with torch.no_grad():
        out2 = head(feats, projs, dev(fx["depth_values"], device))
    assert rel_l1(cpu(out2["refined_depth"]), cpu(out["refined_depth"])) <= 3e-4
    return r


F16_CONVS = ((16, 16, (1, 1, 1)), (32, 32, (1, 1, 1)), (64, 64, (1, 1, 1)), (16, 32, (2, 2, 2)), (16, 32, (1, 2, 2)), (32, 64, (2, 2, 2)), (32, 64, (1, 2, 2)))


def case_slab_exchange_kernels(device):
    """mvs_slab_pack / mvs_slab_reduce (the slab exchange of the view-sharded latency mode) against torch slicing: message j = rows
    [r0_j, r1_j) of the partial volume followed by the same rows of the partial visibility sum; the reduction adds the own slice and
    the received messages in rank order (bit-identical to the sequential sum)."""
    for G in (8, 4, 3):                                              # 8 groups (every shipped config) and the run-time G of ABI v10
        _slab_exchange(device, G)


def _slab_exchange(device, G):
    g = torch.Generator().manual_seed(9)
    B, D, H, W, R = 2, 3, 24, 16, 4
    vol = torch.randn(B, D, H, W, G, generator=g)
    vsum = torch.rand(B, H, W, generator=g)
    rows = [(0, 10), (4, 18), (12, 24), (5, 5)]                      # rank 3 owns nothing
    sends = [None if r1 <= r0 or j == 1 else torch.full((B * D * (r1 - r0) * W * G + B * (r1 - r0) * W,), float("nan")) for j, (r0, r1) in enumerate(rows)]
    dsends = [None if t is None else dev(t, device) for t in sends]
    ops.slab_pack(dev(vol, device), dev(vsum, device), dsends, rows)
    for j, (r0, r1) in enumerate(rows):
        if dsends[j] is None:
            continue
        want = torch.cat([vol[:, :, r0:r1].reshape(-1), vsum[:, r0:r1].reshape(-1)])
        assert torch.equal(cpu(dsends[j]), want), j
    my, (r0, r1) = 1, rows[1]
    n = B * D * (r1 - r0) * W * G + B * (r1 - r0) * W
    recvs = [None if j in (my, 3) else torch.randn(n, generator=g) for j in range(R)]
    out = cpu(ops.slab_reduce(dev(vol, device), dev(vsum, device), [None if t is None else dev(t, device) for t in recvs], my,
                              dev(torch.empty(n), device), r0, r1))
    own = torch.cat([vol[:, :, r0:r1].reshape(-1), vsum[:, r0:r1].reshape(-1)])
    want = torch.zeros(n)
    for j in range(R):
        want = want + (own if j == my else (recvs[j] if recvs[j] is not None else 0.0))
    assert torch.equal(out, want)


# ---------------------------------------------------------------- a16 cascade
def case_cascade_golden(device, prec=None):
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    fx = load_golden("f4_cascade.npz")
    args = with_prec(dict(ARGS, ndepths=[32, 16, 8, 4], depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], inverse_depth=True), prec)
    head = CascadeDepthHead(args)
    for s in range(4):
        head.fusions[s].load_state_dict(golden_weights(fx, "w%d." % (s + 1)), strict=True)
    head = head.eval().to(device)
    feats = {"stage%d" % s: dev(fx["features%d" % s], device) for s in range(1, 5)}
    projs = {"stage%d" % s: dev(fx["proj%d" % s], device) for s in range(1, 5)}
    with torch.no_grad():
        out = head(feats, projs, dev(fx["depth_values"], device), tmp=[5.0, 5.0, 5.0, 1.0])
    for s in range(1, 5):
        st = out["stage%d" % s]
        assert rel_l1(cpu(st["depth_values"]), fx["hyp%d" % s]) <= tol(prec, 2e-5, 3e-4), s
        assert rel_l1(cpu(st["depth"]), fx["depth%d" % s]) <= tol(prec, 5e-5, 3e-4), "stage %d depth vs reference (bar 1e-3)" % s
        assert (cpu(st["photometric_confidence"]) - fx["conf%d" % s]).abs().max() <= tol(prec, 2e-3, 2e-2)
    assert rel_l1(cpu(out["refined_depth"]), fx["refined_depth"]) <= tol(prec, 5e-5, 3e-4)
    assert (cpu(out["photometric_confidence"]) - fx["photometric_confidence"]).abs().max() <= tol(prec, 1e-3, 2e-2)
    assert torch.equal(out["refined_depth"], out["stage4"]["depth"])
    # hand-off layout: the same cascade fed octet-tiled features returns the same depth
    with torch.no_grad():
        out_t = head({k: ops.pack_features(v) for k, v in feats.items()}, projs, dev(fx["depth_values"], device), tmp=[5.0, 5.0, 5.0, 1.0])
    assert rel_l1(cpu(out_t["refined_depth"]), cpu(out["refined_depth"])) <= 1e-6


# ---------------------------------------------------------------- larger sizes (GPU only)
def _seeded_head(device, seed=11, peaky=False, conv_precision=None):
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    args = dict(ARGS, ndepths=[32, 16, 8, 4], depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], inverse_depth=True)
    if conv_precision:
        args["conv_precision"] = conv_precision
    head = CascadeDepthHead(args)
    for i, st in enumerate(head.fusions):
        sd = synth.seeded_state_dict(synth.state_dict_manifest(st.state_dict()), seed + i)
        if peaky:
            sd["cost_reg.prob.weight"] = sd["cost_reg.prob.weight"] * 30.0      # SURVEY.md section 8d "peaky" set
        st.load_state_dict(sd, strict=True)
    return head.eval().to(device), args


def case_cascade_vs_oracle(device, H, W, V, peaky=False, conv_precision=None, **inputs):
    """Any precision policy / format (None = the product default): the same 1e-3 depth bar; the confidence (max softmax probability - not part of
    the north-star bar) is allowed 1e-2 mean absolute error on the x30-logits stress set (bf16x3: 1e-3)."""
    head, args = _seeded_head(device, peaky=peaky, conv_precision=conv_precision)
    feats, projs, dv = synth.make_cascade_inputs(H, W, V, seed=2, rot_deg=1.0, **inputs)
    sds = [{k: v.cpu() for k, v in st.state_dict().items()} for st in head.fusions]
    with torch.no_grad():
        ref = O.cascade_forward(feats, projs, dv, sds, ndepths=args["ndepths"], depth_interals_ratio=args["depth_interals_ratio"],
                                base_ch=args["base_ch"])
        out = head({k: dev(v, device) for k, v in feats.items()}, {k: dev(v, device) for k, v in projs.items()}, dev(dv, device))
    for s in range(1, 5):
        r = rel_l1(cpu(out["stage%d" % s]["depth"]), ref["stage%d" % s]["depth"])
        assert r <= 1e-3, "stage %d depth rel-L1 %g > 1e-3" % (s, r)
    r = rel_l1(cpu(out["refined_depth"]), ref["refined_depth"])
    assert r <= 1e-3, "refined depth rel-L1 %g > 1e-3 (north-star bar)" % r
    # confidence = max softmax probability: with x30 logits a near-tie between two planes turns a 1e-5 logit difference
    # into a visible probability difference at isolated pixels, so the check is on the mean (the max is only reported)
    dconf = (cpu(out["photometric_confidence"]) - ref["photometric_confidence"]).abs()
    assert float(dconf.mean()) <= tol(conv_precision, 1e-3, 1e-2), "confidence mean abs error %g" % float(dconf.mean())
    if conv_precision is None and feats["stage4"].dtype in (torch.float32, torch.float16):
        # the product default fed with the producer-side emitter's hand-off for the fine stages: stages 3-4 as fp16 octet tiles -
        # the gather reads its taps straight from the tiles where C = 8 (gather_lds.h, the direct form (`gl_direct_v`)): the same bar against the same oracle
        with torch.no_grad():
            ft = {k: (ops.pack_features(dev(v, device), torch.float16) if k in ("stage3", "stage4") else dev(v, device)) for k, v in feats.items()}
            out_t = head(ft, {k: dev(v, device) for k, v in projs.items()}, dev(dv, device))
        rt = rel_l1(cpu(out_t["refined_depth"]), ref["refined_depth"])
        assert rt <= 1e-3, "fp16-tile hand-off: refined depth rel-L1 %g > 1e-3" % rt
        assert rel_l1(cpu(out_t["refined_depth"]), cpu(out["refined_depth"])) <= 1e-4, "fp16-tile hand-off vs planar features"
    return r


def case_cascade_vs_oracle_finite(device, H, W, V, conv_precision=None, **inputs):
    """Cascade vs the oracle on a range that makes the reference ITSELF degenerate for part of the image: with a Tanks-and-Temples-
    like 0.5 .. 10 range the stage-2 inverse-depth window 1/depth -/+ 2.67*itv (module.py:712-716) crosses zero for far pixels, the
    hypotheses jump through +-infinity there and neither implementation means anything.  Parity is asserted on every pixel whose
    hypotheses are finite and positive at all four stages IN THE REFERENCE (at least a fifth of the image); the rest only has to be
    reproduced as non-crashing."""
    import torch.nn.functional as F
    head, args = _seeded_head(device, conv_precision=conv_precision)
    feats, projs, dv = synth.make_cascade_inputs(H, W, V, seed=2, rot_deg=1.0, **inputs)
    sds = [{k: v.cpu() for k, v in st.state_dict().items()} for st in head.fusions]
    with torch.no_grad():
        ref = O.cascade_forward({k: v.float() for k, v in feats.items()}, projs, dv, sds, ndepths=args["ndepths"],
                                depth_interals_ratio=args["depth_interals_ratio"], base_ch=args["base_ch"])
        out = head({k: dev(v, device) for k, v in feats.items()}, {k: dev(v, device) for k, v in projs.items()}, dev(dv, device))
    ok = torch.ones(1, H, W, dtype=torch.bool)
    lo, hi = float(dv.min()) * 0.25, float(dv.max()) * 4.0
    for s in range(1, 5):
        hyp = ref["stage%d" % s]["depth_values"]
        good = (torch.isfinite(hyp) & (hyp > lo) & (hyp < hi)).all(1)
        good = good & torch.isfinite(ref["stage%d" % s]["depth"])
        ok = ok & F.interpolate(good[:, None].float(), size=(H, W), mode="nearest")[:, 0].bool()
    frac = float(ok.float().mean())
    assert frac >= 0.2, "only %.0f %% of the pixels keep finite hypotheses in the reference" % (100 * frac)
    d, r = cpu(out["refined_depth"]), ref["refined_depth"]
    err = ((d - r).abs() / r.abs())[ok]
    rel = float(err.mean())
    if conv_precision in _lib.F16_FORMATS:
        # ONE fp16 format on every stage (opt-in since round 5).  The pixels next to the degenerate ones are ill-conditioned (hypotheses of
        # 40 scene units beside a true depth of 8: a 1e-4 probability difference moves the regressed depth by 5e-4): the coarse stages'
        # fp16 noise (6e-5 on sane ranges) becomes 3-5e-3 on the mean here (median 8e-4).  Asserted as measured, documented in DESIGN.md
        # section 5 and warned about at run time (cost_volume.check_hypothesis_conditioning) - which is why these formats are not the default.
        import warnings
        from mvsformerplusplus_amd import cost_volume
        assert float(err.median()) <= 1.5e-3 and rel <= 1e-2, "fp16 format on the degenerate range: median %g mean %g" % (float(err.median()), rel)
        cost_volume._HYP_WARNED = False
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            bad = max(cost_volume.check_hypothesis_conditioning(out["stage%d" % s]["depth_values"]) for s in range(1, 5))
        assert bad > 0 and any("conv_precision='bf16x3'" in str(w.message) for w in rec), "the degenerate schedule must be reported"
    else:
        # the product default ("stagemix": fp32-equivalent coarse stages) and "bf16x3": the north-star bar itself
        assert rel <= 1e-3, "refined depth rel-L1 %g on the %.0f %% of pixels where the reference is finite" % (rel, 100 * frac)
    return rel, frac


def case_cascade_fullsize_properties(device, H=1152, W=1536, V=5, conv_precision=None, **inputs):
    head, args = _seeded_head(device, conv_precision=conv_precision)
    feats, projs, dv = synth.make_cascade_inputs(H, W, V, seed=0, device=device, **inputs)
    with torch.no_grad():
        a = head(feats, projs, dv)
        b = head(feats, projs, dv)
        assert torch.equal(a["refined_depth"], b["refined_depth"]), "the path must be deterministic run to run"
        d = a["refined_depth"]
        assert torch.isfinite(d).all() and torch.isfinite(a["photometric_confidence"]).all()
        assert float(d.min()) >= float(dv.min()) * 0.9 and float(d.max()) <= float(dv.max()) * 1.1
        c = a["photometric_confidence"]
        assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0 + 1e-5
        for s in range(1, 5):
            pv = a["stage%d" % s]["prob_volume"]
            assert (pv.sum(1) - 1).abs().max() <= 1e-4                      # softmax over depth sums to one
            hyp = a["stage%d" % s]["depth_values"]
            assert (hyp[:, :-1] >= hyp[:, 1:]).all()                         # inverse-depth hypotheses run far -> near
        # permuting the source views permutes nothing but the summation order of the aggregation
        perm = [0] + list(range(V - 1, 0, -1))
        fp = {k: v[:, perm].contiguous() for k, v in feats.items()}
        pp = {k: v[:, perm].contiguous() for k, v in projs.items()}
        c2 = head(fp, pp, dv)
        r = rel_l1(c2["refined_depth"].cpu(), d.cpu())
        # fp16 formats: the fp32 sum over views moves by an ulp with the order, which flips the fp16 rounding of isolated cost-volume voxels
        # (2^-11 relative each): the result moves by a fraction of the format's own distance from the oracle (cfg2 3e-5, cfg4 / cfg5 2.6e-4)
        assert r <= tol(conv_precision, 1e-4, 6e-4), "view-order invariance violated: %g" % r


# ---------------------------------------------------------------- BASELINE.json configs
# configs[0] is the reference's own CPU-runnable case; [2]..[4] differ from the bench workload in view count, image size,
# hypothesis range and feature dtype.  Each is checked against the oracle at a size it finishes in seconds and - for the
# multi-stage ones - through size-independent properties at the full size.
BASELINE_CFGS = {
    "cfg3": dict(full=(1152, 1536), small=(256, 320), V=10, inputs={}),
    # Tanks-and-Temples-like range 0.5 .. 3.0 scene units.  (A 0.5 .. 10 range makes the stage-2 inverse-depth window
    # inv(depth) -/+ 2.67 * itv cross zero for far pixels, module.py:712-716: hypotheses jump through +-infinity there and
    # reference and replacement agree only in being meaningless, so that range cannot carry a parity check.)
    "cfg4": dict(full=(1088, 1920), small=(256, 448), V=11,
                 inputs=dict(numdepth=256, depth_min=0.5, depth_interval=2.5 / 255.0, baseline=0.03)),
    "cfg5": dict(full=(1536, 2048), small=(256, 384), V=11,
                 inputs=dict(numdepth=384, depth_min=0.5, depth_interval=2.5 / 383.0, baseline=0.03, feat_dtype=torch.float16)),
}


def case_baseline_cfg1(device, prec=None, final_stage=False):
    """configs[0] / Track S: one StageNet, stage_idx 3 (C = G = 8), 640x512, V = 3, D = 48 fronto-parallel hypotheses
    linspace(425, 935) -> CostRegNet (D > 8) with the 3x3x3 head.  final_stage: args["final_stage"] = True (round 6) - the default policy
    then runs this stand-alone stage in the fine stages' fp16 format instead of the exact coarse-stage one; same 1e-3 bar."""
    from mvsformerplusplus_amd.cost_volume import StageNet
    H, W, V, D = 512, 640, 3, 48
    st = StageNet(dict(with_prec(ARGS, prec), final_stage=True) if final_stage else with_prec(ARGS, prec), D, 3)
    assert st.precision_policy == eff(prec)
    if final_stage and prec is None:
        assert (st.conv_precision, st.gather_precision) == ("f16mix", "f16")
    st.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(st.state_dict()), 5), strict=True)
    st = st.eval().to(device)
    cams = synth.make_cameras(V, H, W, baseline=20.0, seed=0)
    proj = synth.stage_proj_matrices(cams, 1)["stage1"]
    feats = synth.make_features(proj, 8, H, W, dmin=500.0, dmax=860.0, seed=0)
    hyp = torch.linspace(425.0, 935.0, D).view(1, D, 1, 1).repeat(1, 1, H, W)
    sd = {k: v.cpu() for k, v in st.state_dict().items()}
    with torch.no_grad():
        ref = O.stage_forward(feats, proj, hyp, 1.0, sd, G=8)
        out = st(dev(feats, device), dev(proj, device), dev(hyp, device), tmp=1.0)
    r = rel_l1(cpu(out["depth"]), ref["depth"])
    assert r <= 1e-3, "cfg1 depth rel-L1 %g" % r
    pe = float((cpu(out["prob_volume"]) - ref["prob_volume"]).abs().max())
    assert pe <= tol(prec, 2e-3, 2e-2), pe
    return r, pe


def case_track_s_d192(device, H=1152, W=1536, D=192, V=3):
    """SURVEY section 8d Track S, literal D: ONE StageNet (stage_idx 3: C = G = 8) at 1152 x 1536 with 192 hypotheses - a 340-Mvoxel volume,
    10.9 GB in the coarse-stage (split-bf16) format, which rounds 1-4 refused (32-bit byte offsets over a whole batch item; round 5 re-bases
    the staging descriptor per tile, conv_bf16x3_kernels.hip bf_make_rsrc_z).  The oracle cannot run this size; the check is a CROP
    cross-check: the same stage on a 256 x 512 window of the same inputs (principal point shifted by the window origin; every tensor of that
    run is far below 2 GB) must reproduce the full run on the window's interior - the pixels whose U-Net receptive field (+-40) and
    source taps (disparity <= 131 px at depth 425) stay inside the window.  A wrong plane / row offset anywhere beyond 2 GB shows up here.
    Plus the size-independent properties: finite outputs, probabilities sum to 1, depth inside the hypothesis range."""
    from mvsformerplusplus_amd.cost_volume import StageNet
    st = StageNet(dict(ARGS), D, 3)
    assert st.conv_precision == "bf16x3"                                       # D > model_th: the policy's exact form
    st.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(st.state_dict()), 5), strict=True)
    st = st.eval().to(device)
    cams = synth.make_cameras(V, H, W, baseline=20.0, seed=0)
    proj = synth.stage_proj_matrices(cams, 1)["stage1"]
    g = torch.Generator().manual_seed(12)
    feats = torch.randn(1, V, 8, H, W, generator=g)
    dvals = torch.linspace(425.0, 935.0, D)
    with torch.no_grad():
        hyp = dev(dvals.view(1, D, 1, 1), device).expand(1, D, H, W).contiguous()
        out = st(dev(feats, device), dev(proj, device), hyp, tmp=1.0)
        depth, conf = cpu(out["depth"]), cpu(out["photometric_confidence"])
        assert torch.isfinite(depth).all() and torch.isfinite(conf).all()
        assert float(depth.min()) >= 425.0 - 1e-2 and float(depth.max()) <= 935.0 + 1e-2
        psum = out["prob_volume"].sum(1)
        assert float((psum - 1.0).abs().max()) <= 1e-4, "softmax over 192 planes"
        del psum
        y0, x0, hc, wc = 448, 512, 256, 512                                     # window origin multiples of 64: same tile phases as the full run
        pc = proj.clone()
        pc[:, :, 1, 0, 2] -= x0
        pc[:, :, 1, 1, 2] -= y0
        fc = feats[..., y0:y0 + hc, x0:x0 + wc].contiguous()
        hc_ = dev(dvals.view(1, D, 1, 1), device).expand(1, D, hc, wc).contiguous()
        full_pre = cpu(out["prob_volume_pre"][..., y0:y0 + hc, x0:x0 + wc])
        del out
        oc = st(dev(fc, device), dev(pc, device), hc_, tmp=1.0)
    my, mx = 48, 131 + 48
    a = depth[:, y0 + my:y0 + hc - my, x0 + mx:x0 + wc - mx]
    b = cpu(oc["depth"])[:, my:hc - my, mx:wc - mx]
    r = rel_l1(b, a)
    assert r <= 2e-5, "full-size D = 192 run vs the same stage on a window: depth rel-L1 %g" % r
    pa, pb = full_pre[:, :, my:hc - my, mx:wc - mx], cpu(oc["prob_volume_pre"])[:, :, my:hc - my, mx:wc - mx]
    assert (pa - pb).abs().max() <= 2e-4 * max(1.0, float(pa.abs().max())), "logits, every one of the 192 planes"
    return r


def case_baseline_cfg_small(device, name, conv_precision=None):
    c = BASELINE_CFGS[name]
    return case_cascade_vs_oracle(device, c["small"][0], c["small"][1], c["V"], conv_precision=conv_precision, **c["inputs"])


def case_baseline_cfg_wide_range(device, name, prec=None):
    """cfg4 / cfg5 on SURVEY section 8d's literal 0.5 .. 10 range (the cases above use 0.5 .. 3.0)."""
    c = BASELINE_CFGS[name]
    inputs = dict(c["inputs"])
    nd = inputs["numdepth"]
    inputs.update(depth_min=0.5, depth_interval=9.5 / (nd - 1))
    return case_cascade_vs_oracle_finite(device, c["small"][0], c["small"][1], c["V"], conv_precision=prec, **inputs)


def case_cfg2_fullsize_vs_oracle(device, conv_precision=None):
    """BASELINE configs[1] at its FULL size (1152x1536, V = 5, ndepths 32/16/8/4) against the oracle: the north-star bar itself."""
    return case_cascade_vs_oracle(device, 1152, 1536, 5, conv_precision=conv_precision)


def case_baseline_cfg_full(device, name, prec=None):
    c = BASELINE_CFGS[name]
    case_cascade_fullsize_properties(device, c["full"][0], c["full"][1], c["V"], conv_precision=prec, **c["inputs"])


# ---------------------------------------------------------------- stage-1 transformer regulariser
def _tcfg(fx):
    import json
    return json.loads(fx["cfg"])


def case_transformer_golden(device, attention_precision=None):
    """PureTransformerCostReg alone + get_position_3d against fixture f7 (generated from the reference).  attention_precision None = the
    module default ("attn16": one 16-bit term per attention operand like the reference's flash-attn path - fp16 q / k, bf16 p / v): logits within 2e-3;
    "bf16x3" = the fp32-equivalent attention: 2e-4."""
    from mvsformerplusplus_amd import PureTransformerCostReg, get_position_3d
    fx = load_golden("f7_transformer.npz")
    cfg = _tcfg(fx)
    if attention_precision:
        cfg["attention_precision"] = attention_precision
    net = PureTransformerCostReg(8, **cfg)
    assert net.attention_precision == (attention_precision or "attn16")
    net.load_state_dict(golden_weights(fx), strict=True)
    net = net.eval().to(device)
    dv = fx["depth_values"]
    with torch.no_grad():
        pos, hmin, hmax, wmin, wmax = get_position_3d(1, 16, 24, dev(fx["K"], device), dev(fx["hyp"], device), float(dv.min()), float(dv.max()),
                                                      None, None, None, None)
        assert (cpu(pos) - fx["position3d"]).abs().max() <= 1e-5
        assert (torch.stack([cpu(hmin), cpu(hmax), cpu(wmin), cpu(wmax)]) - fx["pe_range"]).abs().max() <= 1e-3
        pos2 = get_position_3d(1, 16, 24, dev(fx["K"], device), dev(fx["hyp"], device), dv.min(), dv.max(), hmin, hmax, wmin, wmax)[0]
        assert torch.equal(cpu(pos2), cpu(pos)), "reusing the measured range must reproduce the positions"
        y = cpu(net(dev(fx["x"], device), dev(fx["position3d"], device)))
        y0 = cpu(net(dev(fx["x"], device), None))
    tol = (2e-4 if net.attention_precision == "bf16x3" else 2e-3) * max(1.0, float(fx["y"].abs().max()))
    assert y.shape == fx["y"].shape
    assert (y - fx["y"]).abs().max() <= tol, float((y - fx["y"]).abs().max())
    assert (y0 - fx["y_nope"]).abs().max() <= tol, float((y0 - fx["y_nope"]).abs().max())
    return float((y - fx["y"]).abs().max())


def case_stage_transformer_golden(device, attention_precision=None):
    from mvsformerplusplus_amd.cost_volume import StageNet
    fx = load_golden("f8_stage_transformer.npz")
    tc = _tcfg(fx)
    if attention_precision:
        tc["attention_precision"] = attention_precision
    args = dict(ARGS, cost_reg_type=["PureTransformerCostReg", "Normal", "Normal", "Normal"], transformer_config=[tc])
    st = StageNet(args, 32, 0)
    st.load_state_dict(golden_weights(fx), strict=True)
    st = st.eval().to(device)
    with torch.no_grad():
        out = st(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), tmp=5.0, position3d=dev(fx["position3d"], device))
    exact = st.cost_reg.attention_precision == "bf16x3"
    assert (cpu(out["prob_volume_pre"]) - fx["prob_volume_pre"]).abs().max() <= (1e-3 if exact else 3e-3)
    assert (cpu(out["prob_volume"]) - fx["prob_volume"]).abs().max() <= (1e-4 if exact else 5e-4)
    assert rel_l1(cpu(out["depth"]), fx["depth"]) <= (1e-5 if exact else 5e-5)


def case_cascade_shipped_golden(device, conv_precision=None, attention_precision=None):
    """Shipped regulariser mix (stage-1 transformer + Frustoconical PE, CostRegNet / CostRegNet3D after it) on the f4 inputs.
    conv_precision "f16x2" (round 3's default, opt-in): the three U-Net stages and all four visibility CNNs in the fp16 form; 3e-4 instead of 1e-4.
    attention_precision None = the module default ("attn16")."""
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    fx, f4 = load_golden("f9_cascade_shipped.npz"), load_golden("f4_cascade.npz")
    tc = _tcfg(fx)
    if attention_precision:
        tc["attention_precision"] = attention_precision
    args = dict(ARGS, ndepths=[32, 16, 8, 4], depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], inverse_depth=True, use_pe3d=True,
                cost_reg_type=["PureTransformerCostReg", "Normal", "Normal", "Normal"], transformer_config=[tc])
    args = with_prec(args, conv_precision)
    exact = not is_f16(conv_precision) and attention_precision == "bf16x3"
    dt = 1e-4 if exact else 3e-4
    head = CascadeDepthHead(args)
    for s, stn in enumerate(head.fusions):
        stn.load_state_dict(golden_weights(fx, "w%d." % (s + 1)), strict=True)
    head = head.eval().to(device)
    assert head.fusions[1].precision_policy == eff(conv_precision) and head.fusions[0].cost_reg.attention_precision == (attention_precision or "attn16")
    feats = {"stage%d" % s: dev(f4["features%d" % s], device) for s in range(1, 5)}
    projs = {"stage%d" % s: dev(f4["proj%d" % s], device) for s in range(1, 5)}
    with torch.no_grad():
        out = head(feats, projs, dev(f4["depth_values"], device))
    for s in range(1, 5):
        assert rel_l1(cpu(out["stage%d" % s]["depth"]), fx["depth%d" % s]) <= dt, s
    assert rel_l1(cpu(out["refined_depth"]), fx["refined_depth"]) <= dt
    assert (cpu(out["photometric_confidence"]) - fx["photometric_confidence"]).abs().max() <= (1e-3 if exact else 2e-2)


def case_attention_stress(device, n=200, gain=2.0, bf16p=False, mode=None):
    """Flash attention alone against float64 softmax attention: token count not a multiple of the key block (masked tail),
    scores large and growing along the key axis so that the lazily raised running maximum must rescale in later blocks.
    mode: "attn16" (the module default: fp16 q / k, bf16 p / v, csrc/attention_f16_kernels.hip), "bf16p", or None = "bf16x3"."""
    from mvsformerplusplus_amd import _lib, ops, packing
    mode = mode or ("bf16p" if bf16p else "bf16x3")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, n, 64, generator=g)
    x = x * torch.linspace(0.2, 1.0, n).reshape(1, n, 1) * gain         # later keys carry larger scores
    w = torch.randn(192, 64, generator=g) * 0.125
    scale = 0.25 * 1.07
    code = {"attn16": _lib.PREC_ATTN16, "bf16p": _lib.PREC_BF16P, "bf16x3": None}[mode]
    got = cpu(ops.tr_attention(dev(x, device), dev(packing.pack_linear_bf16x3(w), device), 4, scale, _lib.PREC_BF16X3, code))
    qkv = (x.double() @ w.double().t()).reshape(2, n, 3, 4, 16).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) * scale, -1) @ qkv[2]
    ref = att.transpose(1, 2).reshape(2, n, 64).float()
    smax = float((qkv[0] @ qkv[1].transpose(-2, -1)).abs().max() * scale * 1.4427)
    assert smax > 3 * 8.0, "the case must exceed the lazy threshold"
    # the split-bf16 score product carries ~2^-17 relative error, i.e. an ABSOLUTE error proportional to the score in
    # the exponent: measured relative output error ~ 5e-7 * max|score in log2 units| (1.6e-4 at 308, 2.8e-5 at 34)
    err = float((got - ref).abs().max())
    # bf16 probabilities (MVS_PREC_BF16P): 2^-9 relative rounding per probability, unbiased.
    # MVS_PREC_ATTN16: fp16 q and k carry 2^-12 relative rounding each, i.e. an absolute score error ~ 2^-12 |score| / 2 in the exponent
    # (this stress set reaches scores of several hundred in log2 units - far beyond the O(10) of the real network, where the error is
    # 1e-3 of the logits, scripts/study_attention_precision.py), plus 2^-9 per probability and value (bf16)
    tol = {"bf16x3": 1e-4, "bf16p": 4e-3, "attn16": 6e-3 + 1.5e-4 * smax}[mode]
    assert err <= tol * max(1.0, float(ref.abs().max())), (err, smax)
    return err


def case_attention_overflow(device, n=300):
    """MVS_PREC_ATTN16's SAFE path: one late key whose scores sit ~800 binades above (or below) everything before it - the fast path's
    probabilities overflow fp32 inside a block, the work-group must notice and redo its queries with the per-step online softmax.
    The operands are built so that the kernel's 16-bit copies are known exactly (q = k = v = x through identity projections, x on a
    2^-6 grid) and no row has a near-tie with the spike (every token carries +-1 along the spike's direction), so the float64 reference
    on those operands isolates the kernel: what remains is the bf16 rounding of the probabilities (2^-9 each)."""
    from mvsformerplusplus_amd import _lib, ops, packing
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1, n, 64, generator=g) * 64).round() / 64
    sign = torch.where(torch.rand(1, n, generator=g) < 0.5, -1.0, 1.0)
    t = 200
    for h in range(4):
        x[:, :, 16 * h] = sign
        x[:, t, 16 * h] = 2048.0                                       # the spike key (and value, and query) of every head
    w = torch.cat([torch.eye(64)] * 3, 0)                               # q = k = v = x
    scale = 0.27
    got = cpu(ops.tr_attention(dev(x, device), dev(packing.pack_linear_bf16x3(w), device), 4, scale, _lib.PREC_BF16X3, _lib.PREC_ATTN16))
    assert torch.isfinite(got).all(), "non-finite attention output: the SAFE path did not run"
    qs = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)      # as mvs_tr_qkv_fwd forms it
    xh = x.reshape(1, n, 4, 16).permute(0, 2, 1, 3)
    q16, k16, v16 = (xh * qs).half().double(), xh.half().double(), xh.bfloat16().double()
    assert torch.equal(k16.float(), xh), "the test's operands must be exact in fp16"
    s2 = q16 @ k16.transpose(-2, -1)                                   # base-2 scores
    jump = s2[..., t] - s2[..., :128].max(-1).values
    assert float(jump.max()) > 140.0 and float(jump.abs().min()) > 100.0, "the case must overflow fp32 inside a block, without near-ties"
    pr = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    ref = ((pr / pr.sum(-1, keepdim=True)) @ v16).transpose(1, 2).reshape(1, n, 64).float()
    err = float(((got - ref).abs() / (1.0 + ref.abs())).max())
    assert err <= 1e-2, err                                             # bf16 probabilities: 2^-9 each
    return err


def case_stage_transformer_bf16p(device):
    """Shipped stage 1 with bf16 attention probabilities (attention_precision="bf16p"): logits move at the 1e-3 level, depth does not."""
    from mvsformerplusplus_amd.cost_volume import StageNet
    fx = load_golden("f8_stage_transformer.npz")
    args = dict(ARGS, cost_reg_type=["PureTransformerCostReg", "Normal", "Normal", "Normal"],
                transformer_config=[dict(_tcfg(fx), attention_precision="bf16p")])
    st = StageNet(args, 32, 0)
    st.load_state_dict(golden_weights(fx), strict=True)
    st = st.eval().to(device)
    assert st.cost_reg.attention_precision == "bf16p"
    with torch.no_grad():
        out = st(dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device), tmp=5.0, position3d=dev(fx["position3d"], device))
    assert (cpu(out["prob_volume_pre"]) - fx["prob_volume_pre"]).abs().max() <= 2e-2
    assert rel_l1(cpu(out["depth"]), fx["depth"]) <= 1e-4


# ---------------------------------------------------------------- depth-map filtering
def _mask_mismatch(a, b):
    return float((a.bool() != b.bool()).float().mean())


def _close_rel(a, b, rtol=2e-3, sane=1e4):
    """Hole pixels (depth 0) project through a 1e-9 denominator: the reference's own values there are ~1e6..1e9 and flip with
    the last bit of a cancellation, so only entries the fixture holds below `sane` are compared (they must be the majority)."""
    ok = b.abs() < sane
    assert float(ok.float().mean()) > 0.5
    return bool(((a - b).abs()[ok] <= rtol * b.abs().clamp_min(1.0)[ok]).all())


def case_fusion_golden(device):
    """misc/fusion.py + the per-view bodies of test.py's two filter drivers against fixture f10 (generated from the reference).
    Threshold comparisons sit on fp32 values that differ in the last bits between implementations, so boolean outputs are
    compared by mismatch rate (<= 0.5 %) and depths where both agree."""
    from mvsformerplusplus_amd import fusion as Fu
    fx = load_golden("f10_fusion.npz")
    d = lambda k: dev(fx[k], device)
    rd, sd, rc, sc = d("ref_depth"), d("srcs_depth"), d("ref_cam"), d("srcs_cam")
    n, v, _, h, w = fx["srcs_depth"].shape
    with torch.no_grad():
        # ---- static: the three API calls the way test.py:393-396 chains them, then the fused one-launch form ----
        sdm = sd * (d("srcs_conf") > float(fx["conf_thresh"])).float().unsqueeze(2)
        xyd, inr = Fu.get_reproj(rd, sdm, rc, sc)
        assert _close_rel(cpu(xyd), fx["s_reproj_xyd"])
        assert _mask_mismatch(cpu(inr), fx["s_in_range"]) <= 5e-3
        masks, mask = Fu.vis_filter(rd, dev(fx["s_reproj_xyd"], device), dev(fx["s_in_range"], device), float(fx["thres_disp"]), 0.01, int(fx["thres_view"]))
        assert _mask_mismatch(cpu(masks), fx["s_vis_masks"]) <= 5e-3 and _mask_mismatch(cpu(mask), fx["s_geo_mask"]) <= 5e-3
        ave = Fu.ave_fusion(rd, dev(fx["s_reproj_xyd"], device), dev(fx["s_vis_masks"], device))
        assert (cpu(ave) - fx["s_depth"]).abs().max() <= 1e-3
        out = Fu.filter_depth(rd, d("ref_conf"), sd, d("srcs_conf"), rc, sc, conf_thresh=float(fx["conf_thresh"]),
                              thres_disp=float(fx["thres_disp"]), thres_view=int(fx["thres_view"]))
        assert _mask_mismatch(cpu(out["mask"]), fx["s_mask"]) <= 5e-3 and _mask_mismatch(cpu(out["geo_mask"]), fx["s_geo_mask"]) <= 5e-3
        same = (cpu(out["geo_mask"]) == fx["s_geo_mask"]) & ((cpu(out["depth"]) - fx["s_depth"]).abs() < 0.5)
        assert float(same.float().mean()) >= 0.99
        assert ((cpu(out["depth"]) - fx["s_depth"]).abs()[same]).max() <= 2e-3
        assert ((cpu(out["points"]) - fx["s_points"]).abs().amax(1, keepdim=True)[same]).max() <= 5e-3
        # ---- dynamic ----
        xyd = Fu.get_reproj_dynamic(rd, sd, rc, sc)
        assert _close_rel(cpu(xyd), fx["d_reproj_xyd"])
        masks, mask = Fu.vis_filter_dynamic(rd, dev(fx["d_reproj_xyd"], device))
        assert tuple(masks.shape) == (n, v, v - 1, h, w) and _mask_mismatch(cpu(masks), fx["d_vis_masks"]) <= 5e-3
        out = Fu.dynamic_filter_depth(rd, d("ref_conf"), sd, rc, sc, conf_thresh=float(fx["conf_thresh"]))
        assert _mask_mismatch(cpu(out["mask"]), fx["d_mask"]) <= 5e-3 and _mask_mismatch(cpu(out["geo_mask"]), fx["d_geo_mask"]) <= 5e-3
        same = (cpu(out["depth"]) - fx["d_depth"]).abs() < 0.5
        assert float(same.float().mean()) >= 0.99
        assert ((cpu(out["depth"]) - fx["d_depth"]).abs()[same]).max() <= 2e-3
        assert ((cpu(out["points"]) - fx["d_points"]).abs().amax(1, keepdim=True)[same]).max() <= 5e-3


# ---- the filters against an fp64 restatement at scene sizes: exact on decided pixels, bounded elsewhere ----
_EPS32 = 2.0 ** -23


def _fp32_delta(q64, q32, scale, sens, mult=16.0, sens_mult=4.0, floor_ulps=8.0):
    """How close to a threshold an fp64 quantity must sit before fp32 rounding may flip the comparison; the largest of
    - `mult` = 16 times the fp32 restatement's error at that entry (run beside the fp64 one: the rounding of the whole chain of
      projections, ~1 ulp of `scale` - pixel coordinates for a distance, depths for a depth difference - on smooth surfaces);
    - `sens_mult` = 4 times `sens`, what the quantity moves when the bilinear sample position moves by one fp32 ulp
      (oracle/fusion_ref.tap_sensitivity).  Next to a zero-depth tap (its reprojection lies far away) the weight of that tap is
      set by the last bit of the sample coordinate: the kernel and the fp32 restatement may round it to different sides of an
      integer, and the restatement's own error then says nothing.  Without this term 1-2 of ~18 M comparisons per MI355X case
      flipped on "decided" pixels, each one a sample within 2e-5 px of an integer next to a hole (e.g. ix = 886.99998942 with
      the tap at 888 a hole: 6.6 px of x from one ulp);
    - a floor of `floor_ulps` = 8 fp32 ulps of `scale`.
    Entries where exactly one of q32 / q64 is finite get an infinite delta."""
    both = torch.isfinite(q64) & torch.isfinite(q32) & torch.isfinite(scale) & (scale > 0)
    sc = scale.abs().where(both, torch.ones_like(scale))
    rel = torch.where(both, (q32 - q64).abs() / sc, torch.zeros_like(q64))
    d = torch.maximum(mult * rel, torch.full_like(rel, floor_ulps * _EPS32)) * scale.abs()
    d = torch.maximum(d, sens_mult * sens.nan_to_num(nan=float("inf")))
    return torch.where(torch.isfinite(q64) != torch.isfinite(q32), torch.full_like(d, float("inf")), d)


def _decide(conds):
    """conds: [(holds (fp64 bool), borderline (bool))] of one AND-ed decision -> (value, borderline): decided when one condition
    is clearly false or all are clearly true."""
    val = conds[0][0].clone()
    for c, _ in conds[1:]:
        val &= c
    clear_false = torch.zeros_like(val)
    clear_true = torch.ones_like(val)
    for c, b in conds:
        clear_false |= ~c & ~b
        clear_true &= c & ~b
    return val, ~(clear_false | clear_true)


def fusion_vs_fp64(got, rd, rconf, sd, sconf, rc, sc, *, dynamic, conf_thresh, p0, p1, vthresh=0.0, bounds=None):
    """The comparison rule every fp64 case of the depth-map filters uses, for ONE batch element (all CPU tensors).
    got: the kernel's outputs (any of reproj_xyd [v,3,h,w], in_range [v,h,w], vis_masks [v,h,w] / [v,v-1,h,w], depth, geo_mask,
    mask [h,w], points [3,h,w]); inputs rd/rconf [h,w], sd/sconf [v,h,w] (sconf None = no gating), rc [2,4,4], sc [v,2,4,4];
    p0/p1 = thres_disp / depth_thresh (static) or dist_base / rel_diff_base (dynamic).

    Every (pixel, view, threshold) comparison is made in fp64 (oracle/fusion_ref.view_quantities) and is *borderline* when its
    fp64 margin is below _fp32_delta.  On the pixels without a borderline comparison ("decided") vis_masks, in_range, geo_mask,
    mask - and so the views that entered the averaged depth - must equal fp64's exactly.  The borderline share is capped at
    3 % static, 12 % dynamic (v - 1 thresholds per view): measured 1.8 % / 8.5 % at 1152x1600 with 10 sources on
    make_box_scene, whose outliers and holes put large tap differences under many samples.  Continuous outputs on decided
    pixels: depth relative to fp64 and points relative to |camera centre| + depth, each within `bounds` plus 16x the fp32
    restatement's own error of the same value (its conditioning); reproj_xyd relative on the entries fp64 holds below 1e4
    (not a hole projection), with no zero-depth tap within two pixels of the sample (fusion_ref.near_zero: the linearised
    tap_sensitivity does not hold there) and whose conditioning (16x the fp32 restatement's error, at least 4x the
    tap_sensitivity) is below the bound - they must be the majority.  Bounds, from the MI355X at 1152x1600 / 1056x1920 / 517x743 and n = 2, 10 sources
    (largest figures on the well-conditioned pixels): depth 1.4e-5 (bound 4e-5), points 1.4e-5 (4e-5), reproj_xyd 2.5e-4 (4e-4).
    Non-finite values: the fp64 depth / points are finite everywhere here and so must the kernel's be.
    -> dict of measured figures (keys with a leading "_": the fp64 mask, decided pixels and points)."""
    from oracle import fusion_ref as R
    b = dict({"depth": 4e-5, "points": 4e-5, "xyd": 4e-4, "xyd_cmp": 0.5, "borderline": 0.12 if dynamic else 0.03}, **(bounds or {}))
    v, h, w = sd.shape
    f64 = torch.float64
    rd64 = rd.double()
    sum_d = torch.zeros(h, w, dtype=f64)
    sum_d32 = torch.zeros(h, w, dtype=f64)
    cond_mult = 16.0
    cnt = torch.zeros(h, w, dtype=f64)
    counts = torch.zeros(max(v - 1, 1), h, w, dtype=f64)
    border = torch.zeros(h, w, dtype=torch.bool)
    vis, inr = [], []
    xyd_stats = {"xyd_rel": 0.0, "xyd_cmp": 0.0}
    for j in range(v):
        s = sd[j]
        if not dynamic and sconf is not None:
            s = s * (sconf[j] > conf_thresh).float()
        q = {}
        for dt in (torch.float32, f64):
            q[dt] = R.view_quantities(rd.to(dt)[None, None], s.to(dt)[None, None, None], rc.to(dt)[None], sc[j].to(dt)[None, None],
                                      dynamic=dynamic, depth_thresh=float(p1))
        a, f = q[f64], q[torch.float32]
        px_scale = torch.maximum(a["x"].abs(), a["y"].abs()).clamp_min(float(max(h, w)))
        dd = _fp32_delta(a["dist"], f["dist"], px_scale, a["sx"] + a["sy"])
        if dynamic:
            dr = _fp32_delta(a["ddiff"], f["ddiff"], (rd64.abs() + a["z"].abs()) / rd64.abs(), a["sz"] / rd64.abs())
            ms = []
            for k in range(v - 1):
                td, tr = (k + 2) / float(p0), (k + 2) / float(p1)
                m, bl = _decide([(a["dist"] < td, (a["dist"] - td).abs() < dd), (a["ddiff"] < tr, (a["ddiff"] - tr).abs() < dr)])
                counts[k] += m
                border |= bl
                ms.append(m)
            sel = ms[-1]
            vis.append(torch.stack(ms))
        else:
            dgx = _fp32_delta(a["gx"], f["gx"], torch.ones_like(a["gx"]), torch.zeros_like(a["gx"]))
            dgy = _fp32_delta(a["gy"], f["gy"], torch.ones_like(a["gy"]), torch.zeros_like(a["gy"]))
            dm = _fp32_delta(a["dmargin"], f["dmargin"], torch.maximum(rd64.abs(), a["z"].abs()), (1 + float(p1)) * a["sz"])
            ir, bx = _decide([(a["gx"] >= -1, (a["gx"] + 1).abs() < dgx), (a["gx"] <= 1, (a["gx"] - 1).abs() < dgx),
                              (a["gy"] >= -1, (a["gy"] + 1).abs() < dgy), (a["gy"] <= 1, (a["gy"] - 1).abs() < dgy)])
            sel, bl = _decide([(ir, bx), (a["dist"] < float(p0), (a["dist"] - float(p0)).abs() < dd), (a["dmargin"] < 0, a["dmargin"].abs() < dm)])
            border |= bl | bx
            vis.append(sel)
            inr.append(ir)
        sum_d += torch.where(sel, a["z"], torch.zeros_like(a["z"]))
        sum_d32 += torch.where(sel, f["z"].double(), torch.zeros_like(a["z"]))
        cnt += sel
        if "reproj_xyd" in got:
            # every entry fp64 holds below 1e4 (not a hole projection) is compared; the bound adds the entry's own conditioning
            ref = torch.stack([a["x"], a["y"], a["z"]])
            cond = torch.maximum((torch.stack([f["x"], f["y"], f["z"]]).double() - ref).abs(),
                                 0.25 * torch.stack([a["sx"], a["sy"], a["sz"]]).nan_to_num(nan=float("inf")))   # 16 x 0.25 = 4 x the sample sensitivity
            scale = ref.abs().clamp_min(1.0)
            ok = ref.abs() < 1e4
            err = (got["reproj_xyd"][j].double() - ref).abs()
            well = ok & ~a["hole"][None] & (cond_mult * cond <= b["xyd"] * scale)   # well-conditioned: no hole tap, not on an edge
            xyd_stats["xyd_rel"] = max(xyd_stats["xyd_rel"], float((err / scale)[well].max()) if well.any() else 0.0)
            xyd_stats["xyd_cmp"] += float(well.double().mean()) / v
    ave = (sum_d + rd64) / (cnt + 1)
    ave_cond = ((sum_d32 + rd64) / (cnt + 1) - ave).abs()          # the fp32 restatement's error of the same average, same views
    if dynamic:
        geo = cnt >= v + 1
        for k in range(v - 1):
            geo |= counts[k] >= k + 2
    else:
        geo = cnt >= (vthresh - 1.1)
    prob = rconf > conf_thresh
    mask = geo & prob
    dec = ~border
    share = float(border.double().mean())
    stats = dict(xyd_stats, borderline=share)
    assert share <= b["borderline"], ("borderline share", share)
    if "vis_masks" in got:
        want = torch.stack(vis)
        gv = got["vis_masks"].bool().reshape(want.shape)
        bad = (gv != want) & dec.expand_as(want)
        assert not bad.any(), ("vis_masks differ on decided pixels", int(bad.sum()), bad.nonzero()[:5].tolist())
    if "in_range" in got and not dynamic:
        want = torch.stack(inr)
        bad = (got["in_range"].reshape(want.shape) > 0) != want
        assert not (bad & dec).any(), ("in_range differs on decided pixels", int((bad & dec).sum()))
    for k, want in (("geo_mask", geo), ("mask", mask)):
        if k in got:
            bad = (got[k].reshape(h, w).bool() != want) & dec
            assert not bad.any(), ("%s differs on decided pixels" % k, int(bad.sum()), bad.nonzero()[:5].tolist())
    if "depth" in got:
        gd = got["depth"].reshape(h, w).double()
        assert torch.isfinite(ave).all() and torch.isfinite(gd).all()
        err, sc_ = (gd - ave).abs(), ave.abs().clamp_min(1e-6)
        assert not ((err > b["depth"] * sc_ + cond_mult * ave_cond) & dec).any(), ("depth", float((err / sc_)[dec].max()))
        well = dec & (cond_mult * ave_cond <= b["depth"] * sc_)
        stats["depth_rel"] = float((err / sc_)[well].max())
        stats["depth_rel_all"] = float((err / sc_)[dec].max())
    if "points" in got:
        p64 = R.backproject(ave[None, None], rc.double()[None])[0]
        E = rc[0].double()
        centre = (-E[:3, :3].t() @ E[:3, 3]).norm()
        gp = got["points"].reshape(3, h, w).double()
        assert torch.isfinite(gp).all()
        err, sc_ = (gp - p64).abs().amax(0), (centre + ave.abs()).clamp_min(1e-6)
        ray = (p64 - (-E[:3, :3].t() @ E[:3, 3])[:, None, None]).norm(dim=0) / ave.abs().clamp_min(1e-6)
        assert not ((err > b["points"] * sc_ + cond_mult * ray * ave_cond) & dec).any(), ("points", float((err / sc_)[dec].max()))
        well = dec & (cond_mult * ray * ave_cond <= b["points"] * sc_)
        stats["points_rel"] = float((err / sc_)[well].max())
        stats["_points64"] = p64
    if "reproj_xyd" in got:
        assert xyd_stats["xyd_cmp"] > b["xyd_cmp"], xyd_stats
        assert xyd_stats["xyd_rel"] <= b["xyd"], ("reproj_xyd", xyd_stats)
    stats["kept"] = float(mask.double().mean())
    stats["_mask64"], stats["_decided"] = mask, dec
    return stats


def _box_inputs(H, W, v, seed=0, metres=False, rot_deg=3.0):
    """Reference view 0 of a make_box_scene with views 1..v as its sources -> (rd, rconf [h,w], sd, sconf [v,h,w], rc, sc) CPU."""
    s = synth.make_box_scene(v + 1, H, W, seed=seed, metres=metres, rot_deg=rot_deg)
    d, c, cams = s["depth"], s["conf"], s["cams"]
    return d[0], c[0], d[1:], c[1:], cams[0], cams[1:]


def _fused(device, dynamic, inp, *, conf_thresh=0.5, p0, p1, vthresh=0.0, gate=True):
    """One launch of the fused filter with every output requested, for n = 1 -> CPU dict shaped as fusion_vs_fp64 takes it."""
    rd, rconf, sd, sconf, rc, sc = (dev(t, device) for t in inp)
    v, h, w = sd.shape
    out = ops.fusion_filter(dynamic, rd[None], sd[None], rc[None], sc[None], ref_conf=rconf[None],
                            srcs_conf=sconf[None] if (gate and not dynamic) else None, conf_thresh=conf_thresh, p0=p0, p1=p1,
                            vthresh=vthresh, want_xyd=True, want_masks=True)
    return {k: cpu(t)[0] for k, t in out.items()}


def case_fusion_scene_fp64(device, H, W, v, dynamic, *, seed=0, metres=False, rot_deg=3.0, thres_disp=1.0, thres_view=2,
                           dist_base=4.0, rel_diff_base=1300.0, bounds=None):
    """The fused filter (every output) on a box-and-plane scene against the fp64 restatement under fusion_vs_fp64's rule."""
    inp = _box_inputs(H, W, v, seed=seed, metres=metres, rot_deg=rot_deg)
    p0, p1 = (dist_base, rel_diff_base) if dynamic else (thres_disp, 0.01)
    with torch.no_grad():
        got = _fused(device, dynamic, inp, p0=p0, p1=p1, vthresh=thres_view)
    rd, rconf, sd, sconf, rc, sc = inp
    st = fusion_vs_fp64(got, rd, rconf, sd, None if dynamic else sconf, rc, sc, dynamic=dynamic, conf_thresh=0.5, p0=p0, p1=p1,
                        vthresh=thres_view, bounds=bounds)
    if not dynamic and thres_view <= 1:
        assert got["geo_mask"].bool().all()                       # sum >= -0.1: every pixel, zero-depth holes included (fusion.py:108)
    if not dynamic and thres_view >= v + 2:
        assert not got["geo_mask"].bool().any()
    if not dynamic:                                               # conf == conf_thresh is rejected: the test is strict (test.py:389-392)
        at = rconf == 0.5
        assert at.any() and not got["mask"].bool()[at].any()
    return st


def case_fusion_batch(device, H, W, v, bounds=None):
    """n = 2 with different cameras and depths per element through every entry point of fusion.py: each element equals the
    kernel's own n = 1 run of it bit for bit, and the fp64 restatement of it (run per element at n = 1: the reference's dynamic
    driver only broadcasts correctly for n = 1, scripts/fuzz_fusion_gpu.py) under fusion_vs_fp64's rule."""
    from mvsformerplusplus_amd import fusion as Fu
    from oracle import fusion_ref as R
    els = [_box_inputs(H, W, v, seed=11, rot_deg=3.0), _box_inputs(H, W, v, seed=12, metres=True, rot_deg=4.0)]
    stack = lambda i: torch.stack([e[i] for e in els])
    rd, rconf, sd, sconf, rc, sc = (dev(stack(i), device) for i in range(6))
    sdg = sd * (sconf > 0.5).float()
    kw = dict(conf_thresh=0.5, thres_disp=1.0, thres_view=2)

    def run(sl):
        r = {}
        x, ir = Fu.get_reproj(rd[sl][:, None], sdg[sl][:, :, None], rc[sl], sc[sl])
        r["s_xyd"], r["s_inr"] = x, ir
        r["s_vis"], r["s_geo"] = Fu.vis_filter(rd[sl][:, None], x, ir, 1.0, 0.01, 2)
        r["s_ave"] = Fu.ave_fusion(rd[sl][:, None], x, r["s_vis"])
        for k, t in Fu.filter_depth(rd[sl][:, None], rconf[sl], sd[sl][:, :, None], sconf[sl], rc[sl], sc[sl], **kw).items():
            r["s_" + k] = t
        x = Fu.get_reproj_dynamic(rd[sl][:, None], sd[sl][:, :, None], rc[sl], sc[sl])
        r["d_xyd"] = x
        r["d_vis"], r["d_last"] = Fu.vis_filter_dynamic(rd[sl][:, None], x, 4, 1300)
        for k, t in Fu.dynamic_filter_depth(rd[sl][:, None], rconf[sl], sd[sl][:, :, None], rc[sl], sc[sl], conf_thresh=0.5).items():
            r["d_" + k] = t
        return {k: cpu(t) for k, t in r.items()}

    with torch.no_grad():
        both = run(slice(0, 2))
        stats = []
        for b in range(2):
            one = run(slice(b, b + 1))
            for k in both:
                assert torch.equal(both[k][b:b + 1], one[k]), ("element %d of the n = 2 run differs from its n = 1 run" % b, k)
            g = lambda k: one[k][0]
            e = [t[b].cpu() for t in (rd, rconf, sd, sconf, rc, sc)]
            stats.append(fusion_vs_fp64({"reproj_xyd": g("s_xyd"), "in_range": g("s_inr"), "vis_masks": g("s_vis"), "geo_mask": g("s_geo"),
                                         "depth": g("s_depth"), "mask": g("s_mask"), "points": g("s_points")}, *e,
                                        dynamic=False, conf_thresh=0.5, p0=1.0, p1=0.01, vthresh=2, bounds=bounds))
            # ave_fusion over vis_filter's masks: z * mask summed in view order, so the fused filter's average bit for bit (every z is
            # finite here), and the restatement's within its summation order
            assert torch.equal(g("s_ave"), g("s_depth"))
            ave_ref = R.ave_fusion(e[0][None, None], g("s_xyd")[None], g("s_vis")[None])[0]
            assert ((g("s_ave") - ave_ref).abs() <= 2e-6 * ave_ref.abs().clamp_min(1.0)).all()
            stats.append(fusion_vs_fp64({"reproj_xyd": g("d_xyd"), "vis_masks": g("d_vis"), "geo_mask": g("d_geo_mask"), "depth": g("d_depth"),
                                         "mask": g("d_mask"), "points": g("d_points")}, *e[:3], None, *e[4:],
                                        dynamic=True, conf_thresh=0.5, p0=4.0, p1=1300.0, bounds=bounds))
            assert torch.equal(g("d_last"), g("d_vis")[:, -1:])
    return stats


def case_fusion_view_limits(device):
    """v = 16 is the kernel's limit (kMaxSrcViews): v = 17 is refused by both filters, v = 1 by the dynamic one."""
    for v, dyn, ok in ((16, False, True), (16, True, True), (17, False, False), (17, True, False), (1, True, False), (1, False, True)):
        rd = torch.full((1, 4, 6), 500.0, device=device)
        sd = torch.full((1, v, 4, 6), 500.0, device=device)
        cams = synth.make_cameras(v + 1, 4, 6)[0].to(device)
        try:
            ops.fusion_filter(dyn, rd, sd, cams[:1], cams[None, 1:])
            raised = None
        except _lib.MvsHipError as e:
            raised = str(e)
        assert (raised is None) == ok, (v, dyn, raised)


def _on_threshold_static(h, w, v, thres_disp, g):
    """reproj_xyd [1,v,3,h,w] whose distances and depth differences sit exactly on, one ulp inside and one ulp outside the
    static thresholds in fp32, plus in_range from {0, 1}; ref depth [1,1,h,w]."""
    f = torch.float32
    px = (torch.arange(w, dtype=f) + 0.5).expand(h, w)
    py = (torch.arange(h, dtype=f) + 0.5)[:, None].expand(h, w)
    rd = (torch.rand(h, w, generator=g) * 500 + 400).to(f)
    xs, ys, zs, inr = [], [], [], []
    p1 = torch.tensor(0.01, dtype=f)
    for _ in range(v):
        along_x = torch.rand(h, w, generator=g) < 0.5
        sign = torch.where(torch.rand(h, w, generator=g) < 0.5, -1.0, 1.0).to(f)
        centre = torch.where(along_x, px, py)
        on = centre + sign * thres_disp                                # exact: pixel centres and thresholds are multiples of 1/4
        kind = torch.randint(0, 5, (h, w), generator=g)                # centre, on, one ulp inside, one ulp outside, twice as far
        c = torch.where(kind == 0, centre, on)
        c = torch.where(kind == 2, torch.nextafter(on, centre), c)
        c = torch.where(kind == 3, torch.nextafter(on, on + sign), c)
        c = torch.where(kind == 4, centre + sign * 2 * thres_disp, c)
        xs.append(torch.where(along_x, c, px))
        ys.append(torch.where(along_x, py, c))
        # depth: |rd - z| == fl(max(rd, z) * 0.01) where a z below rd makes that hold in fp32, else one ulp off it either way
        z = rd - rd * p1
        z = torch.where((rd - z).abs() == torch.maximum(rd, z) * p1, z, rd * (1 - p1))
        pick = torch.randint(0, 4, (h, w), generator=g)
        z = torch.where(pick == 1, torch.nextafter(z, rd), torch.where(pick == 2, torch.nextafter(z, torch.zeros_like(z)), z))
        z = torch.where(pick == 3, rd * 1.003, z)
        zs.append(z)
        inr.append((torch.rand(h, w, generator=g) < 0.9).to(f))
    xyd = torch.stack([torch.stack(xs), torch.stack(ys), torch.stack(zs)], 1)[None]
    return rd[None, None], xyd, torch.stack(inr)[None, :, None]


def _on_threshold_dynamic(h, w, v, dist_base, rel_diff_base, g):
    """reproj_xyd [1,v,3,h,w] whose distances / relative depth differences are the ladder values i / base (exact in fp32 for
    the power-of-two bases used) and their fp32 neighbours, drawn per pixel and view so the threshold counts vary."""
    f = torch.float32
    px = (torch.arange(w, dtype=f) + 0.5).expand(h, w)
    py = (torch.arange(h, dtype=f) + 0.5)[:, None].expand(h, w)
    rd = torch.full((h, w), float(rel_diff_base), dtype=f)
    lad = torch.arange(1, v + 2, dtype=f)
    xs, ys, zs = [], [], []
    for _ in range(v):
        i = lad[torch.randint(0, v + 1, (h, w), generator=g)]
        on = px + i / dist_base                                        # exact: the bases used are powers of two
        nudge = torch.randint(0, 3, (h, w), generator=g)               # on the ladder value, one ulp inside, one ulp outside
        xs.append(torch.where(nudge == 1, torch.nextafter(on, px), torch.where(nudge == 2, torch.nextafter(on, on + 1), on)))
        ys.append(py.clone())
        k = lad[torch.randint(0, v + 1, (h, w), generator=g)]
        z = rd - k                                                     # |rd - z| / rd == k / rel_diff_base exactly
        nudge = torch.randint(0, 3, (h, w), generator=g)
        z = torch.where(nudge == 1, torch.nextafter(z, rd), torch.where(nudge == 2, torch.nextafter(z, torch.zeros_like(z)), z))
        zs.append(z)
    xyd = torch.stack([torch.stack(xs), torch.stack(ys), torch.stack(zs)], 1)[None]
    return rd[None, None], xyd


def case_fusion_thresholds_exact(device, h=9, w=37):
    """The stand-alone entry points fed a constructed reproj_xyd whose values sit exactly on the thresholds (and one fp32 ulp to
    either side): from the same fp32 input the decisions must equal the fp32 restatement's bit for bit.  Pins `<` against `<=`,
    the `vthresh - 1.1` offset (thres_view = 3.05: sum >= 1.95; a `- 1.0` would need 3), the dynamic ladder's i = k + 2 and
    the geo ladder.  Also ave_fusion on the same input, and its non-finite behaviour: it multiplies z * mask like the reference
    (an infinite z behind a zero mask gives NaN), whereas the fused filter adds only the selected views (finite)."""
    from mvsformerplusplus_amd import fusion as Fu
    from oracle import fusion_ref as R
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for v, thres_disp, thres_view in ((1, 1.0, 1), (2, 0.25, 2), (4, 4.0, 3.05), (10, 1.0, 3.05), (16, 0.25, 6)):
            rd, xyd, inr = _on_threshold_static(h, w, v, thres_disp, g)
            m_ref, geo_ref = R.vis_filter(rd, xyd, inr, thres_disp, 0.01, thres_view)
            m, geo = Fu.vis_filter(dev(rd, device), dev(xyd, device), dev(inr, device), thres_disp, 0.01, thres_view)
            assert torch.equal(cpu(m).bool(), m_ref.bool()) and torch.equal(cpu(geo).bool(), geo_ref.bool()), (v, thres_disp, thres_view)
            assert 0 < float(m_ref.float().mean()) < 1
            ave_ref = R.ave_fusion(rd, xyd, m_ref)
            ave = cpu(Fu.ave_fusion(dev(rd, device), dev(xyd, device), dev(m_ref, device)))
            assert ((ave - ave_ref).abs() <= 2e-6 * ave_ref.abs()).all()
            out = ops.fusion_filter(False, dev(rd[:, 0], device), None, None, None, xyd_in=dev(xyd, device), in_range_in=dev(inr[:, :, 0], device),
                                    p0=thres_disp, p1=0.01, vthresh=thres_view, want_masks=True, want_points=False)
            assert ((cpu(out["depth"]) - ave_ref[:, 0]).abs() <= 2e-6 * ave_ref[:, 0].abs()).all()
        for v, db, rdb in ((2, 4.0, 1024.0), (3, 4.0, 1024.0), (10, 2.0, 512.0), (16, 4.0, 1024.0)):
            rd, xyd = _on_threshold_dynamic(h, w, v, db, rdb, g)
            m_ref, last_ref = R.vis_filter_dynamic(rd, xyd, db, rdb)
            m, last = Fu.vis_filter_dynamic(dev(rd, device), dev(xyd, device), db, rdb)
            assert torch.equal(cpu(m), m_ref) and torch.equal(cpu(last), last_ref), (v, db, rdb)
            assert 0.05 < float(m_ref.float().mean()) < 0.95
            ave_ref, geo_ref = R.dynamic_fuse(rd, xyd, m_ref, last_ref)
            out = ops.fusion_filter(True, dev(rd[:, 0], device), None, None, None, xyd_in=dev(xyd, device), p0=db, p1=rdb,
                                    want_masks=True, want_points=False)
            assert torch.equal(cpu(out["geo_mask"]).bool(), geo_ref[:, 0]), v
            assert 0 < float(geo_ref.float().mean()) < 1
            assert ((cpu(out["depth"]) - ave_ref[:, 0]).abs() <= 2e-6 * ave_ref[:, 0].abs()).all()
        # non-finite z on a rejected view
        rd, xyd, inr = _on_threshold_static(h, w, 3, 1.0, g)
        xyd[:, 1, 2] = float("inf")
        inr[:, 1] = 0.0
        m_ref, _ = R.vis_filter(rd, xyd, inr, 1.0, 0.01, 2)
        ave_ref = R.ave_fusion(rd, xyd, m_ref)
        assert torch.isnan(ave_ref).all()
        assert torch.isnan(cpu(Fu.ave_fusion(dev(rd, device), dev(xyd, device), dev(m_ref, device)))).all()
        out = ops.fusion_filter(False, dev(rd[:, 0], device), None, None, None, xyd_in=dev(xyd, device), in_range_in=dev(inr[:, :, 0], device),
                                p0=1.0, p1=0.01, vthresh=2, want_masks=True, want_points=False)
        finite = xyd.clone()
        finite[:, 1, 2] = 0.0
        assert torch.equal(cpu(out["vis_masks"]).bool(), m_ref[:, :, 0].bool())
        assert ((cpu(out["depth"]) - R.ave_fusion(rd, finite, m_ref)[:, 0]).abs() <= 2e-6 * rd[:, 0]).all()


# ---------------------------------------------------------------- section 8f #2: backward of the aggregation, training path
def case_aggregate_backward(device):
    """mvs_warp_corr_aggregate_bwd against torch autograd through the oracle's warp + correlation + aggregation, for C = G
    (one channel per group), C = 4 G, a border-heavy camera pair (zero-padding taps) and bf16 features.  The 4 x zoom row is compared
    with fp64 autograd through tests/warp_ref.py instead: there the oracle's own fp32 inverse moves the taps, and its bar is
    max(the 3e-5 of the other rows, 3 x the oracle's own error against fp64), never more than the 1e-3 it had against the oracle."""
    import warp_ref as R64
    # last case: the source view sees the scene at 4 x the reference's magnification, so the taps of a 16 x 16 tile spread over
    # ~48 x 64 source pixels - more than the LDS window image holds (the tile scatters straight to global memory)
    for C, G, D, H, W, V, dt, zoom in ((8, 8, 4, 12, 20, 3, torch.float32, 1.0), (32, 8, 6, 10, 16, 4, torch.float32, 1.0),
                                      (16, 8, 4, 12, 20, 3, torch.bfloat16, 1.0), (8, 8, 4, 48, 96, 3, torch.float32, 4.0)):
        g = torch.Generator().manual_seed(C + D)
        cams = synth.make_cameras(V, H, W, baseline=60.0, rot_deg=4.0, seed=C)
        cams[:, 1:, 1, :2, :] *= zoom
        feats = torch.randn(1, V, C, H, W, generator=g).to(dt)
        hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.05 * torch.rand(1, D, H, W, generator=g))).contiguous()
        vis = torch.rand(1, V - 1, H, W, generator=g) * 0.9 + 0.05
        gvol = torch.randn(1, G, D, H, W, generator=g)
        # oracle + autograd (float32 math on the same, possibly bf16-rounded, feature values)
        f32 = feats.float().requires_grad_(True)
        visr = vis.clone().requires_grad_(True)
        ref_proj = O.compose_proj(cams[:, 0])
        vol_sum, vis_sum = 0.0, 0.0
        for v in range(1, V):
            warped, _ = O.homo_warping_3D_with_mask(f32[:, v], O.compose_proj(cams[:, v]), ref_proj, hyp)
            ip = O.group_correlation(f32[:, 0], warped, G)
            vol_sum = vol_sum + ip * visr[:, v - 1].unsqueeze(1).unsqueeze(1)
            vis_sum = vis_sum + visr[:, v - 1]
        vol = vol_sum / (vis_sum.unsqueeze(1).unsqueeze(1) + 1e-6)
        (vol * gvol).sum().backward()
        ref_vol, ref_gf, ref_gv = vol.detach(), f32.grad, visr.grad
        if zoom != 1.0:
            f64, v64 = feats.detach().double().requires_grad_(True), vis.detach().double().requires_grad_(True)
            vol64 = R64.aggregate64(f64, cams, hyp, v64, G)[0]
            (vol64 * gvol.double()).sum().backward()
            own = max(float((ref_vol - vol64.detach()).abs().max()), 1.5 * float((ref_gf - f64.grad).abs().max()) / float(f64.grad.abs().max()),
                      1.5 * float((ref_gv - v64.grad).abs().max()) / float(v64.grad.abs().max()))      # the oracle's own distance from fp64
            ref_vol, ref_gf, ref_gv = vol64.detach().float(), f64.grad.float(), v64.grad.float()
        # HIP
        fd, code = ops._feat(dev(feats, device))
        hom = ops.compose_homography(dev(cams, device))
        vol_cl, _ = ops.warp_corr_aggregate(fd, code, hom, dev(hyp, device), dev(vis, device), G)
        # 4 x zoom: the oracle's own taps sit ~1e-4 px off fp64's (coordinates up to 400 px), on white-noise features 1.5e-4 of the value range:
        # measured against fp64 1.1e-4 on the emulator and on the MI355X, bar 4.6e-4
        tol = 3e-5 if zoom == 1.0 else min(1e-3, max(3e-5, 3 * own))
        if zoom != 1.0:
            print("case_aggregate_backward, 4 x zoom: the oracle's own distance from fp64 %.2e, bar %.2e, volume error %.2e" % (own, tol, float((cpu(vol_cl).permute(0, 4, 1, 2, 3) - ref_vol).abs().max())))
        assert (cpu(vol_cl).permute(0, 4, 1, 2, 3) - ref_vol).abs().max() <= tol
        gfeat, gvis = ops.warp_corr_aggregate_bwd(fd, code, hom, dev(hyp, device), dev(vis, device), dev(vis.sum(1), device), vol_cl,
                                                  dev(gvol.permute(0, 2, 3, 4, 1).contiguous(), device), G)
        scale_f, scale_v = float(ref_gf.abs().max()), float(ref_gv.abs().max())
        assert (cpu(gfeat) - ref_gf).abs().max() <= (tol / 1.5) * scale_f + 1e-6, (C, G, "feature gradient")
        assert (cpu(gvis) - ref_gv).abs().max() <= (tol / 1.5) * scale_v + 1e-6, (C, G, "visibility gradient", float((cpu(gvis) - ref_gv).abs().max()), scale_v)
        assert float(cpu(gfeat)[:, 1:].abs().sum()) > 0 and float(cpu(gfeat)[:, 0].abs().sum()) > 0


def case_train_backward_golden(device, tag):
    """Train-mode StageNet (BatchNorm batch statistics, checkpointed regulariser) forward + backward against gradients produced by
    the reference itself (tests/golden/make_golden.py f12): features, every parameter, running statistics after the step."""
    fx = load_golden("f12_train_backward_%s.npz" % tag)
    D = fx["hyp"].shape[1]
    net = StageNet(dict(ARGS), D, int(fx["stage_idx"]))
    net.load_state_dict(golden_weights(fx), strict=True)
    net = net.to(device).train()
    feats = dev(fx["features"], device).requires_grad_(True)
    out = net(feats, dev(fx["proj"], device), dev(fx["hyp"], device), 1.0)
    loss = (out["prob_volume"] * dev(fx["R"], device)).sum() + 0.05 * out["prob_volume_pre"].pow(2).mean()
    loss.backward()
    assert abs(loss.item() - float(fx["loss"])) <= 2e-4 * max(1.0, abs(float(fx["loss"])))
    assert (cpu(out["prob_volume_pre"]) - fx["prob_volume_pre"]).abs().max() <= 2e-3 * float(fx["prob_volume_pre"].abs().max())

    def close(a, b, what, tol=3e-2):
        # Max norm relative to the largest entry of the reference's gradient.  The bulk of the tensors agrees to ~3e-5 (checked
        # through the median below); the bound on a single tensor has to allow for ONE ReLU unit whose pre-activation sits within
        # the 2^-16-class rounding difference between the split-bf16 forward and the reference's fp32 forward: at these fixture
        # sizes (24 576 activations in the first U-Net block) one flipped unit moves that block's BatchNorm-bias gradient by 1e-2
        # of its largest entry and its input gradient by 1.3e-2 (measured; the flip was located and counted: exactly one).
        err = float((cpu(a) - b).abs().max()) / max(float(b.abs().max()), 1e-12)
        errs.append(err)
        assert err <= tol, "%s: %g" % (what, err)
    errs = []
    close(feats.grad, fx["g_features"], "d loss / d features")
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        close(p.grad, fx["g." + name], "d loss / d " + name)
    assert sorted(errs)[len(errs) // 2] <= 2e-4, "median gradient error %g" % sorted(errs)[len(errs) // 2]
    for k, v in net.state_dict().items():
        if "running_" in k:
            close(v, fx["stat." + k], k, 1e-3)
    import os
    if os.environ.get("MVS_TEST_VERBOSE"):
        print("train-backward golden %s: worst relative max-norm error %.2e over %d tensors" % (tag, max(errs), len(errs)))


def case_train_fp32_configured_head(device):
    """A head configured for exact-fp32 INFERENCE (conv_precision="fp32") still trains: the training path runs the same
    fp32-equivalent split-bf16 kernels as for "bf16x3" - the same loss and gradients - and says so once."""
    import warnings
    from mvsformerplusplus_amd import training
    fx = load_golden("f12_train_backward_s3.npz")
    D = fx["hyp"].shape[1]
    grads = {}
    training._FP32_TRAIN_WARNED = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for prec in ("bf16x3", "fp32"):
            net = StageNet(with_prec(ARGS, prec), D, int(fx["stage_idx"]))
            net.load_state_dict(golden_weights(fx), strict=True)
            net = net.to(device).train()
            feats = dev(fx["features"], device).requires_grad_(True)
            out = net(feats, dev(fx["proj"], device), dev(fx["hyp"], device), 1.0)
            ((out["prob_volume"] * dev(fx["R"], device)).sum() + 0.05 * out["prob_volume_pre"].pow(2).mean()).backward()
            grads[prec] = [cpu(feats.grad)] + [cpu(p.grad) for p in net.parameters()]
    assert sum("conv_precision='fp32'" in str(w.message) for w in rec) == 1, "one warning, from the fp32-configured head"
    # the same kernels: equal up to the summation order of the gather backward's atomic scatter (bit-identical on the emulator)
    for a, b in zip(grads["bf16x3"], grads["fp32"]):
        assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-12)
    training._FP32_TRAIN_WARNED = False


def case_train_path_properties(device):
    """Training-path behaviour that needs no golden: eval-mode autograd equals the HIP inference outputs, gradient flows to the
    source AND reference features, and the transformer regulariser refuses to train."""
    fx = load_golden("f2_stage_s3.npz")
    # eval mode: BatchNorm uses running statistics on both paths; "bf16x3": the autograd path runs the fp32-activation kernels whatever the
    # stage's inference format is, so this is the like-for-like comparison (the fp16 default against goldens: case_stage_golden)
    net = make_stage(fx, fx["hyp"].shape[1], 3, device, prec="bf16x3")
    feats, proj, hyp = dev(fx["features"], device), dev(fx["proj"], device), dev(fx["hyp"], device)
    with torch.no_grad():
        ref = net(feats, proj, hyp, 1.0)
    fg = feats.clone().requires_grad_(True)
    out = net(fg, proj, hyp, 1.0)                                # features require grad -> autograd path
    assert out["prob_volume_pre"].requires_grad
    assert (cpu(out["prob_volume_pre"]) - cpu(ref["prob_volume_pre"])).abs().max() <= 1e-3
    assert rel_l1(cpu(out["depth"]), cpu(ref["depth"])) <= 2e-5
    out["prob_volume_pre"].square().mean().backward()
    assert float(fg.grad[:, 0].abs().sum()) > 0 and float(fg.grad[:, 1:].abs().sum()) > 0
    # half-precision features (train.py under AMP hands fp16 / bf16 feature maps over): gradient comes back in the features' dtype and
    # equals the fp32 run's on the rounded inputs
    for dt in ((torch.bfloat16,) if str(device) == "cpu" else (torch.bfloat16, torch.float16)):     # emulator: one dtype (CPU suite's time budget)
        fh = feats.to(dt).requires_grad_(True)
        net(fh, proj, hyp, 1.0)["prob_volume_pre"].square().mean().backward()
        f32 = feats.to(dt).float().requires_grad_(True)
        net(f32, proj, hyp, 1.0)["prob_volume_pre"].square().mean().backward()
        assert fh.grad.dtype == dt and torch.isfinite(fh.grad).all()
        assert (fh.grad.float() - f32.grad).abs().max() <= 1e-2 * f32.grad.abs().max() + 1e-6, dt
    if str(device) == "cpu":
        return            # emulator: the cascade-level check below runs on the MI355X only (CPU suite's time budget; stage-level training: F12 / F13)
    # the 4-stage cascade trains end to end: every stage's parameters and every stage's features receive a gradient
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    fx = load_golden("f4_cascade.npz")
    args = dict(ARGS, ndepths=[32, 16, 8, 4], depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], inverse_depth=True)
    head = CascadeDepthHead(args)
    for s in range(4):
        head.fusions[s].load_state_dict(golden_weights(fx, "w%d." % (s + 1)), strict=True)
    head = head.to(device).train()
    feats = {"stage%d" % s: dev(fx["features%d" % s], device).requires_grad_(True) for s in range(1, 5)}
    projs = {"stage%d" % s: dev(fx["proj%d" % s], device) for s in range(1, 5)}
    out = head(feats, projs, dev(fx["depth_values"], device))
    loss = sum(out["stage%d" % s]["prob_volume_pre"].square().mean() for s in range(1, 5))
    loss.backward()
    for s in range(1, 5):
        assert torch.isfinite(feats["stage%d" % s].grad).all() and float(feats["stage%d" % s].grad.abs().sum()) > 0, s
    for name, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def case_train_kernels(device):
    """The training-mode building blocks one by one against PyTorch on the CPU: batch-statistics BatchNorm + ReLU + skip (forward,
    backward), the fp32-MFMA weight gradient for every stride and channel pair the U-Nets use (ragged tiles, batch 2), and the three
    data-gradient identities the path relies on (conv <-> flipped conv, strided conv <-> transposed conv)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    # ---- BatchNorm + ReLU + skip
    for C, shape in ((8, (2, 3, 6, 10)), (32, (1, 4, 5, 7)), (64, (2, 2, 3, 5))):
        z = (torch.randn(*shape, C, generator=g) * 2 + 0.5).requires_grad_(True)
        skip = torch.randn(*shape, C, generator=g)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).requires_grad_(True), (torch.randn(C, generator=g) * 0.3).requires_grad_(True)
        dy = torch.randn(*shape, C, generator=g)
        y_ref = F.relu(F.batch_norm(z.reshape(-1, C), None, None, gamma, beta, True, 0.1, 1e-5)).reshape(*shape, C) + skip
        (y_ref * dy).sum().backward()
        zd = dev(z.detach(), device)
        sums = ops.bn_stats(zd)
        n = z.numel() // C
        mean, var, invstd = ops.bn_finalize(sums, n, 1e-5)
        assert (cpu(mean) - z.detach().reshape(-1, C).mean(0)).abs().max() <= 1e-5
        assert (cpu(var) - z.detach().reshape(-1, C).var(0, unbiased=False)).abs().max() <= 1e-4
        y = ops.bn_relu_apply(zd, mean, invstd, dev(gamma.detach(), device), dev(beta.detach(), device), dev(skip, device))
        assert (cpu(y) - y_ref.detach()).abs().max() <= 2e-5
        s2 = ops.bn_relu_bwd_reduce(dev(dy, device), zd, mean, invstd, dev(gamma.detach(), device), dev(beta.detach(), device))
        dz = ops.bn_relu_bwd_apply(dev(dy, device), zd, mean, invstd, dev(gamma.detach(), device), dev(beta.detach(), device), s2, n)
        assert (cpu(s2[:C]).float() - beta.grad).abs().max() <= 1e-4 * max(1.0, float(beta.grad.abs().max()))
        assert (cpu(s2[C:]).float() - gamma.grad).abs().max() <= 1e-4 * max(1.0, float(gamma.grad.abs().max()))
        assert (cpu(dz) - z.grad).abs().max() <= 1e-4 * max(1.0, float(z.grad.abs().max())), C
    # ---- grouped statistics: three slices normalised independently in one launch each (the visibility CNN's per-view BatchNorm)
    C, G3 = 16, 3
    z = torch.randn(G3 * 2, 5, 7, C, generator=g) * torch.tensor([1.0, 3.0, 0.5]).repeat_interleave(2).view(-1, 1, 1, 1) + 0.3
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    dy = torch.randn(z.shape, generator=g)
    rm, rv = torch.zeros(C), torch.ones(C)
    zd = dev(z, device)
    rmd, rvd = dev(rm.clone(), device), dev(rv.clone(), device)
    sums = ops.bn_stats(zd, G3)
    n = z.numel() // C // G3
    mean, var, invstd = ops.bn_finalize(sums, n, 1e-5, rmd, rvd, 0.1)
    y = ops.bn_relu_apply(zd, mean, invstd, dev(gamma, device), dev(beta, device))
    s2 = ops.bn_relu_bwd_reduce(dev(dy, device), zd, mean, invstd, dev(gamma, device), dev(beta, device))
    dz = ops.bn_relu_bwd_apply(dev(dy, device), zd, mean, invstd, dev(gamma, device), dev(beta, device), s2, n)
    bn = torch.nn.BatchNorm1d(C, momentum=0.1)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    for gi in range(G3):
        zs = z[2 * gi:2 * gi + 2].clone().requires_grad_(True)
        ys = F.relu(bn(zs.reshape(-1, C))).reshape(zs.shape)
        (ys * dy[2 * gi:2 * gi + 2]).sum().backward()
        assert (cpu(y)[2 * gi:2 * gi + 2] - ys.detach()).abs().max() <= 2e-5, gi
        assert (cpu(dz)[2 * gi:2 * gi + 2] - zs.grad).abs().max() <= 1e-4 * max(1.0, float(zs.grad.abs().max())), gi
    assert (cpu(s2)[:, :C].sum(0).float() - bn.bias.grad).abs().max() <= 1e-4 * max(1.0, float(bn.bias.grad.abs().max()))
    assert (cpu(s2)[:, C:].sum(0).float() - bn.weight.grad).abs().max() <= 1e-4 * max(1.0, float(bn.weight.grad.abs().max()))
    assert (cpu(rmd) - bn.running_mean).abs().max() <= 1e-5 and (cpu(rvd) - bn.running_var).abs().max() <= 1e-4     # three momentum steps, in order
    # ---- weight gradient (and the transposed-convolution form)
    for CA, CB, stride, shape in ((8, 16, (1, 2, 2), (2, 4, 10, 36)), (16, 16, (1, 1, 1), (1, 5, 9, 20)), (32, 64, (2, 2, 2), (1, 4, 6, 8)),
                                 (64, 64, (1, 1, 1), (1, 2, 3, 5)), (8, 16, (2, 2, 2), (2, 6, 8, 18))):
        a = torch.randn(shape[0], CA, *shape[1:], generator=g)
        w = torch.randn(CB, CA, 3, 3, 3, generator=g) * 0.1
        out = F.conv3d(a, w, None, stride=stride, padding=1)
        gy = torch.randn(out.shape, generator=g)
        ref = torch.nn.grad.conv3d_weight(a, w.shape, gy, stride=stride, padding=1)
        dw = ops.conv3d_wgrad(dev(a.permute(0, 2, 3, 4, 1).contiguous(), device), dev(gy.permute(0, 2, 3, 4, 1).contiguous(), device), stride)
        assert (cpu(dw) - ref).abs().max() <= 2e-5 * float(ref.abs().max()) + 1e-5, (CA, CB, stride)
    # k = (1,3,3): the 2-D layers of the visibility CNN on D = 1 volumes
    a2 = torch.randn(3, 16, 21, 37, generator=g)
    w2 = torch.randn(8, 16, 3, 3, generator=g) * 0.1
    gy2 = torch.randn(3, 8, 21, 37, generator=g)
    ref2 = torch.nn.grad.conv2d_weight(a2, w2.shape, gy2, padding=1)
    dw2 = ops.conv3d_wgrad(dev(a2.permute(0, 2, 3, 1).contiguous().unsqueeze(1), device), dev(gy2.permute(0, 2, 3, 1).contiguous().unsqueeze(1), device),
                           (1, 1, 1), kd=1)
    assert (cpu(dw2)[:, :, 0] - ref2).abs().max() <= 2e-5 * float(ref2.abs().max()) + 1e-5
    # ConvTranspose3d(16 -> 8, stride (1,2,2)): dW[ci][co] from (a = output gradient, g = input)
    x = torch.randn(1, 16, 3, 5, 6, generator=g, requires_grad=False)
    wt = (torch.randn(16, 8, 3, 3, 3, generator=g) * 0.1).requires_grad_(True)
    yt = F.conv_transpose3d(x, wt, None, stride=(1, 2, 2), padding=1, output_padding=(0, 1, 1))
    gyt = torch.randn(yt.shape, generator=g)
    (yt * gyt).sum().backward()
    dwt = ops.conv3d_wgrad(dev(gyt.permute(0, 2, 3, 4, 1).contiguous(), device), dev(x.permute(0, 2, 3, 4, 1).contiguous(), device), (1, 2, 2))
    assert (cpu(dwt) - wt.grad).abs().max() <= 2e-5 * float(wt.grad.abs().max()) + 1e-5


def case_device_packing(device):
    """The packing kernels against packing.py, bit for bit, for every layer shape of the U-Nets and the visibility CNN, plus the
    flipped / transposed form used for data gradients."""
    g = torch.Generator().manual_seed(4)
    for co, ci, kd, ch in ((16, 8, 3, 8), (16, 16, 3, 16), (32, 16, 3, 8), (32, 32, 3, 16), (64, 32, 3, 8), (64, 64, 3, 16), (16, 16, 1, 16), (8, 16, 1, 16)):
        w = torch.randn(co, ci, kd, 3, 3, generator=g)
        ref = packing.pack_conv_weights_bf16x3(w, ch)
        got = cpu(ops.pack_conv_weights_device(dev(w, device), ch))
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (co, ci, kd)
        if co == ci or kd == 3:
            wt = w.transpose(0, 1).flip(2, 3, 4).contiguous()
            cht = packing.conv_chunk(co, (1, 1, 1)) if kd == 3 else 16
            if co % cht == 0:
                ref_t = packing.pack_conv_weights_bf16x3(wt, cht)
                got_t = cpu(ops.pack_conv_weights_device(dev(w, device), cht, tflip=True))
                assert torch.equal(got_t.view(torch.int16), ref_t.view(torch.int16)), ("tflip", co, ci, kd)
    for ci, co in ((64, 32), (32, 16), (16, 8)):
        for sd in (1, 2):
            w = torch.randn(ci, co, 3, 3, 3, generator=g)
            ref = packing.pack_deconv_weights_bf16x3(w, sd)
            got = cpu(ops.pack_deconv_weights_device(dev(w, device), sd))
            assert got.numel() == ref.numel() and torch.equal(got.view(torch.int16), ref.view(torch.int16)), (ci, co, sd)


def case_regnet_train_native(device):
    """RegNetTrain (forward convolutions and data gradients on the split-bf16 MFMA kernels, weight gradients on fp32 MFMA, BatchNorm
    kernels) against PyTorch autograd through the same modules, CostRegNet (stride 2,2,2) and CostRegNet3D (1,2,2), train mode."""
    import copy
    from mvsformerplusplus_amd import training as T
    from train_torch_route import regnet_forward_torch
    for cls, shape in ((M.CostRegNet3D, (2, 4, 16, 24)), (M.CostRegNet, (2, 16, 16, 24))):
        reg = cls(8, 8)
        reg.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(reg.state_dict()), 3))
        reg.train()
        native = copy.deepcopy(reg).to(device)
        g = torch.Generator().manual_seed(1)
        x = torch.randn(shape[0], 8, *shape[1:], generator=g) * 0.3
        R = torch.randn(shape[0], *shape[1:], 8, generator=g)
        xa = x.clone().requires_grad_(True)
        ya = regnet_forward_torch(reg, xa)                          # [B,1,D,H,W] logits incl. `prob`
        xb = dev(x.permute(0, 2, 3, 4, 1).contiguous(), device).requires_grad_(True)
        fb = T.regnet_forward_native(native, xb)
        yb = native.prob(fb.permute(0, 4, 1, 2, 3))
        assert (cpu(yb) - ya.detach()).abs().max() <= 1e-4 * float(ya.abs().max())
        w = torch.randn(ya.shape, generator=g)
        (ya * w).sum().backward()
        (yb * dev(w, device)).sum().backward()
        errs = [float((cpu(xb.grad).permute(0, 4, 1, 2, 3) - xa.grad).abs().max() / xa.grad.abs().max())]
        for (n, p), (_, q) in zip(reg.named_parameters(), native.named_parameters()):
            errs.append(float((cpu(q.grad) - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-12)))
        assert max(errs) <= 3e-2 and sorted(errs)[len(errs) // 2] <= 2e-4, (cls.__name__, max(errs))     # see case_train_backward_golden
        for (n, b1), (_, b2) in zip(reg.named_buffers(), native.named_buffers()):
            if "running_" in n:
                assert (cpu(b2) - b1).abs().max() <= 1e-4 * max(1.0, float(b1.abs().max())), n


def case_regnet_train_recompute(device):
    """checkpoint-style recomputation in the native U-Net (module.py:393-396, 488-492: the reference runs forward_once under
    torch.utils.checkpoint): with `recompute_in_backward = True` the forward keeps the input volume, the parameters and [C]-sized
    statistics only, the backward regenerates the activations with the saved statistics - the output is BIT-IDENTICAL to the
    keep-everything mode, every gradient, the running statistics and num_batches_tracked (two momentum steps per iteration) equal it
    to the run-to-run spread of the weight-gradient kernel's atomics (exactly, on the sequential emulator), and the
    tensors held between forward and backward shrink to the input volume + weights.  The size rule picks the mode when the flag is unset."""
    import copy
    from mvsformerplusplus_amd import training as T
    for cls, shape, granular in ((M.CostRegNet3D, (2, 4, 16, 24), False), (M.CostRegNet, (1, 16, 16, 24), False), (M.CostRegNet3D, (1, 4, 16, 24), True)):
        reg = cls(8, 8)
        reg.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(reg.state_dict()), 3))
        reg.train()
        if granular:                                      # cumulative-average BatchNorm: the granular (not one-call) block path
            for m in reg.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.momentum = None
        g = torch.Generator().manual_seed(2)
        x = torch.randn(shape[0], *shape[1:], 8, generator=g) * 0.3
        wgt = torch.randn(shape[0], *shape[1:], 8, generator=g)
        res = {}
        for mode in (False, True):
            net = copy.deepcopy(reg).to(device)
            net.recompute_in_backward = mode
            xb = dev(x, device).requires_grad_(True)
            fb = T.regnet_forward_native(net, xb)
            held = sum(t.numel() * t.element_size() for t in {id(t): t for t in fb.grad_fn.saved_tensors}.values())
            (fb * dev(wgt, device)).sum().backward()
            res[mode] = (cpu(fb.detach()), cpu(xb.grad), [cpu(p.grad) for p in net.parameters() if p.grad is not None], [cpu(b.float()) for b in net.buffers()], held)
        keep, rec = res[False], res[True]
        # the regenerated activations are bit-identical (deterministic convolutions, saved statistics): so is the output; gradients pass
        # through the weight-gradient kernel's same-address fp32 atomics, whose order differs from launch to launch on the GPU
        close = lambda a, b: torch.equal(a, b) or float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-30)
        assert torch.equal(keep[0], rec[0]) and close(keep[1], rec[1]), cls.__name__
        assert all(close(a, b) for a, b in zip(keep[2], rec[2])), cls.__name__ + ": parameter gradients"
        assert all(close(a, b) for a, b in zip(keep[3], rec[3])), cls.__name__ + ": running statistics / num_batches_tracked"
        vol_bytes = x.numel() * 4
        par_bytes = sum(p.numel() * 4 for n, p in reg.named_parameters() if not n.startswith("prob"))
        assert rec[4] <= vol_bytes + par_bytes + (64 << 10), (cls.__name__, rec[4], vol_bytes, par_bytes)     # input volume + parameters + [C] statistics
        est = T.RegNetTrain.kept_bytes(reg, x.shape)
        assert abs((keep[4] - rec[4]) - est) <= 0.15 * est, (cls.__name__, keep[4], rec[4], est)               # the activations are what went away
    reg = M.CostRegNet3D(8, 8)
    assert not T.RegNetTrain._wants_recompute(reg, (2, 4, 512, 640)) and T.RegNetTrain._wants_recompute(reg, (2, 4, 1152, 1536))


def case_attention_backward(device):
    """mvs_tr_attention_bwd and the AttentionTrain autograd node (native qkv + flash-attention forward, native backward) against
    float64 autograd through F.scaled_dot_product_attention: token counts that are not multiples of the block (200, 333), batch 2,
    the entropy-invariance scale, and a peaky case (large scores: the log-sum-exp path)."""
    import math
    import torch.nn.functional as F
    from mvsformerplusplus_amd import training as T
    g = torch.Generator().manual_seed(12)
    for B, n, gain in ((2, 200, 1.0), (1, 333, 6.0)):
        heads, C = 4, 64
        t = torch.randn(B, n, C, generator=g)
        w = torch.randn(3 * C, C, generator=g) * (gain / math.sqrt(C))
        R = torch.randn(B, n, C, generator=g)
        scale = (C // heads) ** -0.5 * math.log(n, 1500.0)
        t64, w64 = t.double().requires_grad_(True), w.double().requires_grad_(True)
        q, k, v = (t64 @ w64.t()).reshape(B, n, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
        a64 = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, n, C)
        (a64 * R.double()).sum().backward()
        # the raw entry point on the float64 route's own q | k | v and output
        qkv32 = (t64 @ w64.t()).detach().float()
        d_qkv = cpu(ops.tr_attention_bwd(dev(qkv32, device), dev(a64.detach().float(), device), dev(R, device), heads, scale))
        d_t = (d_qkv.reshape(B * n, 3 * C).double() @ w64.detach()).reshape(B, n, C)
        assert (d_t - t64.grad).abs().max() <= 2e-5 * float(t64.grad.abs().max()), (n, "mvs_tr_attention_bwd")
        # the autograd node end to end (forward on the split-bf16 kernels)
        tn, wn = dev(t, device).requires_grad_(True), dev(w, device).requires_grad_(True)
        an = T.AttentionTrain.apply(tn, wn, heads, scale)
        assert (cpu(an) - a64.detach().float()).abs().max() <= 2e-4 * float(a64.abs().max()), n
        (an * dev(R, device)).sum().backward()
        for name, got, ref in (("d_t", cpu(tn.grad), t64.grad), ("d_W", cpu(wn.grad), w64.grad)):
            assert (got - ref.float()).abs().max() <= 5e-4 * float(ref.abs().max()), (n, name, float((got - ref.float()).abs().max() / ref.abs().max()))


def case_transformer_block_backward(device):
    """TransformerBlockTrain (native forward, hand-written backward: module.py:535-583) against float64 autograd through the block's
    own parameters: output, the token gradient and all 13 parameter gradients."""
    import copy, math
    import torch.nn.functional as F
    from mvsformerplusplus_amd import training as T
    g = torch.Generator().manual_seed(5)
    B, n, C, heads = 2, 150, 64, 4
    blk = M.FlashAttnBlock(C, num_heads=heads, mlp_ratio=4)
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() == 0 else 1.0 / math.sqrt(p.shape[-1]) if p.dim() == 2 else 0.3))
        blk.gamma1.fill_(0.7); blk.gamma2.fill_(1.3)
        blk.norm1.weight.add_(1.0); blk.norm2.weight.add_(1.0)
    t = torch.randn(B, n, C, generator=g)
    R = torch.randn(B, n, C, generator=g)
    scale = (C // heads) ** -0.5
    ref = copy.deepcopy(blk).double()
    t64 = t.double().requires_grad_(True)
    q, k, v = ref.attn.qkv(t64).reshape(B, n, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    a = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, n, C)
    u = ref.norm1(t64 + ref.gamma1 * ref.attn.proj(a))
    y64 = ref.norm2(u + ref.gamma2 * ref.ffn.linear2(F.gelu(ref.ffn.linear1(u))))
    (y64 * R.double()).sum().backward()
    nat = copy.deepcopy(blk).to(device)
    tn = dev(t, device).requires_grad_(True)
    yn = T.TransformerBlockTrain.apply(tn, heads, scale, nat.attn.qkv.weight, nat.attn.proj.weight, nat.attn.proj.bias, nat.gamma1,
                                       nat.norm1.weight, nat.norm1.bias, nat.norm1.eps, nat.ffn.linear1.weight, nat.ffn.linear1.bias,
                                       nat.ffn.linear2.weight, nat.ffn.linear2.bias, nat.gamma2, nat.norm2.weight, nat.norm2.bias, nat.norm2.eps)
    assert (cpu(yn) - y64.detach().float()).abs().max() <= 2e-4 * float(y64.abs().max())
    (yn * dev(R, device)).sum().backward()
    errs = {"d_t": float((cpu(tn.grad) - t64.grad.float()).abs().max() / t64.grad.abs().max())}
    for (name, p), (_, q64) in zip(nat.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, name
        errs[name] = float((cpu(p.grad) - q64.grad.float()).abs().max() / q64.grad.abs().max().clamp_min(1e-12))
    assert max(errs.values()) <= 1e-3, errs


def case_train_midsize_vs_cpu_autograd(device):
    """Train-mode forward + backward of one stage at 128 x 160, B = 2, V = 3 (a size where every U-Net level has thousands of voxels)
    against PyTorch CPU autograd with NO library kernel in it (tests/train_torch_route.stage_forward_train_cpu: the oracle's
    warping / correlation + the module's own layers), CostRegNet3D (D = 8) and CostRegNet (D = 16).  Loss to 1e-4; every gradient
    tensor's cosine >= 0.999; per-tensor max-norm error <= max(1e-2, 10 x its own yardstick), the yardstick being what 3e-6-relative
    noise on the CPU route's conv outputs does to the SAME tensor over three draws (a ReLU unit within the forward's rounding of zero
    flips with it: the measured size of a flip, not a guess); median <= max(1e-3, 3 x the yardstick's median)."""
    import copy
    from train_torch_route import stage_forward_train_cpu
    for D, C, stage in ((8, 16, 2), (16, 32, 1)):
        B, V, H, W = 2, 3, 128, 160
        net = StageNet(dict(ARGS), D, stage)
        net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 77 + D), strict=True)
        net.train()
        cams = synth.make_cameras(V, H, W, baseline=30.0, rot_deg=1.0, seed=D, batch=B)
        g = torch.Generator().manual_seed(D)
        feats = synth.make_features(cams, C, H, W, dmin=480.0, dmax=880.0, seed=D)
        hyp = ((1.0 / torch.linspace(1 / 900.0, 1 / 430.0, D))[None, :, None, None] * (1 + 0.02 * torch.rand(B, D, H, W, generator=g))).contiguous()
        R = torch.randn(B, D, H, W, generator=g)

        def run(m, fn):
            m.zero_grad()
            f = feats.clone().requires_grad_(True)
            out = fn(m, f)
            loss = (out["prob_volume"] * R).sum() + 0.05 * out["prob_volume_pre"].pow(2).mean()
            loss.backward()
            return float(loss), f.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}
        l_ref, gf_ref, gp_ref = run(copy.deepcopy(net), lambda m, f: stage_forward_train_cpu(m, f, cams, hyp, 1.0))
        yard = {}
        for draw in range(3):
            noisy = copy.deepcopy(net)
            gen = torch.Generator().manual_seed(500 + draw)
            for mod in list(noisy.cost_reg.modules()) + list(noisy.vis.modules()):
                if isinstance(mod, (torch.nn.Conv3d, torch.nn.ConvTranspose3d, torch.nn.Conv2d)):
                    mod.register_forward_hook(lambda m_, i_, o_, gen=gen: o_ + 3e-6 * float(o_.abs().max()) * torch.randn(o_.shape, generator=gen))
            _, _, gp_n = run(noisy, lambda m, f: stage_forward_train_cpu(m, f, cams, hyp, 1.0))
            for n in gp_n:
                yard[n] = max(yard.get(n, 0.0), float((gp_n[n] - gp_ref[n]).abs().max() / gp_ref[n].abs().max().clamp_min(1e-20)))
        dnet = copy.deepcopy(net).to(device)
        dfeat = dev(feats, device).requires_grad_(True)
        out = dnet(dfeat, dev(cams, device), dev(hyp, device), 1.0)
        loss = (out["prob_volume"] * dev(R, device)).sum() + 0.05 * out["prob_volume_pre"].pow(2).mean()
        loss.backward()
        assert abs(float(loss) - l_ref) <= 1e-4 * max(1.0, abs(l_ref)), (D, float(loss), l_ref)
        cos = lambda a, b: float(torch.dot(a.flatten().double(), b.flatten().double()) / (a.double().norm() * b.double().norm()).clamp_min(1e-300))
        errs = [float((cpu(dfeat.grad) - gf_ref).abs().max() / gf_ref.abs().max())]
        assert cos(cpu(dfeat.grad), gf_ref) >= 0.999, (D, "features")
        top = max(float(v.abs().max()) for v in gp_ref.values())
        for n, p in dnet.named_parameters():
            ref = gp_ref[n]
            if float(ref.abs().max()) <= 1e-6 * top:
                continue                                                  # analytically-zero gradients hold noise on both sides
            e = float((cpu(p.grad) - ref).abs().max() / ref.abs().max())
            errs.append(e)
            assert cos(cpu(p.grad), ref) >= 0.999, (D, n, cos(cpu(p.grad), ref))
            assert e <= max(1e-2, 10.0 * yard.get(n, 0.0)), (D, n, e, yard.get(n))
        ymed = sorted(yard.values())[len(yard) // 2]
        if os.environ.get("MVS_TEST_VERBOSE"):
            print("D=%d loss %.6f / %.6f  median err %.2e worst %.2e | yardstick median %.2e worst %.2e" %
                  (D, float(loss), l_ref, sorted(errs)[len(errs) // 2], max(errs), ymed, max(yard.values())))
        assert sorted(errs)[len(errs) // 2] <= max(1e-3, 3.0 * ymed), (D, sorted(errs)[len(errs) // 2], ymed)


def case_train_backward_transformer_golden(device):
    """Train-mode forward + backward of the SHIPPED stage 1 (transformer regulariser + Frustoconical PE) against the reference's own
    loss and gradients (f13): native cost volume / visibility CNN / gather backward, PyTorch autograd through the transformer."""
    from mvsformerplusplus_amd.cost_volume import StageNet
    fx = load_golden("f13_train_backward_transformer.npz")
    args = dict(ARGS, cost_reg_type=["PureTransformerCostReg", "Normal", "Normal", "Normal"], transformer_config=[_tcfg(fx)])
    net = StageNet(args, 32, 0)
    net.load_state_dict(golden_weights(fx), strict=True)
    net = net.to(device).train()
    feats = dev(fx["features"].float(), device).requires_grad_(True)
    out = net(feats, dev(fx["proj"], device), dev(fx["hyp"], device), 1.0, position3d=dev(fx["position3d"], device))
    loss = (out["prob_volume"] * dev(fx["R"], device)).sum() + 0.05 * out["prob_volume_pre"].pow(2).mean()
    loss.backward()
    assert abs(loss.item() - float(fx["loss"])) <= 2e-4 * max(1.0, abs(float(fx["loss"])))
    errs = [float((cpu(feats.grad) - fx["g_features"]).abs().max() / fx["g_features"].abs().max())]
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        ref = torch.as_tensor(fx["g." + name], dtype=torch.float32)            # 0-dim parameters (gamma1 / gamma2) come back as scalars
        errs.append(float((cpu(p.grad) - ref).abs().max() / ref.abs().max().clamp_min(1e-12)))
    assert max(errs) <= 3e-2 and sorted(errs)[len(errs) // 2] <= 5e-4, (max(errs), sorted(errs)[len(errs) // 2])


# ---------------------------------------------------------------- the warp / gather kernels on non-DTU camera rigs, against fp64
# tests/rig_cases.py builds the rigs (90 degree roll, convergent views, a source camera inside the hypothesis range, per-view intrinsics,
# a far world origin, planes ON a source's camera plane, a batch of two different rigs) and tests/warp_ref.py is the fp64 comparator.  One
# rule for every value comparison:  kernel error <= max(the project's bar for that output, 3 x the fp32 oracle's own error against fp64
# on the same voxels) - the oracle term is computed here, the factor 3 covers max-statistics noise between two fp32 evaluations.  Only
# voxels within depth/32 of a source's camera plane (fp64) are left out of value comparisons; every element of every output must be finite.
def _rig_check(figs, what, got, ref64, orc32, bar, sel=None, info=()):
    """One comparison under the rule above; `figs` (the calling case's own) collects what -> [kernel error, the oracle's error, error / allowed]."""
    got = cpu(got).double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), (what, info, "non-finite output")
    d, o = (got - ref64).abs(), (orc32.double() - ref64).abs()
    if sel is not None:
        sel = sel.expand_as(d)
        d, o = d[sel], o[sel]
    err, oerr = (float(d.max()), float(o.max())) if d.numel() else (0.0, 0.0)
    fig = figs.setdefault(what, [0.0, 0.0, 0.0])
    fig[0], fig[1], fig[2] = max(fig[0], err), max(fig[1], oerr), max(fig[2], err / max(bar, 3 * oerr))
    assert err <= max(bar, 3 * oerr), (what, info, "error %.3g > max(bar %.3g, 3 x the oracle's %.3g)" % (err, bar, oerr))
    return err, oerr


def _print_figures(title, figs):
    print("\n%s: kernel error vs fp64 | the fp32 oracle's error vs fp64 | worst error / allowed" % title)
    for k in sorted(figs):
        print("  %-56s %.2e | %.2e | %.2f" % ((k,) + tuple(figs[k])))


def _corner_displacement(hom_a, hom_b, H, W, depths):
    """Max distance in pixels between the projections of the four image corners under two homographies [..., 3, 4] (fp64), at `depths`."""
    worst = 0.0
    for x in (0.0, W - 1.0):
        for y in (0.0, H - 1.0):
            for d in depths:
                q = torch.tensor([x, y, 1.0], dtype=torch.float64)
                pa = hom_a[..., :3, :3] @ q * d + hom_a[..., :3, 3]
                pb = hom_b[..., :3, :3] @ q * d + hom_b[..., :3, 3]
                ua, ub = pa[..., :2] / pa[..., 2:3], pb[..., :2] / pb[..., 2:3]
                worst = max(worst, float((ua - ub).norm(dim=-1).max()))
    return worst


def _hom12(h):
    """[..., 12] (R row-major, then t) as the kernels write it -> [..., 3, 4] fp64"""
    h = cpu(h).double()
    return torch.cat([h[..., :9].reshape(h.shape[:-1] + (3, 3)), h[..., 9:].unsqueeze(-1)], -1)


def case_homography_rigs(device):
    """ops.compose_homography, ops.cascade_prologue (all four stage scalings of the intrinsics) and ops.homography_from_proj on every rig
    against warp_ref.homography64: the displacement of the four image corners at both ends of the hypothesis range, in pixels.
    Bar: max(1e-3 px, 3 x the displacement of the reference's own expression, matmul(src, inverse(ref)) in fp32) - for homography_from_proj,
    which starts from the composed fp32 projections, both the fp64 value and the oracle's start from those as well.
    Measured, worst displacement in px at stage scale x1 .. x8 (emulator | MI355X, the oracle's next to it; the oracle runs on the host,
    so its figure depends on the host's LAPACK):
      near-world rigs   compose / prologue 8.7e-6 .. 7.0e-5 | 1.6e-5 .. 1.3e-4   oracle 1.1e-5 .. 8.6e-5
                        from_proj 9.3e-6 | 9.3e-6   its oracle 1.1e-5
      far-world rigs    compose / prologue 7.3e-5 .. 5.8e-4 | 9.4e-5 .. 7.5e-4   oracle 5.0e-4 .. 4.0e-3 | 9.2e-4 .. 7.4e-3
                        from_proj 2.9e-6 | 2.9e-6   its oracle 4.6e-4 | 8.9e-4
    (compose / prologue start from [E, K] and multiply K E in fp32 like the reference; that rounding is their distance from fp64.)"""
    import rig_cases as RC
    import warp_ref as R64
    worst = {}
    for name, spec in RC.RIGS.items():
        for H, W in ((24, 40), (20, 70)):
            s = spec.get("s", 1.0)
            cams = torch.stack([RC.make_rig(e, H, W, s=s, zoom=spec.get("zoom", 2.0), far=spec.get("far", False), n_views=spec.get("n_views"))
                                for e in spec["elems"]])
            depths = (430.0 * s, 930.0 * s)
            stages = []
            for k in range(4):
                p = cams.clone()
                p[:, :, 1, :2, :] *= 2.0 ** k
                stages.append(p)
            homs, _ = ops.cascade_prologue([dev(p, device) for p in stages])
            for k, p in enumerate(stages):
                ref = R64.homography64(p)[..., :3, :]
                P = O.compose_proj(p.reshape(-1, 2, 4, 4)).reshape(p.shape[:2] + (4, 4))
                orc = torch.matmul(P[:, 1:], torch.inverse(P[:, :1]))[..., :3, :].double()
                Hk, Wk = H * 2 ** k, W * 2 ** k
                oerr = _corner_displacement(orc, ref, Hk, Wk, depths)
                got = {"cascade_prologue": _hom12(homs[k])}
                if k == 0:
                    got["compose_homography"] = _hom12(ops.compose_homography(dev(p, device)))
                    B, V = p.shape[:2]
                    src_p = P[:, 1:].reshape(-1, 4, 4).contiguous()
                    ref_p = P[:, :1].expand(B, V - 1, 4, 4).reshape(-1, 4, 4).contiguous()
                    fp = _hom12(ops.homography_from_proj(dev(src_p, device), dev(ref_p, device))).reshape(B, V - 1, 3, 4)
                    # this entry point starts from the COMPOSED fp32 projections: its fp64 value is the inverse of those
                    ref_fp = R64.homography64_from_proj(src_p, ref_p)[..., :3, :].reshape(B, V - 1, 3, 4)
                    orc_fp = torch.matmul(src_p, torch.inverse(ref_p))[..., :3, :].reshape(B, V - 1, 3, 4).double()
                    oerr_fp = _corner_displacement(orc_fp, ref_fp, Hk, Wk, depths)       # the oracle from the same composed projections
                    e = _corner_displacement(fp, ref_fp, Hk, Wk, depths)
                    assert e <= max(1e-3, 3 * oerr_fp), (name, "homography_from_proj", e, oerr_fp)
                    worst[("oracle from_proj", bool(spec.get("far")))] = max(worst.get(("oracle from_proj", bool(spec.get("far"))), 0.0), oerr_fp)
                    worst[("from_proj", bool(spec.get("far")))] = max(worst.get(("from_proj", bool(spec.get("far"))), 0.0), e)
                for what, h in got.items():
                    assert bool(torch.isfinite(h).all())
                    e = _corner_displacement(h, ref, Hk, Wk, depths)
                    assert e <= max(1e-3, 3 * oerr), (name, what, k, "corner displacement %.3g px, the oracle's %.3g px" % (e, oerr))
                    key = (what + (" x%d" % 2 ** k), bool(spec.get("far")))
                    worst[key] = max(worst.get(key, 0.0), e)
                    worst[("oracle x%d" % 2 ** k, bool(spec.get("far")))] = max(worst.get(("oracle x%d" % 2 ** k, bool(spec.get("far"))), 0.0), oerr)
    print("\ncase_homography_rigs: worst corner displacement in px, (entry point, far-world rig)")
    for k in sorted(worst):
        print("  %-32s %.2e" % (k, worst[k]))


def case_warp_rigs(device, name, shape):
    """homo_warping_3D_with_mask (the plain homo_warp op) on one rig, fp32 and bf16 source features, against warp_ref.warp64.
    Features: the comparison rule above with the project's 2e-4 (case_warp_golden) as the bar.  The mask may differ from fp64 only where
    the fp64 |xn| or |yn| is within 1e-4 of 1 or |pz| <= 1e-4 depth; that borderline set holds at most 1 % of the voxels (asserted from
    fp64; its measure is of order 1e-4).  On the singular rig the features are exactly 0 wherever the fp64 coordinate is beyond 1e4 px.
    Measured over the 30 cases, max abs error of the warped features vs fp64 (emulator | MI355X, then the oracle's own):
      near-world rigs 2.4e-4 | 2.1e-4, oracle 1.8e-4 (all three at 16 x 192, where a x 2.1 source coordinate reaches 400 px; 5.4e-5 | 4.8e-5,
      oracle 9.9e-5 on the smaller shapes);   far-world rigs 5.1e-4 | 4.9e-4, oracle 3.0e-3 | 3.7e-3 (its fp32 inverse)
    worst error / allowed 0.50 | 0.43; no mask difference outside the borderline set, whose largest share is 5.8e-4."""
    import rig_cases as RC
    import warp_ref as R64
    r = RC.reference(name, shape)
    cams, hyp, feats = r["cams"], r["hyp"], r["feats"]
    B, V, C, H, W = feats.shape
    singular = bool(RC.RIGS[name].get("singular"))
    ref_p = O.compose_proj(cams[:, 0])
    figs, worst_share = {}, 0.0
    for v in range(1, V):
        w64 = r["warp"][v - 1]
        src_p = O.compose_proj(cams[:, v])
        xn, yn = w64["ix"] / (W - 1) * 2 - 1, w64["iy"] / (H - 1) * 2 - 1
        border = ((xn.abs() - 1).abs() <= 1e-4) | ((yn.abs() - 1).abs() <= 1e-4) | (w64["pz"].abs() <= 1e-4 * hyp.double())
        counted = border.clone()
        if singular:
            counted[:, 3:5] = False                    # the planted planes lie ON the camera plane: borderline by construction
        share = float(counted.double().mean())
        assert share <= 0.01, (name, v, "borderline share", share)
        worst_share = max(worst_share, share)
        for dt in (torch.float32, torch.bfloat16):
            src = feats[:, v].to(dt)
            if dt == torch.float32:
                ref, orc = w64["warped"], r["warp32"][v - 1][0]
            else:
                ref = R64.warp64_hom(src.float(), r["hom64"][:, v - 1], hyp)[0]
                orc = O.homo_warping_3D_with_mask(src.float(), src_p, ref_p, hyp)[0]
            w, m = homo_warping_3D_with_mask(dev(src, device), dev(src_p, device), dev(ref_p, device), dev(hyp, device))
            m = cpu(m)
            assert not bool(((m != w64["mask"]) & ~border).any()), (name, v, dt, "mask differs from fp64 away from the frame border / camera plane")
            _rig_check(figs, "warp: features", w, ref, orc, 2e-4, r["inc"][:, v - 1].unsqueeze(1), (name, shape, v, dt))
            if singular:
                far = r["far_px"][:, v - 1].unsqueeze(1).expand_as(ref)
                assert far[:, :, 3].all() == (v == 1), "the planted plane lies on source 1's camera plane: beyond 1e4 px everywhere"
                assert not far.any() or float(cpu(w)[far].abs().max()) == 0.0, (name, v, "features on the singular planes")
    _print_figures("case_warp_rigs %s %s (borderline share %.2e)" % (name, shape, worst_share), figs)


def _cl(vol):
    """channel-last [B,D,H,W,G] -> [B,G,D,H,W] on the CPU"""
    return cpu(vol).float().permute(0, 4, 1, 2, 3)


def _gather_rig_outputs(device, feats, cams, hyp, vis, lds):
    """Every gather pass of one (features, rig) call -> dict of CPU tensors (volumes / correlations as [B,(V-1,)G,D,H,W])."""
    Gr, hd, vd = 8, dev(hyp, device), dev(vis, device)
    D = hyp.shape[1]
    f, code = ops._feat(dev(feats, device))
    hom = ops.compose_homography(dev(cams, device))
    out = {"ent": cpu(ops.warp_corr_entropy(f, code, hom, hd, Gr)), "vol": _cl(ops.warp_corr_aggregate(f, code, hom, hd, vd, Gr)[0])}
    if not lds:
        return out
    out["ent_w16"] = cpu(ops.warp_corr_entropy(f, code, hom, hd, Gr, f16_window=True))
    out["vol_f16"] = _cl(ops.warp_corr_aggregate(f, code, hom, hd, vd, Gr, f16=True)[0])
    ent_k, corr = ops.warp_corr_entropy_keep(f, code, hom, hd, Gr)
    out["ent_keep"], out["corr_keep"] = cpu(ent_k), cpu(corr).float().permute(0, 1, 5, 2, 3, 4)
    out["agg_f16"] = _cl(ops.corr_aggregate(corr, vd))
    out["agg_f32"] = _cl(ops.corr_aggregate(corr, vd, f16=False))
    out["agg_split"] = _cl(ops.from_split(ops.corr_aggregate(corr, vd, split=True)))
    if D > 4:
        ent_x, corr_x = ops.warp_corr_entropy_keep(f, code, hom, hd, Gr, exact=True)
        out["ent_exact"], out["corr_exact"] = cpu(ent_x), cpu(corr_x).permute(0, 1, 5, 2, 3, 4)
        out["agg_exact"] = _cl(ops.corr_aggregate(corr_x, vd, f16=False))
        out["agg_exact_split"] = _cl(ops.from_split(ops.corr_aggregate(corr_x, vd, split=True)))
    return out


def case_gather_rigs(device, name, shape):
    """Every gather pass on one (rig, shape) of rig_cases.GATHER_CASES against fp64: warp_corr_entropy (plain and f16_window), warp_corr_aggregate
    (fp32 and f16), warp_corr_entropy_keep (fp16 and, D > 4, exact), corr_aggregate (f16 / split / fp32) and the octet-tiled fp32 and fp16
    hand-offs of pack_features - where the shape takes the LDS-staged kernels (W % 8 == 0); the direct-gather kernels otherwise (plain passes).
    Bars (the project's, or 3 x the oracle's own error): entropy 5e-5; volume and correlations 5e-5 max(1, max|ref|); kept fp16 correlations
    6e-4 max(1, max|ref|); streamed / gathered fp16 volume 1.2e-3 scale, its fp32 and split forms 6e-4 scale.  The relations of case_gather_variants
    hold here too (tiled == planar, fp16 tiles == planar fp16 bit for bit, exact streamed == second gather, per-view partial sums == fused),
    each element of the mixed batch equals its own B = 1 run bit for bit, and on the singular rig the kept correlations are exactly 0
    wherever the fp64 coordinate is beyond 1e4 px.  A volume voxel is compared where every view's sample is, an entropy pixel where every
    plane of that view is: none for source 1 of the forward rigs from D = 16 on, where a whole plane hugs its camera plane, so up to D = 8
    at least a quarter of every view's pixels must be (asserted), which keeps the entropy of the behind-the-camera view value-checked at
    (16, 8, 24, 40), (32, 8, 12, 32) and, on the direct-gather kernels, (16, 8, 12, 36).
    zoom1.9 / zoom2.1 run at (8, 4, 12, 160) and (16, 8, 16, 192), where one tile's fp32 window of source 1 fits GL_CAP at 1.9 and exceeds
    it at 2.1 (rig_cases.rig_conditions asserts it from fp64): both the staged gather and gl_unit's gather from global memory are compared.
    Measured over the 30 cases, max abs error vs fp64: kernel (emulator | MI355X), then the fp32 oracle's own on the same voxels:
      near-world rigs   entropy 1.4e-4 | 1.9e-4, oracle 1.1e-4        volume 1.4e-4 | 1.6e-4, oracle 1.8e-4
                        exact kept correlations 1.9e-4 | 2.3e-4, oracle 1.7e-4     exact streamed volume 1.1e-4 | 1.6e-4, oracle 1.4e-4
                        kept fp16 correlations 1.9e-3 | 1.9e-3 (one fp16 rounding of values up to 5), oracle 2.6e-4
                        streamed fp16 volume 2.5e-3 | 2.5e-3, as fp32 / split 1.5e-3 | 1.5e-3       gathered fp16 volume 1.7e-3 | 1.7e-3
                        (the largest fp32 figures are those of the 192 pixel wide zoom shapes; without them: entropy 4.0e-5 | 8.0e-5, oracle
                        5.9e-5, volume 5.8e-5 | 8.7e-5, oracle 9.6e-5)
      far-world rigs    entropy 3.3e-4 | 3.3e-4, oracle 1.7e-3 | 2.3e-3 volume 3.3e-4 | 3.2e-4, oracle 1.8e-3 | 2.2e-3
                        exact kept correlations 4.7e-4 | 4.5e-4, oracle 2.6e-3 | 2.1e-3  kept fp16 correlations 1.7e-3 | 1.7e-3
    (the oracle runs on the host: its far-world figures depend on the host's LAPACK inverse).  Worst error / allowed over every comparison
    0.74 | 0.74 (kept fp16 correlations); fp32 outputs: 0.44 | 0.56.  On the far-world rigs the kernels are 5 x closer to fp64 than the oracle."""
    import rig_cases as RC
    import warp_ref as R64
    r = RC.reference(name, shape)
    cams, hyp, feats, vis = r["cams"], r["hyp"], r["feats"], r["vis"]
    B, V, C, H, W = feats.shape
    D = hyp.shape[1]
    info, figs = (name, shape), {}
    f_dev, hd, vd, hom = dev(feats, device), dev(hyp, device), dev(vis, device), ops.compose_homography(dev(cams, device))
    lds = ops.gather_keeps_correlations(f_dev, 8, hd)
    assert lds == (W % 8 == 0), (info, "which kernels take this shape")
    got = _gather_rig_outputs(device, feats, cams, hyp, vis, lds)
    inc = r["inc"]                                        # [B,V-1,D,H,W]
    inc_all = inc.all(1)[:, None]                         # volume voxels: every view's sample is comparable
    inc_px = inc.all(2)                                   # entropy pixels [B,V-1,H,W]: every plane is comparable
    if D <= 8 and not RC.RIGS[name].get("singular"):      # up to D = 8 every view's entropy is value-checked on a quarter of its pixels
        assert float(inc_px.double().mean((0, 2, 3)).min()) >= 0.25, (info, "entropy pixels compared per view", inc_px.double().mean((0, 2, 3)))
    vscale = max(1.0, float(r["vol64"].abs().max()))
    cscale = max(1.0, float(r["corr64"].abs().max()))
    inc_c = inc[:, :, None]
    _rig_check(figs, "gather: entropy", got["ent"], r["ent64"], r["ent32"], 5e-5, inc_px, info)
    _rig_check(figs, "gather: volume", got["vol"], r["vol64"], r["vol32"], 5e-5 * vscale, inc_all, info)
    if lds:
        _rig_check(figs, "gather: entropy, fp16 window", got["ent_w16"], r["ent64_16"], r["ent32_16"], 5e-5, inc_px, info)
        _rig_check(figs, "gather: entropy, keeping pass", got["ent_keep"], r["ent64_16"], r["ent32_16"], 5e-5, inc_px, info)
        _rig_check(figs, "gather: kept fp16 correlations", got["corr_keep"], r["corr64_16"], r["corr32_16"], 6e-4 * cscale, inc_c, info)
        _rig_check(figs, "gather: fp16 volume", got["vol_f16"], r["vol64_16"], r["vol32_16"], 1.2e-3 * vscale, inc_all, info)
        _rig_check(figs, "gather: streamed fp16 volume", got["agg_f16"], r["vol64_16"], r["vol32_16"], 1.2e-3 * vscale, inc_all, info)
        _rig_check(figs, "gather: streamed volume, fp32 out", got["agg_f32"], r["vol64_16"], r["vol32_16"], 6e-4 * vscale, inc_all, info)
        _rig_check(figs, "gather: streamed volume, split out", got["agg_split"], r["vol64_16"], r["vol32_16"], 6e-4 * vscale, inc_all, info)
        if D > 4:
            _rig_check(figs, "gather: entropy, exact keeping pass", got["ent_exact"], r["ent64"], r["ent32"], 5e-5, inc_px, info)
            _rig_check(figs, "gather: exact kept correlations", got["corr_exact"], r["corr64"], r["corr32"], 5e-5 * cscale, inc_c, info)
            _rig_check(figs, "gather: exact streamed volume", got["agg_exact"], r["vol64"], r["vol32"], 5e-5 * vscale, inc_all, info)
            _rig_check(figs, "gather: exact streamed volume, split", got["agg_exact_split"], r["vol64"], r["vol32"], 5e-5 * vscale, inc_all, info)
            assert (got["agg_exact"] - got["vol"]).abs().max() <= 4e-6 * vscale, (info, "exact streamed volume == second gather")
        if RC.RIGS[name].get("singular"):
            far = r["far_px"][:, :, None].expand_as(got["corr_keep"])
            assert far[:, 0, :, 3].all(), "the planted plane projects beyond 1e4 px everywhere"
            assert float(got["corr_keep"][far].abs().max()) == 0.0 and float(got["corr_exact"][far].abs().max()) == 0.0, (info, "kept correlations on the singular planes")
        # the octet-tiled hand-offs: fp32 tiles give the planar numbers, fp16 tiles the bits of planar fp16 features
        pk = ops.pack_features(f_dev)
        assert torch.equal(cpu(pk.unpack()), feats), "pack_features must be a pure re-layout"
        ent_t = cpu(ops.warp_corr_entropy(pk, ops._feat(pk)[1], hom, hd, 8))
        vol_t = _cl(ops.warp_corr_aggregate(pk, ops._feat(pk)[1], hom, hd, vd, 8)[0])
        _rig_check(figs, "gather: entropy, fp32 tiles", ent_t, r["ent64"], r["ent32"], 5e-5, inc_px, info)
        _rig_check(figs, "gather: volume, fp32 tiles", vol_t, r["vol64"], r["vol32"], 5e-5 * vscale, inc_all, info)
        assert (ent_t - got["ent"]).abs().max() <= 1e-6 and (vol_t - got["vol"]).abs().max() <= 1e-6 * vscale, (info, "tiled == planar")
        fh = dev(feats.half(), device)
        ft16 = ops.pack_features(fh)
        assert ft16.dtype == torch.float16
        e_p, c_p = ops.warp_corr_entropy_keep(fh, ops._feat(fh)[1], hom, hd, 8)
        e_t, c_t = ops.warp_corr_entropy_keep(ft16, ops._feat(ft16)[1], hom, hd, 8)
        assert torch.equal(cpu(e_p), cpu(e_t)) and torch.equal(cpu(c_p), cpu(c_t)), (info, "fp16 tiles == planar fp16: keeping pass")
        v_p = ops.warp_corr_aggregate(fh, ops._feat(fh)[1], hom, hd, vd, 8, f16=True)[0]
        v_t = ops.warp_corr_aggregate(ft16, ops._feat(ft16)[1], hom, hd, vd, 8, f16=True)[0]
        assert torch.equal(cpu(v_p), cpu(v_t)), (info, "fp16 tiles == planar fp16: pass 2")
        w_p = ops.warp_corr_entropy(fh, ops._feat(fh)[1], hom, hd, 8, f16_window=True)
        w_t = ops.warp_corr_entropy(ft16, ops._feat(ft16)[1], hom, hd, 8, f16_window=True)
        assert torch.equal(cpu(w_p), cpu(w_t)), (info, "fp16 tiles == planar fp16: plain pass 1")
        # fp16 tiles against fp64: here the reference view's features are fp16-rounded as well
        f16 = feats.half().float()
        _, corr64_h, ent64_h = R64.aggregate64(f16, cams, hyp, vis, 8)
        _, corr32_h, ent32_h, _ = RC.oracle32(f16, cams, hyp, vis)
        _rig_check(figs, "gather: entropy, fp16 tiles", e_t, ent64_h, ent32_h, 5e-5, inc_px, info)
        _rig_check(figs, "gather: kept correlations, fp16 tiles", cpu(c_t).float().permute(0, 1, 5, 2, 3, 4), corr64_h, corr32_h, 6e-4 * cscale, inc_c, info)
    # per-view partial sums == the fused form
    f, code = ops._feat(f_dev)
    parts = [ops.warp_corr_aggregate(f, code, hom, hd, vd, 8, normalise=False, view_begin=v, view_end=v + 1) for v in range(1, V)]
    both = ops.volume_normalise_(sum(p[0] for p in parts), sum(p[1] for p in parts))
    assert (_cl(both) - got["vol"]).abs().max() <= 2e-6 * vscale, (info, "partial sums")
    if B > 1:       # a batch of different rigs: every element equals its own B = 1 run, bit for bit
        for b in range(B):
            one = _gather_rig_outputs(device, feats[b:b + 1], cams[b:b + 1], hyp[b:b + 1], vis[b:b + 1], lds)
            for k in got:
                assert torch.equal(one[k][0], got[k][b]), (info, "batch element %d differs from its own B = 1 run" % b, k)
    _print_figures("case_gather_rigs %s %s" % info, figs)


def case_aggregate_backward_rigs(device, name, shape):
    """mvs_warp_corr_aggregate_bwd on roll90 / convergent / zoom (factor 2) / forward against fp64 autograd through warp_ref, at (8, 4, 12, 20)
    and (32, 6, 10, 16).  Bar: 3e-5 of the gradient's max, or 3 x the error of fp32 autograd through the oracle.  Voxels within depth/32 of
    a source's camera plane get a zero upstream gradient (a feature gradient sums over voxels, so they cannot be left out afterwards).  At
    D = 4 the forward rig's source 1 sits at z = 680 instead of 600: at 600 one whole plane of the four lies within depth/32 of its camera
    plane, which is more than the 10 % the excluded set may hold; two of the four planes are still behind that camera, and the rig
    conditions are asserted at these shapes too: 25 % of the voxels behind source 1, 0.5 % behind it AND inside its image, the latter also
    counted among the voxels with a non-zero upstream gradient.
    Measured over the 8 cases, relative to the gradient's max (emulator | MI355X, then fp32 autograd through the oracle): feature gradient
    3.0e-6 | 3.0e-6, oracle 2.9e-6; visibility gradient 7.2e-6 | 6.1e-6, oracle 4.2e-6; worst error / allowed 0.24 | 0.20."""
    import rig_cases as RC
    import warp_ref as R64
    C, D, H, W = shape
    g = torch.Generator().manual_seed(C + D + len(name))
    zc = 680.0 if (name == "forward" and D == 4) else 600.0
    cams = RC.make_rig(name, H, W, forward_z=zc)[None]
    V = cams.shape[1]
    hyp = RC.make_hyp(D, H, W, 1.0, g)
    feats = torch.randn(1, V, C, H, W, generator=g)
    vis = torch.rand(1, V - 1, H, W, generator=g) * 0.9 + 0.05
    hom64 = R64.homography64(cams)
    excl = torch.stack([hyp.double() > 32 * R64.project64(hom64[:, v], hyp, H, W)[2].abs() for v in range(V - 1)], 1)
    for v in range(V - 1):
        share = float(excl[:, v].double().mean())
        assert share <= 0.10 and (name == "forward" or share == 0.0), (name, shape, v, "excluded share", share)
    if name == "forward":      # the conditions of rig_cases.rig_conditions at this shape: the mirrored taps do reach the gradients
        xn, yn, pz = R64.project64(hom64[:, 0], hyp, H, W)
        ix, iy = (xn + 1) / 2 * (W - 1), (yn + 1) / 2 * (H - 1)
        inside = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
        assert float((pz <= 0).double().mean()) >= 0.25, "planes behind source 1"
        assert float(((pz <= 0) & inside).double().mean()) >= 0.005, ("behind source 1 AND inside its image", float(((pz <= 0) & inside).double().mean()))
        assert float(((pz <= 0) & inside & ~excl[:, 0]).double().mean()) >= 0.005, "... with a non-zero upstream gradient"
    gvol = torch.randn(1, 8, D, H, W, generator=g) * (~excl.any(1))[:, None]
    # fp64 autograd through the restatement, and fp32 autograd through the oracle for the bar
    f64, v64 = feats.double().requires_grad_(True), vis.double().requires_grad_(True)
    vol64 = R64.aggregate64(f64, cams, hyp, v64, 8)[0]
    (vol64 * gvol.double()).sum().backward()
    f32, v32 = feats.clone().requires_grad_(True), vis.clone().requires_grad_(True)
    ref_p, vol_sum, vis_sum = O.compose_proj(cams[:, 0]), 0.0, 0.0
    for v in range(1, V):
        warped, _ = O.homo_warping_3D_with_mask(f32[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
        vol_sum = vol_sum + O.group_correlation(f32[:, 0], warped, 8) * v32[:, v - 1].unsqueeze(1).unsqueeze(1)
        vis_sum = vis_sum + v32[:, v - 1]
    (vol_sum / (vis_sum.unsqueeze(1).unsqueeze(1) + 1e-6) * gvol).sum().backward()
    fd, code = ops._feat(dev(feats, device))
    hom = ops.compose_homography(dev(cams, device))
    vol_cl, _ = ops.warp_corr_aggregate(fd, code, hom, dev(hyp, device), dev(vis, device), 8)
    gfeat, gvis = ops.warp_corr_aggregate_bwd(fd, code, hom, dev(hyp, device), dev(vis, device), dev(vis.sum(1), device), vol_cl,
                                              dev(gvol.permute(0, 2, 3, 4, 1).contiguous(), device), 8)
    sf, sv = float(f64.grad.abs().max()), float(v64.grad.abs().max())
    figs = {}
    _rig_check(figs, "backward: feature gradient / max", cpu(gfeat) / sf, f64.grad / sf, f32.grad / sf, 3e-5, None, (name, shape))
    _rig_check(figs, "backward: visibility gradient / max", cpu(gvis) / sv, v64.grad / sv, v32.grad / sv, 3e-5, None, (name, shape))
    assert float(cpu(gfeat)[:, 1:].abs().sum()) > 0 and float(cpu(gfeat)[:, 0].abs().sum()) > 0
    _print_figures("case_aggregate_backward_rigs %s %s" % (name, shape), figs)


def case_cascade_rigs(device, name, conv_precision=None):
    """A whole CascadeDepthHead at 64 x 128, V = 3, on a near-world rig against O.cascade_forward (the fp32 oracle is the comparator here,
    so the far-world rigs do not qualify): the bars of case_cascade_vs_oracle - 1e-3 depth rel-L1 per stage and refined, the same
    confidence bar - with the fp16-tile hand-off leg in the default precision.
    Measured refined-depth rel-L1 (emulator | MI355X): default precision convergent 3.7e-5 | 3.5e-5, roll90 3.6e-5 | 3.7e-5, zoom 4.1e-5 | 3.9e-5;
    bf16x3 6.0e-7 .. 8.9e-7 | 5.4e-7 .. 9.8e-7."""
    import rig_cases as RC
    r = case_cascade_vs_oracle(device, 64, 128, 3, conv_precision=conv_precision, cams=RC.make_rig(name, 64, 128)[None])
    print("\ncase_cascade_rigs %s %s: refined depth rel-L1 vs the oracle %.2e" % (name, eff(conv_precision), r))
    return r
