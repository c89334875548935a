"""CPU: the native DINOv2MVSNet (mvsformerplusplus_amd.network) and its two glue kernels (csrc/resize_kernels.hip) on the host emulator:
the kernels against fp64 F.interpolate, the whole module against fixture F29 (the reference's own network, tests/golden/
make_golden_network.py), the module contract (state-dict names, load_checkpoint, patch_network) and every refusal.

Bars (the project's own, none derived here): LAYER_BAR x max(1, max|ref|) for one entry point; MODULE_BAR of a tensor's range for the
bicubic output, conv31 after the add and each stage's features; depth relative L1 <= 1e-3 (the README's bar); confidence within
tests/test_dropin_reference.py's bound for the default precision policy.  Measured on the emulator: resize_bicubic 4.4e-7 .. 1.1e-6 and
resize_bilinear_add 4.4e-8 .. 1.0e-7 x max(1, max|ref|) against fp64 (ATen's own fp32 bicubic kernel: 1.5e-4 at 320 -> 140 columns, because
it rounds the source coordinate in fp32; the kernel evaluates it exactly).  F29 case c: bicubic output 4.1e-6 and conv31 1.2e-5 of the
range, features 6.6e-6 .. 9.6e-6, depth relative L1 6.9e-6 .. 3.2e-5 (worst pixel 3.1e-4), confidence <= 1.0e-3.  On an MI355X
(tests/test_network_gpu.py): cases a, b, c features 5.9e-6 .. 1.2e-5, depth 2.8e-6 .. 5.0e-5, confidence <= 2.0e-3.  The tests print what
they measured (pytest -s)."""
import glob
import hashlib
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden, rel_l1
from mvsformerplusplus_amd import DINOv2MVSNet, _lib, checkpoint_state_dict, ops, patch_network, synth
from mvsformerplusplus_amd.cascade import CascadeDepthHead

LAYER_BAR = 3e-5          # per entry point: x max(1, max|ref|)          (tests/test_fpn.py, tests/test_fmt.py, tests/test_vit.py)
MODULE_BAR = 2e-4         # module outputs: x the tensor's range
DEPTH_BAR = 1e-3          # relative L1 of every stage's depth and of refined_depth (README)
CONF_BAR = 3e-2           # absolute, the default policy's bound of tests/test_dropin_reference.py

BICUBIC_CASES = [((2, 3, 32, 64), (28, 56)), ((3, 3, 96, 128), (28, 28)), ((1, 3, 20, 24), (42, 70)), ((1, 3, 2, 3), (14, 14)),
                 ((1, 3, 192, 320), (84, 140))]
BILINEAR_CASES = [((3, 64, 8, 8), (12, 16)), ((2, 64, 8, 16), (4, 8)), ((2, 64, 3, 2), (9, 11)), ((1, 64, 5, 7), (5, 7))]
F29_CASES = {"a": (64, 64, 3, 0.4375, (28, 28), (8, 8)), "b": (96, 128, 3, 0.3, (28, 28), (12, 16)), "c": (32, 64, 2, 1.0, (28, 56), (4, 8))}
STAGES = ("stage1", "stage2", "stage3", "stage4")
_FX = {}


# ---- the glue kernels -------------------------------------------------------------------------------------------------------------------
def layer_error(got, want, what):
    err = float((got.double().cpu() - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous() and err <= LAYER_BAR * scale, (what, err, LAYER_BAR * scale)
    return err / scale


def check_bicubic(shape, size, device):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape) + sum(size)))
    want = F.interpolate(x.double(), size, mode="bicubic", align_corners=False)
    return layer_error(ops.resize_bicubic(x.to(device), *size), want, ("bicubic", shape, size))


def check_bicubic_view(device):
    """A [B V, 3, H, W] view of [B, V, 3, H, W] and a view with strided rows and columns are read in place."""
    big = torch.randn(2, 3, 3, 40, 66, generator=torch.Generator().manual_seed(7)).to(device)
    worst = 0.0
    for v, size in ((big[1], (14, 28)), (big[0][:, :, 1::2, 2::3], (14, 28)), (big.permute(0, 2, 1, 3, 4)[1], (28, 42))):
        assert not v.is_contiguous() or v.data_ptr() != big.data_ptr()
        want = F.interpolate(v.double().cpu(), size, mode="bicubic", align_corners=False)
        worst = max(worst, layer_error(ops.resize_bicubic(v, *size), want, ("bicubic view", tuple(v.shape), v.stride())))
    return worst


def check_bilinear_add(shape, size, device):
    g = torch.Generator().manual_seed(sum(shape) + sum(size))
    x, base = torch.randn(*shape, generator=g), torch.randn(shape[0], shape[1], *size, generator=g)
    want = base.double() + F.interpolate(x.double(), size, mode="bilinear", align_corners=False)
    got = ops.resize_bilinear_add(base.to(device), x.to(device))
    err = layer_error(got, want, ("bilinear add", shape, size))
    if tuple(shape[2:]) == tuple(size):
        assert torch.equal(got.cpu(), base + x)                                    # the product's case: bit for bit
        xs = torch.randn(shape[0], shape[1], size[0], 2 * size[1], generator=g)[..., ::2]
        assert torch.equal(ops.resize_bilinear_add(base.to(device), xs.to(device)).cpu(), base + xs)       # a strided x as well
    return err


@pytest.mark.parametrize("shape,size", BICUBIC_CASES)
def test_resize_bicubic(emu, shape, size):
    print("resize_bicubic %s -> %s: %.3g x max(1, max|ref|) (bar %g)" % (shape, size, check_bicubic(shape, size, emu), LAYER_BAR))


def test_resize_bicubic_reads_views_in_place(emu):
    print("resize_bicubic on strided views: %.3g x max(1, max|ref|)" % check_bicubic_view(emu))


@pytest.mark.parametrize("shape,size", BILINEAR_CASES)
def test_resize_bilinear_add(emu, shape, size):
    print("resize_bilinear_add %s -> %s: %.3g x max(1, max|ref|) (bar %g)" % (shape, size, check_bilinear_add(shape, size, emu), LAYER_BAR))


def test_resize_refusals(emu):
    x = torch.zeros(1, 3, 8, 8)
    for bad in (x.double(), x[0], torch.zeros(1, 3, 0, 8)):
        with pytest.raises(ValueError, match="fp32 tensor"):
            ops.resize_bicubic(bad, 4, 4)
    with pytest.raises(ValueError, match="at least 1 x 1"):
        ops.resize_bicubic(x, 0, 4)
    with pytest.raises(ValueError, match="agree in N, C"):
        ops.resize_bilinear_add(torch.zeros(1, 4, 8, 8), x)
    with pytest.raises(_lib.MvsHipError, match="N \\* C <= 65535"):
        ops.resize_bicubic(torch.zeros(1, 65536, 1, 1), 1, 1)


def test_resize_needs_a_device():
    """Without the emulator the binding refuses host tensors: there is no PyTorch fall-back behind the wrappers."""
    with pytest.raises(_lib.MvsHipError):
        ops.resize_bicubic(torch.zeros(1, 3, 8, 8), 4, 4)
    with pytest.raises(_lib.MvsHipError):
        ops.resize_bilinear_add(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 4, 4))


# ---- fixture F29 ------------------------------------------------------------------------------------------------------------------------
def f29():
    """Every array of tests/golden/f29_network_*.npz; arrays the generator split along the view axis ("key#part") are rejoined."""
    if "fx" not in _FX:
        fx, parts = {}, {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, "f29_network_*.npz"))):
            for k, v in load_golden(os.path.basename(path)).items():
                if "#" in k:
                    parts.setdefault(k.split("#")[0], {})[int(k.split("#")[1])] = v
                elif k != "__name__":
                    fx[k] = v
        for k, d in parts.items():
            fx[k] = torch.cat([d[i] for i in range(len(d))], 1)
        _FX["fx"] = fx
    return _FX["fx"]


def f29_args(**changes):
    if "args" not in _FX:
        _FX["args"] = json.load(open(os.path.join(GOLDEN, "f29_network_args.json")))
    return dict(json.loads(json.dumps(_FX["args"])), **changes)


def f29_manifest():
    fx = f29()
    return {k: tuple(json.loads(s)) for k, s in zip(fx["net.keys"], fx["net.shapes"])}


def f29_weights():
    """The state dict F29 was generated with: manifest + seed and the two overrides stored in F29 as JSON (seeded N(0, 1) values for the
    "normal" keys, synth's draw times a factor for the "scale" prefixes), checked against the SHA-256 stored in F29."""
    if "sd" not in _FX:
        fx, man = f29(), f29_manifest()
        sd = synth.seeded_state_dict(man, int(fx["net.seed"]))
        rule = json.loads(fx["net.overrides"])
        g = torch.Generator().manual_seed(int(fx["net.override_seed"]))
        for key in rule["normal"]:
            sd[key] = torch.randn(man[key], generator=g)
        for key in man:
            for prefix, factor in rule["scale"].items():
                if key.startswith(prefix):
                    sd[key] = sd[key] * factor
        h = hashlib.sha256()
        for k in sorted(sd):
            h.update(k.encode())
            h.update(sd[k].contiguous().numpy().tobytes())
        assert h.hexdigest() == fx["net.sha256"], "torch / numpy generator changed: regenerate F29 (tests/golden/make_golden_network.py)"
        _FX["sd"] = sd
    return _FX["sd"]


def network(device="cpu", **changes):
    net = DINOv2MVSNet(f29_args(**changes))
    net.load_state_dict(f29_weights(), strict=True)
    return net.eval().to(device)


def shared_network(device, rescale):
    """ONE network per device for every F29 case (126 M parameters: built and packed once); `rescale` is the only setting the cases change
    and the module reads it per call."""
    key = ("net", str(device))
    if key not in _FX:
        _FX[key] = network(device)
    _FX[key].rescale = rescale
    return _FX[key]


def case_inputs(name, device):
    fx = f29()
    return (fx[name + "/imgs"].to(device), {k: fx["%s/proj.%s" % (name, k)].to(device) for k in STAGES}, fx[name + "/depth_values"].to(device))


def run_captured(net, imgs, projs, dv):
    """net(imgs, projs, dv) plus what the forward passed on the way: (outputs, {"vit_imgs", "conv31", "feat"})."""
    cap = {}
    inner = net.feature_maps

    def spy(x):
        cap["feat"] = inner(x, capture=cap)
        return cap["feat"]

    net.feature_maps = spy
    try:
        with torch.no_grad():
            out = net(imgs, projs, dv)
    finally:
        del net.feature_maps
    return out, cap


def within_range(got, want, what):
    frac = float((got.double().cpu() - want.double()).abs().max()) / float(want.max() - want.min())
    assert got.shape == want.shape and frac <= MODULE_BAR, (what, tuple(got.shape), tuple(want.shape), frac, MODULE_BAR)
    return frac


def check_case(name, device, net=None):
    """F29 case `name` through the whole module on `device` -> the measured figures; every bar of this file is asserted."""
    fx = f29()
    H, W, V, rescale, vit_size, c31_size = F29_CASES[name]
    net = shared_network(device, rescale) if net is None else net
    assert float(fx[name + "/rescale"]) == rescale and net.vit_size(H, W) == vit_size
    out, cap = run_captured(net, *case_inputs(name, device))
    p = name + "/"
    assert sorted(out.keys()) == fx[p + "out_names"]
    assert cap["vit_imgs"].shape == (V, 3) + vit_size and cap["conv31"].shape == (V, 64) + c31_size
    m = {"vit_imgs": within_range(cap["vit_imgs"], fx[p + "vit_imgs"], (name, "vit_imgs")),
         "conv31": within_range(cap["conv31"], fx[p + "conv31"], (name, "conv31")), "feat": [], "depth": [], "depth_max": [], "conf": []}
    for k in STAGES:
        m["feat"].append(within_range(cap["feat"][k], fx[p + "feat." + k], (name, k)))
        d, want = out[k]["depth"].cpu(), fx[p + k + ".depth"]
        m["depth"].append(rel_l1(d, want))
        m["depth_max"].append(float(((d - want).abs() / want.abs()).max()))
        m["conf"].append(float((out[k]["photometric_confidence"].cpu() - fx[p + k + ".conf"]).abs().max()))
    m["depth"].append(rel_l1(out["refined_depth"].cpu(), fx[p + "refined_depth"]))
    m["conf"].append(float((out["photometric_confidence"].cpu() - fx[p + "photometric_confidence"]).abs().max()))
    print("F29 case %s on %s: bicubic %.3g, conv31 %.3g, features %s of each range (bar %g); depth relative L1 %s, last = refined (bar %g; "
          "worst pixel per stage %s); confidence %s (bar %g)"
          % (name, device, m["vit_imgs"], m["conv31"], ["%.3g" % f for f in m["feat"]], MODULE_BAR, ["%.3g" % f for f in m["depth"]], DEPTH_BAR,
             ["%.3g" % f for f in m["depth_max"]], ["%.3g" % f for f in m["conf"]], CONF_BAR))
    assert torch.equal(out["refined_depth"], out["stage4"]["depth"])
    assert max(m["depth"]) <= DEPTH_BAR and max(m["conf"]) <= CONF_BAR, m
    _FX[("out", name, str(device))] = out
    return m


@pytest.mark.parametrize("name", ["c", pytest.param("a", marks=pytest.mark.slow), pytest.param("b", marks=pytest.mark.slow)])
def test_f29_case(emu, name):
    """Case c takes about 75 s on the emulator, a and b about 150 s each (marked slow; the GPU file runs all three)."""
    check_case(name, emu)


# ---- module contract --------------------------------------------------------------------------------------------------------------------
def test_state_dict_is_the_reference_s():
    """779 keys under the six prefixes, in the reference's order and with its shapes (F29 stores the reference model's manifest),
    126 054 413 parameters; the seeded state dict loads with strict=True and round-trips unchanged."""
    man = f29_manifest()
    net = DINOv2MVSNet(f29_args())
    sd = net.state_dict()
    assert len(man) == 779 and list(sd.keys()) == list(man.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == man
    assert {k.split(".")[0] for k in sd} == {"encoder", "decoder", "vit", "decoder_vit", "FMT_module", "fusions"}
    assert sum(p.numel() for p in net.parameters()) == 126054413 == int(f29()["net.parameters"])
    assert isinstance(net, CascadeDepthHead) and net.rescale == 0.4375 and net.vit_size(1152, 1536) == (504, 672)
    want = f29_weights()
    net.load_state_dict(want, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_load_checkpoint(tmp_path):
    """A released checkpoint as test.py:213-220 reads it: checkpoint["state_dict"], "module." stripped, pe_dict entries skipped."""
    want = f29_weights()
    ck = {"state_dict": {"module." + k: v for k, v in want.items()}, "epoch": 3}
    ck["state_dict"]["module.fusions.0.cost_reg.pe_dict.4-8-8"] = torch.zeros(3)
    sd = checkpoint_state_dict(ck)
    assert list(sd.keys()) == list(want.keys()) and all(sd[k] is want[k] for k in want)
    plain = checkpoint_state_dict({"state_dict": dict(want)})                      # saved without DataParallel: no prefix
    assert list(plain.keys()) == list(want.keys())
    path = tmp_path / "model_best.pth"
    torch.save(ck, path)
    net = DINOv2MVSNet(f29_args())
    assert net.load_checkpoint(str(path)) is net
    for k, v in net.state_dict().items():
        assert torch.equal(v, want[k]), k
    with pytest.raises(ValueError, match="state_dict"):
        checkpoint_state_dict({"model": {}})
    broken = dict(ck["state_dict"])
    del broken["module.vit.cls_token"]
    with pytest.raises(RuntimeError, match="vit.cls_token"):
        DINOv2MVSNet(f29_args()).load_checkpoint({"state_dict": broken})


REFERENCE = os.environ.get("MVS_REFERENCE", "/root/reference")


def test_patch_network_on_a_live_reference_model(emu):
    """patch_network(reference instance) = DINOv2MVSNet(args) + load_state_dict: the same outputs bit for bit on F29 case c, the reference
    model left as it was, eval mode whatever the instance's mode."""
    if not os.path.isfile(os.path.join(REFERENCE, "models", "networks", "DINOv2_mvsformer_model.py")):
        pytest.skip("the reference tree is not on this machine")
    sys.path.append(REFERENCE)
    try:
        from models.networks.DINOv2_mvsformer_model import DINOv2MVSNet as RefNet
        ref = RefNet(f29_args(rescale=1.0))                      # case c's setting: its forward is shared with test_f29_case[c]
    finally:
        sys.path.remove(REFERENCE)
    ref.load_state_dict(f29_weights(), strict=True)
    ref.train()
    net = patch_network(ref)
    assert isinstance(net, DINOv2MVSNet) and not net.training and ref.training and type(ref.vit).__module__.startswith("models.")
    assert net.args == ref.args and net.args is not ref.args and net.rescale == 1.0
    other = shared_network(emu, 1.0)
    for (k, v), (k2, v2) in zip(net.state_dict().items(), other.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    with torch.no_grad():
        a = net(*case_inputs("c", emu))
        b = _FX.get(("out", "c", emu)) or other(*case_inputs("c", emu))             # test_f29_case[c]'s run, when it came first
    assert sorted(a) == sorted(b)
    for k in ("refined_depth", "photometric_confidence", "prob_volume", "depth_values"):
        assert torch.equal(a[k], b[k]), k
    for k in STAGES:
        assert torch.equal(a[k]["depth"], b[k]["depth"]) and torch.equal(a[k]["photometric_confidence"], b[k]["photometric_confidence"]), k
    with pytest.raises(TypeError, match="DINOv2MVSNet"):
        patch_network(torch.nn.Linear(2, 2))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def small_inputs(B=1, V=2, H=32, W=32):
    projs = synth.stage_proj_matrices(synth.make_cameras(V, H, W, baseline=30.0, rot_deg=1.0, seed=1, batch=B), 4)
    return torch.rand(B, V, 3, H, W), projs, torch.arange(425.0, 425.0 + 2.65 * 191.5, 2.65)[None].repeat(B, 1)


def test_refusals(emu):
    """B > 1, train mode, inputs that require grad, sizes: each a clear error before any kernel runs."""
    net = DINOv2MVSNet(f29_args()).eval()
    with pytest.raises(NotImplementedError, match="B = 2"):
        net(*small_inputs(B=2))
    with pytest.raises(ValueError, match=r"\[1, V, 3, H, W\]"):
        net(torch.rand(2, 3, 32, 32), *small_inputs()[1:])
    imgs, projs, dv = small_inputs()
    with pytest.raises(RuntimeError, match="patch_all"):
        net(imgs.clone().requires_grad_(True), projs, dv)
    with pytest.raises(RuntimeError, match="patch_all"):
        net(imgs, projs, dv.clone().requires_grad_(True))
    with torch.no_grad():
        with pytest.raises(ValueError, match="multiples of 8"):
            net(*small_inputs(H=36, W=32))
        with pytest.raises(ValueError, match="one 14 x 14 patch"):
            net(*small_inputs(H=24, W=64))
        with pytest.raises(NotImplementedError, match="torch.cuda.graph"):
            net.capture()
    net.train()
    with pytest.raises(RuntimeError, match="patch_all"):
        net(imgs, projs, dv)
    with pytest.raises(RuntimeError, match="patch_all"):
        net.feature_maps(imgs)
    with pytest.raises(NotImplementedError, match="feat_chs"):
        DINOv2MVSNet(f29_args(feat_chs=[8, 16, 32, 48]))


def test_a_size_a_sub_module_refuses(emu):
    """40 x 64 passes the network's own checks (multiples of 8, one patch) but stage 1 is 5 x 8 and the stage-1 transformer's down_rate is
    (2, 4, 4): the sub-module's error comes through as it is.  A 3-block ViT keeps the emulated run short."""
    args = f29_args()
    args["dino_cfg"] = dict(args["dino_cfg"], depth=3)
    net = DINOv2MVSNet(args)
    net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 3), strict=True)
    with torch.no_grad(), pytest.raises(ValueError, match="down_rate"):
        net.eval()(*small_inputs(H=40, W=64))


def test_host_tensors_are_refused():
    """Product behaviour (no emulator): host tensors raise, and so does a mix of devices - nothing falls back to PyTorch arithmetic."""
    net = DINOv2MVSNet(f29_args()).eval()
    with torch.no_grad(), pytest.raises(_lib.MvsHipError, match="ROCm device"):
        net(*small_inputs())
    with torch.no_grad(), pytest.raises(_lib.MvsHipError, match="ROCm device"):
        net.feature_maps(small_inputs()[0])
