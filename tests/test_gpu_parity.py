"""-m gpu: parity of the real gfx950 library (through the C ABI) against the oracle and the golden vectors."""
import os

import pytest
import torch

import parity_cases as P
import rig_cases as RC
from conftest import PRECS, PRECS_ALL, rel_l1      # PRECS = [None (the product default: the "stagemix" policy), "bf16x3" (the fp32-equivalent mode)]

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    from mvsformerplusplus_amd import _lib
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    assert os.path.exists(_lib.LIB_PATH), "libmvs_hip.so missing: python -m mvsformerplusplus_amd.build"
    _lib.lib()
    assert _lib._REQUIRE_DEVICE
    yield


@pytest.mark.parametrize("tag", ["a", "b"])
def test_warp_golden(tag):
    P.case_warp_golden(DEV, tag)


def test_warp_dtypes():
    P.case_warp_dtypes(DEV)


def test_warp_siblings():
    P.case_warp_siblings(DEV)


def test_precisions():
    P.case_precisions(DEV)


@pytest.mark.parametrize("prec", PRECS)
def test_single_layers(prec):
    P.case_single_layers(DEV, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["f3_costregnet.npz", "f3_costregnet3d_d4.npz", "f3_costregnet3d_d8.npz"])
def test_regnet_golden(name, prec):
    P.case_regnet_golden(DEV, name, prec)


def test_generic_conv_layers():
    P.case_generic_conv_layers(DEV)


def test_regnet_generic_golden():
    P.case_regnet_generic_golden(DEV)


def test_costregnet2d_golden():
    P.case_costregnet2d_golden(DEV)


def test_position_encoding_golden():
    P.case_position_encoding_golden(DEV)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", ["g4_s1", "g4_s3", "g16_s2"])
def test_stage_other_groups_golden(tag, prec):
    P.case_stage_other_groups_golden(DEV, tag, prec)


@pytest.mark.parametrize("G", [4, 2])
def test_cascade_other_groups_vs_oracle(G):
    P.case_cascade_other_groups_vs_oracle(DEV, G=G)


def test_stage_pieces():
    P.case_stage_pieces(DEV)


@pytest.mark.parametrize("prec", PRECS_ALL)
@pytest.mark.parametrize("tag", ["s1", "s3"])
def test_stage_golden(tag, prec):
    P.case_stage_golden(DEV, tag, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_stage_bd_hypotheses(prec):
    """[B, D] hypotheses vs fixture F14 generated from the reference."""
    P.case_stage_bd_hypotheses(DEV, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_stage_modes(prec):
    P.case_stage_modes(DEV, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_stage_lowp_features(prec):
    P.case_stage_lowp_features(DEV, prec)


def test_small_fns():
    P.case_small_fns(DEV)


def test_auto_policy():
    P.case_auto_policy(DEV)


def test_feature_heads():
    P.case_feature_heads(DEV)


def test_fused_small_launches():
    P.case_fused_small_launches(DEV)


def test_range_variants():
    P.case_range_variants(DEV)


def test_generic_shapes():
    P.case_generic_shapes(DEV)


def test_vis_cnn():
    P.case_vis_cnn(DEV)


def test_gather_variants():
    P.case_gather_variants(DEV)


def test_gather_windows():
    P.case_gather_windows(DEV)


def test_split_format():
    P.case_split_format(DEV)


def test_f16_layers():
    P.case_f16_layers(DEV)


def test_f16_saturation():
    P.case_f16_saturation(DEV)


def test_f16_cascade():
    P.case_f16_cascade(DEV)


def test_slab_exchange_kernels():
    P.case_slab_exchange_kernels(DEV)


def test_aggregate_backward():
    P.case_aggregate_backward(DEV)


@pytest.mark.parametrize("tag", ["s3", "s1"])
def test_train_backward_golden(tag):
    P.case_train_backward_golden(DEV, tag)


def test_train_path_properties():
    P.case_train_path_properties(DEV)


def test_train_midsize_vs_cpu_autograd():
    P.case_train_midsize_vs_cpu_autograd(DEV)


@pytest.mark.parametrize("prec", PRECS_ALL)
def test_cascade_golden(prec):
    P.case_cascade_golden(DEV, prec)


def test_cpu_tensors_are_refused():
    """No CPU fallback: the product path must fail loudly when handed host tensors."""
    from mvsformerplusplus_amd import _lib, ops
    with pytest.raises(_lib.MvsHipError):
        ops.compose_homography(torch.zeros(1, 2, 2, 4, 4))


@pytest.mark.parametrize("prec", PRECS_ALL)
def test_cascade_midsize_vs_oracle(prec):
    """384x512, V=5, peaky logits (prob weights x30): final depth within 1e-3 relative L1 of the oracle - in the product default format
    (predicted 4e-4 by scripts/study_activation_precision.py) as in the fp32-equivalent one - and the plain set a decade below."""
    P.case_cascade_vs_oracle(DEV, 384, 512, 5, peaky=True, conv_precision=prec)
    assert P.case_cascade_vs_oracle(DEV, 384, 512, 5, peaky=False, conv_precision=prec) <= P.tol(prec, 1e-5, 2e-4)


@pytest.mark.parametrize("prec", PRECS)
def test_cascade_fullsize_properties(prec):
    """BASELINE configs[1] size (1152x1536, V=5): run-to-run determinism, finite outputs inside the hypothesis range, softmax sums,
    hypothesis ordering, view-order invariance of the aggregation (size-independent properties; the oracle is too slow to repeat here)."""
    P.case_cascade_fullsize_properties(DEV, conv_precision=prec)



def test_track_s_d192_fullsize():
    """SURVEY 8d Track S at its literal size (1152 x 1536, D = 192: an 11 GB volume) - round 5 lifted the 2 GB ceiling of the MFMA convolutions."""
    r = P.case_track_s_d192(DEV)
    print("Track S D=192 1152x1536: full run vs window run, depth rel-L1 %.2e" % r)

@pytest.mark.parametrize("prec", PRECS)
def test_baseline_cfg1_stage4_d48(prec):
    """BASELINE configs[0]: 640x512, V=3, D=48, stage-4-only StageNet (CostRegNet + the 3x3x3 head) vs the oracle."""
    r, pe = P.case_baseline_cfg1(DEV, prec)
    print("cfg1 %s: depth rel-L1 %.2e, prob_volume max abs %.2e" % (P.eff(prec), r, pe))


def test_baseline_cfg1_final_stage():
    """The same stand-alone stage with args["final_stage"]: the default policy's fp16 format, same bar."""
    r, pe = P.case_baseline_cfg1(DEV, None, final_stage=True)
    print("cfg1 final_stage (f16mix): depth rel-L1 %.2e, prob_volume max abs %.2e" % (r, pe))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["cfg3", "cfg4", "cfg5"])
def test_baseline_cfgs_small_vs_oracle(name, prec):
    """BASELINE configs[2..4] (V=10 / 1920x1088 V=11 D=256 / 2048x1536 V=11 D=384 fp16 features) at a reduced image size."""
    P.case_baseline_cfg_small(DEV, name, conv_precision=prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["cfg4", "cfg5"])
def test_baseline_cfgs_wide_range_vs_oracle(name, prec):
    """cfg4 / cfg5 on the literal 0.5 .. 10 hypothesis range, compared where the reference's own hypotheses stay finite."""
    P.case_baseline_cfg_wide_range(DEV, name, prec)


@pytest.mark.parametrize("prec", PRECS)         # full size: the product default and the fp32-equivalent format (28 s each, most of it the CPU oracle);
def test_cfg2_fullsize_vs_oracle(prec):         # "f16x2" / "f16" run the same comparison at 384x512 (test_cascade_midsize_vs_oracle)
    """BASELINE configs[1] at full size against the oracle (refined depth within 1e-3 relative L1, every stage too): the north-star bar
    itself, in the product default (measured 2.4e-6 since round 5's exact coarse stages; 4.7e-5 in round 4's uniform fp16) and in the fp32-equivalent format (~1e-6)."""
    r = P.case_cfg2_fullsize_vs_oracle(DEV, conv_precision=prec)
    assert r <= P.tol(prec, 1e-5, 3e-4), r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["cfg3", "cfg4", "cfg5"])
def test_baseline_cfgs_fullsize_properties(name, prec):
    """The same configs at their full image size through size-independent properties."""
    P.case_baseline_cfg_full(DEV, name, prec)


@pytest.mark.parametrize("attn", [None, "bf16x3"])
def test_transformer_golden(attn):
    """PureTransformerCostReg + get_position_3d vs fixture f7 (from the reference); None = the default attention
    precision ("attn16"), "bf16x3" = the fp32-equivalent attention of rounds 1-3."""
    P.case_transformer_golden(DEV, attn)


@pytest.mark.parametrize("attn", [None, "bf16x3"])
def test_stage_transformer_golden(attn):
    P.case_stage_transformer_golden(DEV, attn)


@pytest.mark.parametrize("prec,attn", [(None, None), ("bf16x3", "bf16x3"), (None, "bf16x3")])
def test_cascade_shipped_golden(prec, attn):
    """The shipped regulariser mix (cost_reg_type of config/mvsformer++.json) end to end vs fixture f9: product defaults (policy "stagemix": fp16 U-Nets on the fine stages,
    16-bit attention), everything fp32-equivalent, and the mixed case."""
    P.case_cascade_shipped_golden(DEV, conv_precision=prec, attention_precision=attn)


@pytest.mark.parametrize("n", [200, 4099])
def test_attention_stress(n):
    """Masked key tail + running-maximum rescales far into the key stream, vs float64 softmax attention."""
    P.case_attention_stress(DEV, n=n)


@pytest.mark.parametrize("n", [200, 4099])
def test_attention_stress_f16(n):
    """The same for the module default: fp16 q / k, bf16 p / v (csrc/attention_f16_kernels.hip)."""
    P.case_attention_stress(DEV, n=n, mode="attn16")


def test_attention_overflow():
    """The 16-bit attention's SAFE path: a score jump that overflows fp32 inside a key block (csrc/attention_f16_kernels.hip)."""
    P.case_attention_overflow(DEV)
    P.case_attention_overflow(DEV, n=4099)


def test_fusion_golden():
    """depth-map filters (static + dynamic) vs fixture f10 generated from misc/fusion.py."""
    P.case_fusion_golden(DEV)


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("H,W,kw", [(1152, 1600, {}), (1056, 1920, {"metres": True, "rot_deg": 4.0, "seed": 2}), (517, 743, {"seed": 3})],
                         ids=["dtu", "tt", "ragged"])
def test_fusion_scene_fp64(H, W, kw, dynamic):
    """The fused filter at the DTU / T&T output sizes and a size whose pixel count is not a multiple of 256 (517x743: the tail
    workgroup), 10 sources, against the fp64 restatement (parity_cases.fusion_vs_fp64)."""
    P.case_fusion_scene_fp64(DEV, H, W, 10, dynamic, **kw)


def test_fusion_batch():
    """n = 2 (blockIdx.y) through every entry point, per element against its own n = 1 run and the fp64 restatement."""
    P.case_fusion_batch(DEV, 517, 743, 10)


def test_fusion_view_limits():
    P.case_fusion_view_limits(DEV)


def test_fusion_thresholds_exact():
    P.case_fusion_thresholds_exact(DEV)


def test_attention_bf16p():
    """MVS_PREC_BF16P: bf16 softmax probabilities in p.v (optional fast mode of the transformer stage)."""
    P.case_attention_stress(DEV, n=4099, bf16p=True)
    P.case_stage_transformer_bf16p(DEV)


def test_cascade_hip_graph_capture():
    """The whole cascade (both regulariser mixes) is capturable in a HIP graph: no host synchronisation, no allocation outside the
    caching allocator, every launch on the current stream; a replay reproduces the eager result bit for bit."""
    import bench
    from mvsformerplusplus_amd import synth
    for shipped in (False, True):
        head = bench.build_head(DEV, shipped=shipped)
        feats, projs, dv = synth.make_cascade_inputs(128, 192, 3, seed=3, device=DEV)
        with torch.no_grad():
            eager = head(feats, projs, dv)["refined_depth"].clone()
            graphed = head.capture(feats, projs, dv)                # the product API: CascadeDepthHead.capture -> GraphedCascade
            out = graphed()
            torch.cuda.synchronize()
            assert torch.equal(out["refined_depth"], eager)
            # a new reference view written into the captured input tensors, replayed: equals the eager result on the same data
            f2, p2, d2 = synth.make_cascade_inputs(128, 192, 3, seed=4, device=DEV)
            for k in feats:
                feats[k].copy_(f2[k])
                projs[k].copy_(p2[k])
            out = graphed()
            torch.cuda.synchronize()
            assert torch.equal(out["refined_depth"], head(feats, projs, dv)["refined_depth"])


def test_train_kernels():
    P.case_train_kernels(DEV)


def test_regnet_train_native():
    P.case_regnet_train_native(DEV)


def test_attention_backward():
    P.case_attention_backward(DEV)


def test_transformer_block_backward():
    P.case_transformer_block_backward(DEV)


def test_regnet_train_recompute():
    P.case_regnet_train_recompute(DEV)


def test_train_backward_transformer_golden():
    P.case_train_backward_transformer_golden(DEV)


def test_device_packing():
    P.case_device_packing(DEV)


def test_train_fp32_configured_head():
    P.case_train_fp32_configured_head(DEV)


def test_generic_conv_fuzz():
    P.case_generic_conv_fuzz(DEV, n_cases=60, seed=0)


# ---- the warp / gather kernels on non-DTU camera rigs against the fp64 restatement (tests/warp_ref.py, tests/rig_cases.py) ----
def test_homography_rigs():
    P.case_homography_rigs(DEV)


@pytest.mark.parametrize("name,shape", RC.GATHER_CASES, ids=RC.GATHER_IDS)
def test_warp_rigs(name, shape):
    P.case_warp_rigs(DEV, name, shape)


@pytest.mark.parametrize("name,shape", RC.GATHER_CASES, ids=RC.GATHER_IDS)
def test_gather_rigs(name, shape):
    P.case_gather_rigs(DEV, name, shape)


@pytest.mark.parametrize("name,shape", RC.BACKWARD_CASES, ids=RC.BACKWARD_IDS)
def test_aggregate_backward_rigs(name, shape):
    P.case_aggregate_backward_rigs(DEV, name, shape)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["convergent", "roll90", "zoom"])
def test_cascade_rigs(name, prec):
    P.case_cascade_rigs(DEV, name, prec)
