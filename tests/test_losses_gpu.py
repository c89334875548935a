"""GPU (MI355X): the losses and the validation metrics on the device - the checks of tests/test_losses.py (fixture F30 and the fp64
restatement tests/loss_ref.py, the same bars), plus get_multi_stage_losses on the outputs of the native train-mode StageNet (fixture F6's
inputs): the loss equals the restatement on the same outputs and backward() reaches the features and the weights.  Never reads the
reference tree."""
import pytest
import torch

import loss_ref as R
from conftest import load_golden
from parity_cases import dev, make_stage
from test_losses import (assert_loss, check_ce, check_determinism, check_meter, check_metrics, check_metrics_direct, check_multi_stage, check_reg,
                         check_reg_api, check_refusals)
from mvsformerplusplus_amd import losses

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", sorted(R.CE_CASES))
def test_ce_loss_on_device(name):
    check_ce(name, DEV)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", sorted(R.REG_CASES))
def test_reg_loss_on_device(name, clip):
    check_reg(name, clip, DEV)


@pytest.mark.parametrize("name", sorted(R.REG_CASES))
def test_reg_loss_api_on_device(name):
    check_reg_api(name, DEV)


def test_multi_stage_losses_on_device():
    check_multi_stage(DEV)


@pytest.mark.parametrize("blended", [False, True])
@pytest.mark.parametrize("name", sorted(R.METRIC_CASES))
def test_validation_metrics_on_device(name, blended):
    check_metrics(name, blended, DEV)


@pytest.mark.parametrize("name", sorted(R.METRIC_CASES))
def test_metric_functions_on_device(name):
    check_metrics_direct(name, DEV)


def test_validation_meter_on_device():
    check_meter(DEV)


def test_determinism_on_device():
    check_determinism(DEV)


def test_refusals_on_device():
    check_refusals(DEV)


def test_losses_on_the_native_train_mode_stage():
    """F6's inputs through the native StageNet in train mode, then the "ce" loss of its output dictionary against a ground truth planted
    inside the hypotheses: the loss equals the restatement on the same outputs, and backward() leaves finite, non-zero gradients on the
    features and on the weights."""
    fx = load_golden("f6_stage_train_ce.npz")
    net = make_stage(fx, 8, 2, DEV)
    net.training = True                                   # BN layers stay in eval mode, like the fixture
    feats = dev(fx["features"], DEV).clone().requires_grad_(True)
    hyp = dev(fx["hyp"], DEV)
    out = net(feats, dev(fx["proj"], DEV), hyp, 5.0)
    assert out["prob_volume_pre"].requires_grad and out["depth_values"].dim() == 4
    h = out["depth_values"].detach().cpu()
    B, D, H, W = h.shape
    inverse = bool(h[0, 0, 0, 0] > h[0, -1, 0, 0])           # the fixture's hypotheses as they are stored
    gt, mask = R.make_gt_mask(h, inverse, 321)
    got = losses.get_multi_stage_losses({"dlossw": [1.0, 0.75]}, ["ce", "ce"], {"stage1": out, "stage2": out}, {"stage1": gt.to(DEV), "stage2": gt.to(DEV)},
                                        {"stage1": mask.to(DEV), "stage2": mask.to(DEV)}, None, inverse)
    logits = out["prob_volume_pre"].detach().cpu()
    for k, w in (("stage1", 1.0), ("stage2", 0.75)):
        ref, comp = (float(R.ce_value(logits, h, gt, mask, inverse, w, dt)) for dt in (torch.float64, torch.float32))
        assert ref == ref and ref > 0
        assert_loss(got[k].detach(), ref, comp, comp, "native stage " + k)
    (got["stage1"] + got["stage2"]).backward()
    assert bool(torch.isfinite(feats.grad).all()) and float(feats.grad.abs().sum()) > 0
    grads = [(n, p.grad) for n, p in net.named_parameters() if p.requires_grad]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for _, g in grads), [n for n, g in grads if g is None]
    assert any(float(g.abs().sum()) > 0 for _, g in grads)
