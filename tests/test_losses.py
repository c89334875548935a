"""CPU (host-emulated kernels): the multi-stage depth losses and the validation metrics of csrc/loss_kernels.hip behind
mvsformerplusplus_amd.losses / .metrics, against fixture F30 (recorded from the reference, tests/golden/make_golden_losses.py) and the
fp64 restatement tests/loss_ref.py.  The check functions take a device and are run again on the MI355X by tests/test_losses_gpu.py.

Bars: the bin index and the valid mask equal the fixture's bit for bit; a loss sits within four times the fp32
composite's own distance from the fp64 value (floor 2^-22 relative) of the restatement AND of the fixture; a gradient within the larger of
four times the composite's own error and 1e-6 of max |grad|, elementwise, with exact zeros at masked pixels; the metrics within 1e-6
relative of the fixture with the NaN / 0 conventions; two runs are bit-identical."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_ref as R
from conftest import load_golden
from mvsformerplusplus_amd import _lib, losses, metrics, ops


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("f30_losses.npz")


def assert_loss(got, ref, comp, fixed, what):
    """got: our fp32 loss; ref / comp: the fp64 and the fp32 restatement; fixed: the reference's recorded value."""
    got = float(got)
    if math.isnan(ref):
        assert math.isnan(got) and math.isnan(float(fixed)), (what, got, fixed)
        return
    bar = R.loss_bar(ref, comp)
    print("%s: loss %.9g ref %.12g composite off by %.3g, ours by %.3g (fixture by %.3g), bar %.3g"
          % (what, got, ref, abs(comp - ref), abs(got - ref), abs(got - float(fixed)), bar))
    assert abs(got - ref) <= bar, (what, got, ref, bar)
    assert abs(got - float(fixed)) <= bar, (what, got, float(fixed), bar)


def assert_grad(got, ref, bar, valid, what):
    """got within `bar` (elementwise, R.grad_bar of the two restatements) of ref; exact zeros where the pixel is not valid."""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    print("%s: max |grad| %.3g, worst error %.3g, worst error / bar %.3g" % (what, float(ref.abs().max()), float(err.max()),
                                                                               float((err / bar.clamp_min(1e-300)).max())))
    assert bool((err <= bar).all()), (what, float(err.max()))
    off = ~(valid if valid.dim() == got.dim() else valid.unsqueeze(1).expand_as(got))
    assert bool((got[off] == 0).all()), "%s: a masked pixel has a gradient" % what


# ---- cross entropy ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ce_reference(name):
    x = R.ce_inputs(name)
    assert R.checksum(x) == fixture()["in.ce.%s" % name], "the regenerated inputs of %s differ from the ones the fixture was recorded on" % name
    fn = lambda dtype: (lambda l: R.ce_value(l, x["hyp"], x["gt"], x["mask"], x["inverse"], R.CE_WEIGHT, dtype))  # noqa: E731
    return x, R.value_and_grad(fn(torch.float64), x["logits"], torch.float64), R.value_and_grad(fn(torch.float32), x["logits"], torch.float32)


def run_ce(x, dev):
    logits = x["logits"].to(dev).requires_grad_(True)
    stage = {"stage1": {"depth_values": x["hyp"].to(dev), "prob_volume_pre": logits}}
    out = losses.get_multi_stage_losses({"dlossw": [R.CE_WEIGHT]}, ["ce"], stage, {"stage1": x["gt"].to(dev)}, {"stage1": x["mask"].to(dev)},
                                        None, x["inverse"])
    assert list(out) == ["stage1"] and out["stage1"].dim() == 0 and out["stage1"].dtype == torch.float32
    out["stage1"].backward()
    return out["stage1"].detach(), logits.grad


def check_ce(name, dev):
    fx = fixture()
    x, (ref, gref), (comp, gcomp) = ce_reference(name)
    D = x["hyp"].shape[1]
    want_valid = fx["ce.%s.valid" % name]
    want_index = R.stored_index(fx["ce.%s.index" % name].long(), want_valid, D, x["inverse"])
    index, valid = R.ce_decisions(x["hyp"], x["gt"], x["mask"], x["inverse"])
    assert torch.equal(valid, want_valid) and torch.equal(index[valid], fx["ce.%s.index" % name].long()[valid]), "the restatement's decisions"
    loss1, count, got_index, lse = ops.ce_loss_fwd(x["logits"].to(dev), x["hyp"].to(dev), x["gt"].to(dev), x["mask"].to(dev), x["inverse"],
                                                   R.CE_WEIGHT)
    assert torch.equal(got_index.cpu(), want_index), "index differs from the reference's gt_index_volume / final mask"
    assert int(count) == fx["ce.%s.n" % name] == int(want_valid.sum())
    want_lse = torch.logsumexp(x["logits"].double(), 1)
    assert float((lse.cpu().double() - want_lse).abs().max()) <= 2e-6
    loss, grad = run_ce(x, dev)
    assert torch.allclose(loss.reshape(1), loss1, rtol=0, atol=0, equal_nan=True), "the autograd function and the op disagree"
    assert_loss(loss, ref, comp, fx["ce.%s.loss" % name], "ce " + name)
    assert bool(torch.isfinite(grad).all())
    assert_grad(grad, gref, R.grad_bar(gref, gcomp), want_valid, "ce " + name)
    if "ce.%s.grad" % name in fx:                                    # the reference's own backward(), recorded for the small cases
        assert_grad(grad, fx["ce.%s.grad" % name].double(), R.grad_bar(gref, gcomp), want_valid, "ce %s (fixture)" % name)
    if fx["ce.%s.n" % name] == 0:
        assert math.isnan(float(loss)) and bool((grad == 0).all())


# ---- regression -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reg_reference(name, clip):
    x = R.reg_inputs(name)
    assert R.checksum(x) == fixture()["in.reg.%s" % name], "the regenerated inputs of %s differ from the ones the fixture was recorded on" % name
    hyp = x["hyp"] if clip else None
    fn = lambda dtype: (lambda d: R.reg_value(d, x["gt"], x["mask"], x["interval"], hyp, x["inverse"], R.REG_WEIGHT, dtype))  # noqa: E731
    return x, R.value_and_grad(fn(torch.float64), x["depth"], torch.float64), R.value_and_grad(fn(torch.float32), x["depth"], torch.float32)


def run_reg(x, clip, dev):
    depth = x["depth"].to(dev).requires_grad_(True)
    args = {"dlossw": [R.REG_WEIGHT]}
    if clip:
        args["clip_func"] = "dynamic"
    stage = {"stage1": {"depth_values": x["hyp"].to(dev), "depth": depth}}
    out = losses.get_multi_stage_losses(args, ["reg"], stage, {"stage1": x["gt"].to(dev)}, {"stage1": x["mask"].to(dev)},
                                        x["interval"].to(dev), x["inverse"])
    out["stage1"].backward()
    return out["stage1"].detach(), depth.grad


def check_reg(name, clip, dev):
    fx = fixture()
    tag = "reg.%s.%s" % (name, "dynamic" if clip else "plain")
    x, (ref, gref), (comp, gcomp) = reg_reference(name, clip)
    valid = x["mask"] > 0.5
    loss, grad = run_reg(x, clip, dev)
    assert_loss(loss, ref, comp, fx[tag + ".loss"], tag)
    assert bool(torch.isfinite(grad).all())
    assert_grad(grad, gref, R.grad_bar(gref, gcomp), valid, tag)
    if tag + ".grad" in fx:
        assert_grad(grad, fx[tag + ".grad"].double(), R.grad_bar(gref, gcomp), valid, tag + " (fixture)")
    else:
        assert math.isnan(float(loss)) and bool((grad == 0).all())
    if clip:            # the clamp is live on some valid pixels and idle on others
        d = R.ascending(x["hyp"], x["inverse"])
        rng = (d[:, -1] - d[:, 0]) / x["interval"].reshape(-1, 1, 1)
        e = (x["depth"] / x["interval"].reshape(-1, 1, 1) - x["gt"] / x["interval"].reshape(-1, 1, 1)).abs()
        hit = (torch.where(e < 1, 0.5 * e * e, e - 0.5) > rng * 1.001) & valid
        assert name == "rzero" or (bool(hit.any()) and bool((~hit & valid).any()))
        assert bool((grad.cpu()[hit] == 0).all())


def check_reg_api(name, dev):
    """reg_loss (stages 2 and 4 have a ground truth, weights 0.5 and 1.5), simple_loss, get_loss("re") and the log_var refusal."""
    fx = fixture()
    x = R.reg_inputs(name)
    t = {k: v.to(dev) for k, v in x.items() if torch.is_tensor(v)}
    four = {k: {"depth": t["depth"]} for k in losses.STAGE_KEYS}
    gts, masks = {"stage2": t["gt"], "stage4": t["gt"]}, {"stage2": t["mask"], "stage4": t["mask"]}
    got = losses.reg_loss(four, gts, masks, [1.0, 0.5, 2.0, 1.5], t["interval"])
    assert sorted(got) == fx["reg.%s.reg_loss.keys" % name]
    for k, w, fixed in zip(sorted(got), (0.5, 1.5), fx["reg.%s.reg_loss.values" % name].tolist()):
        ref, comp = (float(R.reg_value(x["depth"], x["gt"], x["mask"], x["interval"], None, False, w, dt)) for dt in (torch.float64, torch.float32))
        assert_loss(got[k], ref, comp, fixed, "reg_loss %s %s" % (name, k))
    unit = losses.get_loss({"focal": False, "gamma": 0.0}, "re", four, gts, masks, t["interval"], True)
    assert sorted(unit) == sorted(got)
    ref, comp = (float(R.reg_value(x["depth"], x["gt"], x["mask"], None, None, False, 1.0, dt)) for dt in (torch.float64, torch.float32))
    assert_loss(losses.simple_loss({"depth": t["depth"]}, t["gt"], t["mask"]), ref, comp, fx["reg.%s.simple_loss" % name], "simple_loss " + name)
    with pytest.raises(NotImplementedError, match="log_var"):
        losses.get_multi_stage_losses({"dlossw": [1.0]}, ["reg"], {"stage1": {"depth_values": t["hyp"], "depth": t["depth"], "log_var": t["depth"]}},
                                      {"stage1": t["gt"]}, {"stage1": t["mask"]}, t["interval"], False)


# ---- the four-stage dictionary ----------------------------------------------------------------------------------------------------
def check_multi_stage(dev):
    fx = fixture()
    outputs, gts, masks, interval = R.multi_stage_inputs()
    assert sum(R.checksum(outputs[k]) + R.checksum({"gt": gts[k], "mask": masks[k]}) for k in outputs) == fx["in.ms"]
    to = lambda d: {k: v.to(dev) for k, v in d.items()}  # noqa: E731
    o, g, m = {k: to(v) for k, v in outputs.items()}, to(gts), to(masks)
    got = losses.get_multi_stage_losses(R.MS_ARGS, R.MS_TYPES, o, g, m, interval.to(dev), True)
    assert list(got) == fx["ms.keys"]
    refs = {}
    for i, k in enumerate(got):
        s, w = outputs[k], R.MS_ARGS["dlossw"][i]
        if R.MS_TYPES[i] == "ce":
            refs[k] = [float(R.ce_value(s["prob_volume_pre"], s["depth_values"], gts[k], masks[k], True, w, dt)) for dt in (torch.float64, torch.float32)]
        else:
            refs[k] = [float(R.reg_value(s["depth"], gts[k], masks[k], interval, s["depth_values"], True, w, dt)) for dt in (torch.float64, torch.float32)]
        assert_loss(got[k], refs[k][0], refs[k][1], fx["ms.values"][i], "multi-stage " + k)
    last = losses.get_loss({"focal": True, "gamma": 2.0}, "ce", o, g, m, interval.to(dev), True)      # focal / gamma: accepted and ignored
    assert list(last) == fx["ms.get_loss_ce.keys"] == ["stage4"]
    ref, comp = (float(R.ce_value(outputs["stage4"]["prob_volume_pre"], outputs["stage4"]["depth_values"], gts["stage4"], masks["stage4"], True, 1.0, dt))
                 for dt in (torch.float64, torch.float32))
    assert_loss(last["stage4"], ref, comp, fx["ms.get_loss_ce.values"][0], "get_loss ce")
    two = losses.ce_loss({k: o[k] for k in ("stage1", "stage2")}, g, m, None, inverse_depth=True)
    assert list(two) == fx["ms.ce_loss_two.keys"] == ["stage2"]
    with pytest.raises(AssertionError):
        losses.get_multi_stage_losses(R.MS_ARGS, ["ce", "ce", "reg"], o, g, m, interval.to(dev), True)
    with pytest.raises(AssertionError):
        losses.get_multi_stage_losses(R.MS_ARGS, ["ce", "ce", "l1", "ce"], o, g, m, interval.to(dev), True)
    half = {k: dict(v, prob_volume_pre=v["prob_volume_pre"].to(torch.bfloat16).requires_grad_(True)) for k, v in o.items()}
    low = losses.get_multi_stage_losses(R.MS_ARGS, R.MS_TYPES, half, g, m, interval.to(dev), True)       # 16-bit logits are cast, the
    sum(low.values()).backward()                                                                          # gradient returns in their dtype
    assert half["stage1"]["prob_volume_pre"].grad.dtype == torch.bfloat16 and abs(float(low["stage1"].detach()) - float(got["stage1"])) < 0.05


# ---- metrics ----------------------------------------------------------------------------------------------------------------------
def metric_tensors(name, dev):
    x = R.metric_inputs(name)
    assert R.checksum(x) == fixture()["in.met.%s" % name], "the regenerated inputs of %s differ from the ones the fixture was recorded on" % name
    return {k: v.to(dev) for k, v in x.items()}


def assert_metrics(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, got.tolist(), want.tolist())
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, equal_nan=True, err_msg=what)


def check_metrics(name, blended, dev):
    fx, t = fixture(), metric_tensors(name, dev)
    want = fx["met.%s.%s" % (name, "blended" if blended else "dtu")]
    for mask in (t["mask"], t["mask"] > 0.5):                        # the stage's fp32 mask, or the bool map the reference is handed
        got = metrics.validation_metrics(t["est"], t["gt"], mask, t["interval"], blended=blended)
        assert list(got) == list(metrics.VALIDATION_KEYS) and all(v.dim() == 0 and v.device.type == t["est"].device.type for v in got.values())
        assert_metrics([float(got[k]) for k in metrics.VALIDATION_KEYS], want, "%s blended=%s" % (name, blended))
    if name == "mimage0":                                            # no valid pixel in image 0: NaN ratios poison the batch, an empty band is 0
        assert all(math.isnan(float(got["thres%dmm_error" % k])) for k in R.MM) and all(float(got["abs_depth_thres0-%dmm_error" % k]) > 0 for k in R.MM)
    if name == "mzero":
        assert all(float(got["abs_depth_thres0-%dmm_error" % k]) == 0 for k in R.MM)
    # the counts behind them are integers: exact against a count of the planted and spread errors with the fp32 thresholds
    thr = torch.from_numpy(R.metric_thresholds(t["interval"].cpu(), blended))
    counts, sums, means = ops.depth_metrics(t["est"], t["gt"], t["mask"], [float(k) for k in R.MM], [(0.0, float(k)) for k in R.MM],
                                            interval=t["interval"], divisor=1.0 if blended else 2.65, per_sample=blended)
    err = (t["est"].cpu() - t["gt"].cpu()).abs()
    on = t["mask"].cpu() > 0.5
    for b in range(err.shape[0]):
        want_counts = [int(on[b].sum())] + [int(((err[b] > thr[b, i]) & on[b]).sum()) for i in range(4)] + \
                      [int(((err[b] >= 0) & (err[b] <= thr[b, i]) & on[b]).sum()) for i in range(4)]
        assert counts[b].tolist() == want_counts, (name, blended, b)
        for i in range(4):
            inside = (err[b] <= thr[b, i]) & on[b]
            assert abs(float(sums[b, i]) - float(err[b][inside].double().sum())) <= 1e-12 * max(1.0, float(sums[b, i]))


def check_metrics_direct(name, dev):
    fx, t = fixture(), metric_tensors(name, dev)
    mask = t["mask"] > 0.5
    got = [metrics.Thres_metrics(t["est"], t["gt"], mask, 1.0), metrics.Thres_metrics(t["est"], t["gt"], mask, 3),
           metrics.AbsDepthError_metrics(t["est"], t["gt"], mask), metrics.AbsDepthError_metrics(t["est"], t["gt"], mask, [0.5, 3.0]),
           metrics.AbsDepthError_metrics(t["est"], t["gt"], mask, [1e6, 2e6])]
    assert all(v.dim() == 0 for v in got)
    assert_metrics([float(v) for v in got], fx["met.%s.direct" % name], name + " direct")
    with pytest.raises(AssertionError):
        metrics.Thres_metrics(t["est"], t["gt"], mask, torch.tensor(1.0))


def check_meter(dev):
    t = metric_tensors("m13", dev)
    meter = metrics.ValidationMeter()
    a = metrics.validation_metrics(t["est"], t["gt"], t["mask"], t["interval"])
    b = metrics.validation_metrics(t["est"], t["gt"], t["mask"], t["interval"], blended=True)
    meter.update(a)
    meter.update(b)
    mean = meter.mean()
    assert sorted(mean) == sorted(list(metrics.VALIDATION_KEYS) + ["mean_error"])
    for k in metrics.VALIDATION_KEYS:
        assert abs(mean[k] - (float(a[k]) + float(b[k])) / 2) <= 1e-12
    assert abs(mean["mean_error"] - sum(mean["thres%dmm_error" % k] for k in R.MM) / 4.0) <= 1e-15
    meter.reset()
    assert meter.mean() == {}


# ---- determinism and refusals -----------------------------------------------------------------------------------------------------
def check_determinism(dev):
    x = R.ce_inputs("d5")                                            # several workgroups
    (l1, g1), (l2, g2) = run_ce(x, dev), run_ce(x, dev)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    r = R.reg_inputs("r37")
    (l1, g1), (l2, g2) = run_reg(r, True, dev), run_reg(r, True, dev)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    t = metric_tensors("m37", dev)
    a, b = (metrics.validation_metrics(t["est"], t["gt"], t["mask"], t["interval"]) for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in a)


def check_refusals(dev):
    x = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in R.ce_inputs("d4").items()}
    lo, hy, gt, mk = x["logits"], x["hyp"], x["gt"], x["mask"]
    for bad in ((lo[0], hy, gt, mk), (lo.double(), hy, gt, mk), (lo, hy[:, :3], gt, mk), (lo, hy, gt[:, :5], mk), (lo, hy, gt, mk.bool()),
                (lo[:, :1], hy[:, :1], gt, mk)):                     # rank, dtype, D mismatch, map size, mask dtype, D < 2
        with pytest.raises(ValueError):
            ops.ce_loss_fwd(*bad, False)
    loss, count, index, lse = ops.ce_loss_fwd(lo, hy, gt, mk, False)
    one = torch.ones(1, device=dev)
    for bad in ((lo, index.long(), lse, one, count), (lo, index, lse[0], one, count), (lo, index, lse, one, count.long())):
        with pytest.raises(ValueError):
            ops.ce_loss_bwd(*bad)
    r = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in R.reg_inputs("r13").items()}
    for bad in ((r["depth"][0], r["gt"], r["mask"], r["interval"]), (r["depth"], r["gt"].double(), r["mask"], r["interval"]),
                (r["depth"], r["gt"], r["mask"], r["interval"][:1]), (r["depth"], r["gt"], r["mask"], r["interval"], r["hyp"][:, :1])):
        with pytest.raises(ValueError):
            ops.reg_loss_fwd(*bad)
    t = metric_tensors("m13", dev)
    for bad in ((t["est"][0], t["gt"], t["mask"], [1.0], [None]), (t["est"], t["gt"].double(), t["mask"], [1.0], [None]),
                (t["est"], t["gt"], t["mask"].double(), [1.0], [None]), (t["est"], t["gt"], t["mask"], [1.0] * 9, [None] * 9),
                (t["est"], t["gt"], t["mask"], [1.0], [None, None])):
        with pytest.raises(ValueError):
            ops.depth_metrics(*bad)


# ---- the CPU suite (emulated kernels) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CE_CASES))
def test_ce_loss(emu, name):
    check_ce(name, emu)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", sorted(R.REG_CASES))
def test_reg_loss(emu, name, clip):
    check_reg(name, clip, emu)


@pytest.mark.parametrize("name", sorted(R.REG_CASES))
def test_reg_loss_api(emu, name):
    check_reg_api(name, emu)


def test_multi_stage_losses(emu):
    check_multi_stage(emu)


@pytest.mark.parametrize("blended", [False, True])
@pytest.mark.parametrize("name", sorted(R.METRIC_CASES))
def test_validation_metrics(emu, name, blended):
    check_metrics(name, blended, emu)


@pytest.mark.parametrize("name", sorted(R.METRIC_CASES))
def test_metric_functions(emu, name):
    check_metrics_direct(name, emu)


def test_validation_meter(emu):
    check_meter(emu)


def test_determinism(emu):
    check_determinism(emu)


def test_refusals(emu):
    check_refusals(emu)


def test_host_tensors_are_refused():
    """Without the emulator there is no CPU route: every entry point raises MvsHipError on host tensors."""
    x, r, t = R.ce_inputs("d2"), R.reg_inputs("r13"), R.metric_inputs("m13")
    with pytest.raises(_lib.MvsHipError):
        ops.ce_loss_fwd(x["logits"], x["hyp"], x["gt"], x["mask"], False)
    with pytest.raises(_lib.MvsHipError):
        ops.reg_loss_fwd(r["depth"], r["gt"], r["mask"], r["interval"])
    with pytest.raises(_lib.MvsHipError):
        losses.simple_loss({"depth": r["depth"]}, r["gt"], r["mask"])
    with pytest.raises(_lib.MvsHipError):
        metrics.validation_metrics(t["est"], t["gt"], t["mask"], t["interval"])


def test_public_names():
    import mvsformerplusplus_amd as pkg
    for name in losses.__all__ + [n for n in metrics.__all__ if n != "VALIDATION_KEYS"]:
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(losses if name in losses.__all__ else metrics, name)
