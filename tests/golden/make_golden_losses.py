#!/usr/bin/env python3
"""Generate fixture F30 (tests/golden/f30_losses.npz) by IMPORTING the reference (build container only; not run in the suite).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py

models/losses.py and utils.py are loaded by file path.  utils.py imports ``torchvision`` and ``omegaconf``, which the container does not
have and the recorded functions never touch: both are stubbed.

The inputs come from tests/loss_ref.py (exact integer hashes: every machine regenerates the same bits); the fixture records a checksum of
each case's inputs and what the reference made of them on the CPU:
  ce.<case>.*    loss (fp32), gt_index_volume before the boolean indexing (walk order, uint8), the final mask, N, and for the small cases the
                 gradient of the logits by the reference's own backward()
  reg.<case>.*   the "reg" loss without and with clip_func "dynamic" and the gradients of the depth map; reg_loss() and simple_loss() values
  ms.*           get_multi_stage_losses on the four-stage dictionary, get_loss("ce") (the last stage only) and its keys
  met.<case>.*   the eight validation entries in the DTU and the blended form, and direct calls of the two metric functions
gt_index_volume and the final mask are locals of the reference's function: they are read from its frame with a trace function while it
runs, nothing of it is copied.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MVS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import loss_ref as R  # noqa: E402

GRAD_MAX_ELEMS = 8192         # gradients of larger volumes are left out to keep the file small (the gradient bars use the fp64 restatement)


def load_reference():
    for name in ("torchvision", "torchvision.utils", "omegaconf"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.modules["omegaconf"].OmegaConf = object
    mods = []
    for name, rel in (("ref_losses", os.path.join("models", "losses.py")), ("ref_utils", "utils.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def traced_locals(fn, names, *args, **kwargs):
    """Run fn and return (result, {name: the LAST 3-D tensor the local `name` held in fn's own frame})."""
    seen = {}

    def tracer(frame, event, arg):
        if frame.f_code is not fn.__code__:
            return None

        def local(frame, event, arg):
            for n in names:
                v = frame.f_locals.get(n)
                if torch.is_tensor(v) and v.dim() == 3:
                    seen[n] = v.detach().clone()
            return local
        return local
    sys.settrace(tracer)
    try:
        out = fn(*args, **kwargs)
    finally:
        sys.settrace(None)
    return out, seen


def main():
    L, U = load_reference()
    out = {}

    for name in sorted(R.CE_CASES):
        x = R.ce_inputs(name)
        out["in.ce.%s" % name] = R.checksum(x)
        logits = x["logits"].clone().requires_grad_(True)
        stage = {"stage1": {"depth_values": x["hyp"], "prob_volume_pre": logits}}
        res, seen = traced_locals(L.get_multi_stage_losses, ("gt_index_volume", "final_mask"), {"dlossw": [R.CE_WEIGHT]}, ["ce"], stage,
                                  {"stage1": x["gt"]}, {"stage1": x["mask"]}, None, x["inverse"])
        loss = res["stage1"]
        valid = seen["final_mask"].to(torch.bool)
        out["ce.%s.loss" % name] = loss.detach().numpy()
        out["ce.%s.index" % name] = seen["gt_index_volume"].numpy().astype(np.uint8)
        out["ce.%s.valid" % name] = valid.numpy()
        out["ce.%s.n" % name] = int(valid.sum())
        if logits.numel() <= GRAD_MAX_ELEMS:
            loss.backward()
            out["ce.%s.grad" % name] = logits.grad.numpy()

    for name in sorted(R.REG_CASES):
        x = R.reg_inputs(name)
        out["in.reg.%s" % name] = R.checksum(x)
        for tag, args in (("plain", {"dlossw": [R.REG_WEIGHT]}), ("dynamic", {"dlossw": [R.REG_WEIGHT], "clip_func": "dynamic"})):
            depth = x["depth"].clone().requires_grad_(True)
            stage = {"stage1": {"depth_values": x["hyp"], "depth": depth}}
            loss = _one_reg_stage(L, args, stage, x)
            out["reg.%s.%s.loss" % (name, tag)] = loss.detach().numpy()
            if bool(torch.isfinite(loss)):
                loss.backward()
                out["reg.%s.%s.grad" % (name, tag)] = depth.grad.numpy()
        four = {k: {"depth": x["depth"]} for k in ("stage1", "stage2", "stage3", "stage4")}
        res = L.reg_loss(four, {"stage2": x["gt"], "stage4": x["gt"]}, {"stage2": x["mask"], "stage4": x["mask"]}, [1.0, 0.5, 2.0, 1.5], x["interval"])
        out["reg.%s.reg_loss.keys" % name] = np.asarray(sorted(res))
        out["reg.%s.reg_loss.values" % name] = np.asarray([res[k].item() for k in sorted(res)], dtype=np.float32)
        out["reg.%s.simple_loss" % name] = L.simple_loss({"depth": x["depth"]}, x["gt"], x["mask"]).numpy()

    outputs, gts, masks, interval = R.multi_stage_inputs()
    out["in.ms"] = sum(R.checksum(outputs[k]) + R.checksum({"gt": gts[k], "mask": masks[k]}) for k in outputs)
    res = L.get_multi_stage_losses(R.MS_ARGS, R.MS_TYPES, outputs, gts, masks, interval, True)
    out["ms.keys"] = np.asarray(list(res))
    out["ms.values"] = np.asarray([res[k].item() for k in res], dtype=np.float32)
    res = L.get_loss({"focal": False, "gamma": 0.0}, "ce", outputs, gts, masks, interval, True)
    out["ms.get_loss_ce.keys"] = np.asarray(list(res))
    out["ms.get_loss_ce.values"] = np.asarray([res[k].item() for k in res], dtype=np.float32)
    two = {k: outputs[k] for k in ("stage1", "stage2")}
    out["ms.ce_loss_two.keys"] = np.asarray(list(L.ce_loss(two, gts, masks, None, inverse_depth=True)))

    for name in sorted(R.METRIC_CASES):
        x = R.metric_inputs(name)
        out["in.met.%s" % name] = R.checksum(x)
        est, gt, mask, itv = x["est"], x["gt"], x["mask"] > 0.5, x["interval"]
        di = itv[0].item() / 2.65
        out["met.%s.dtu" % name] = np.asarray([U.AbsDepthError_metrics(est, gt, mask, [0, di * k]).item() for k in R.MM] +
                                              [U.Thres_metrics(est, gt, mask, di * k).item() for k in R.MM], dtype=np.float32)
        rows = []
        for j in range(itv.shape[0]):
            dj = itv[j].item()
            rows.append([U.AbsDepthError_metrics(est[j:j + 1], gt[j:j + 1], mask[j:j + 1], [0, dj * k]).item() for k in R.MM] +
                        [U.Thres_metrics(est[j:j + 1], gt[j:j + 1], mask[j:j + 1], dj * k).item() for k in R.MM])
        out["met.%s.blended" % name] = (np.asarray(rows, dtype=np.float64).sum(0) / itv.shape[0]).astype(np.float32)
        out["met.%s.direct" % name] = np.asarray([U.Thres_metrics(est, gt, mask, 1.0).item(), U.Thres_metrics(est, gt, mask, 3).item(),
                                                 U.AbsDepthError_metrics(est, gt, mask).item(),
                                                 U.AbsDepthError_metrics(est, gt, mask, [0.5, 3.0]).item(),
                                                 U.AbsDepthError_metrics(est, gt, mask, [1e6, 2e6]).item()], dtype=np.float32)

    path = os.path.join(HERE, "f30_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d entries, %d bytes" % (path, len(out), os.path.getsize(path)))


def _one_reg_stage(L, args, stage, x):
    return L.get_multi_stage_losses(args, ["reg"], stage, {"stage1": x["gt"]}, {"stage1": x["mask"]}, x["interval"], x["inverse"])["stage1"]


if __name__ == "__main__":
    main()
