#!/usr/bin/env python3
"""Measure the native depth losses and validation metrics (mvsformerplusplus_amd.losses / .metrics); needs the MI355X.

    python scripts/bench_losses.py [--reps 30] [--out profiles/losses_bench.json]

One process, shapes warmed, legs alternated rep by rep, device events around each leg, median milliseconds:
  loss       the "ce" stage loss forward + backward (get_multi_stage_losses on one stage, then backward()) at the training sizes of
             DESIGN.md section 8, B = 2 and (D, H x W) = (32, 64 x 80), (16, 128 x 160), (8, 256 x 320), (4, 512 x 640); the comparator is the
             same arithmetic in PyTorch-ROCm ops (the fp32 restatement of tests/loss_ref.py: flip, intervals, comparisons, boolean-mask
             gather, F.cross_entropy) with its autograd backward
  metrics    validation_metrics (one metrics launch + its finalize, no synchronisation) against the composite metric functions as a
             validation loop calls them (per image boolean indexing, one .item() per entry), at 512 x 640 and 1152 x 1536, B = 1
For each: the time, the launches (native: counted by construction; composite: the non-view ATen ops its FORWARD dispatches, each at
least one launch - the autograd backward adds about as many again) and the bytes the native kernels have to move (every input read
once, every output written once) as a fraction of the 8 TB/s HBM rate.  Reads nothing outside the repository.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 8.0e12
LOSS_SIZES = ((32, 64, 80), (16, 128, 160), (8, 256, 320), (4, 512, 640))
METRIC_SIZES = ((512, 640), (1152, 1536))
VIEWS = ("view", "_unsafe_view", "reshape", "expand", "permute", "unsqueeze", "squeeze", "slice", "select", "transpose", "t", "detach", "alias",
         "as_strided", "_reshape_alias", "lift_fresh")


class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.overloadpacket.__name__ not in VIEWS:
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_ops(fn):
    with OpCounter() as c:
        fn()
    return c.n


def composite_metrics(est, gt, mask, interval):
    """The DTU branch as a validation loop runs it: eight metric calls, each per image with boolean indexing, and a host read per entry."""
    di = interval[0].item() / 2.65
    on = mask > 0.5
    out = []
    for k in (2, 4, 8, 14):
        per = []
        for b in range(est.shape[0]):
            err = (est[b][on[b]] - gt[b][on[b]]).abs()
            err = err[(err >= 0.0) & (err <= di * k)]
            per.append(err.mean() if err.shape[0] else torch.zeros((), device=est.device))
        out.append(torch.stack(per).mean().item())
    for k in (2, 4, 8, 14):
        per = [((est[b][on[b]] - gt[b][on[b]]).abs() > di * k).float().mean() for b in range(est.shape[0])]
        out.append(torch.stack(per).mean().item())
    return out


def timed(legs, reps):
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e))
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import loss_ref as R
    from mvsformerplusplus_amd import losses, metrics
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "hbm_rate_used": HBM, "loss": {}, "metrics": {}}

    for D, H, W in LOSS_SIZES:
        B = 2
        hyp = R.make_hyp(B, D, H, W, True, 11)
        gt, mask = R.make_gt_mask(hyp, True, 11)
        logits = (R.uniform((B, D, H, W), 19) * 8.0 - 4.0).float().to(dev).requires_grad_(True)
        hyp, gt, mask = hyp.to(dev), gt.to(dev), mask.to(dev)
        stage = {"stage1": {"depth_values": hyp, "prob_volume_pre": logits}}

        def native():
            logits.grad = None
            losses.get_multi_stage_losses({"dlossw": [1.0]}, ["ce"], stage, {"stage1": gt}, {"stage1": mask}, None, True)["stage1"].backward()

        def composite():
            logits.grad = None
            R.ce_value(logits, hyp, gt, mask, True, 1.0, torch.float32).backward()

        def composite_forward():
            return R.ce_value(logits, hyp, gt, mask, True, 1.0, torch.float32)

        med, best = timed({"native": native, "composite": composite}, a.reps)
        V, P = B * D * H * W, B * H * W
        nbytes = 16 * V + 24 * P            # forward: logits, hyp, gt, mask in, index, lse out; backward: logits, index, lse in, the gradient out
        r = {"ms": med, "min_ms": best, "native_launches": 3, "composite_ops": count_ops(composite_forward), "native_bytes": nbytes,
             "native_hbm_fraction": nbytes / (med["native"] * 1e-3) / HBM, "speedup": med["composite"] / med["native"]}
        result["loss"]["%dx%dx%d" % (D, H, W)] = r
        print("ce loss D=%d %dx%d: native %.3f ms (3 launches, %.1f MB, %.1f%% of HBM), composite %.3f ms (%d forward ops): %.1fx"
              % (D, H, W, med["native"], nbytes / 1e6, 100 * r["native_hbm_fraction"], med["composite"], r["composite_ops"], r["speedup"]), flush=True)

    for H, W in METRIC_SIZES:
        gt = (425.0 + 500.0 * R.uniform((1, H, W), 5)).float().to(dev)
        est = (gt.double() + (R.uniform((1, H, W), 6).to(dev) - 0.5) * 80.0).float()
        mask = (R.hash24(H * W, 7) % 4 > 0).float().reshape(1, H, W).to(dev)
        interval = torch.tensor([2.5], device=dev)

        def native():
            return metrics.validation_metrics(est, gt, mask, interval)

        def composite():
            return composite_metrics(est, gt, mask, interval)

        med, best = timed({"native": native, "composite": composite}, a.reps)
        nbytes = 12 * H * W
        r = {"ms": med, "min_ms": best, "native_launches": 2, "composite_ops": count_ops(composite), "composite_host_syncs": 9,
             "native_bytes": nbytes, "native_hbm_fraction": nbytes / (med["native"] * 1e-3) / HBM, "speedup": med["composite"] / med["native"]}
        result["metrics"]["%dx%d" % (H, W)] = r
        print("metrics %dx%d: native %.3f ms (2 launches, %.1f MB, %.1f%% of HBM), composite %.3f ms (%d ops, 9 host reads): %.1fx"
              % (H, W, med["native"], nbytes / 1e6, 100 * r["native_hbm_fraction"], med["composite"], r["composite_ops"], r["speedup"]), flush=True)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
