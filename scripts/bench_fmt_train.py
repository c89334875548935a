#!/usr/bin/env python3
"""Measure one training step (forward + backward) of the native FMT_with_pathway (training.fmt_forward_train);
needs the MI355X.

    python scripts/bench_fmt_train.py [--cases 512x640x4,1024x1280x2] [--views 5] [--reps 10] [--out profiles/fmt_train_bench.json] [--no-count]

Cases are HxWxB: by default both ends of the shipped multi-scale training list.  One process, shapes warmed, legs alternated rep by rep,
device events around each leg, median milliseconds per step (all B x V views, all 4 input and 66 parameter gradients):
  native         TrainableFMT_with_pathway in train mode: the inference launches forward, hand-written block backward (tensor
                 expressions + rocBLAS GEMMs) and three HIP launches + two ordered reductions per pathway level backward
  torch_fp32     the same arithmetic as PyTorch-ROCm autograd over the restatement of tests/fmt_ref.py in fp32 (same weights)
  native_level3 / torch_level3   the full-resolution pathway level (16 -> 8) alone, forward + backward, for all views
Launches per step are counted: the native C-ABI calls (by their kernel count) plus the device kernels torch's profiler sees, and the
profiler's kernel count for the PyTorch legs.  Reads nothing outside the repository.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHS = (64, 32, 16, 8)
NAMES = ("self", "cross", "self", "cross")
STAGES = ("stage1", "stage2", "stage3", "stage4")
KERNELS_PER_CALL = {"mvs_fmt_kv_fwd": 2, "mvs_fmt_block_fwd": 1, "mvs_fmt_path_fwd": 1, "mvs_fmt_smooth_fwd": 1, "mvs_fmt_path_bwd": 2,
                    "mvs_fmt_smooth_wgrad": 2}
OURS = ("fmt_block_kernel", "fmt_kv_", "conv2d_split_kernel", "fmt_path_bwd_kernel", "fmt_smooth_wgrad_kernel", "fmt_partial_reduce_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="512x640x4,1024x1280x2")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-count", action="store_true", help="skip the launch count (torch's profiler)")
    a = ap.parse_args()
    cases = [tuple(int(v) for v in s.split("x")) for s in a.cases.split(",")]
    V = a.views
    import fmt_ref as R
    from mvsformerplusplus_amd import _lib, synth, training
    from mvsformerplusplus_amd.fmt import TrainableFMT_with_pathway
    dev = torch.device("cuda", 0)
    cfg = dict(attention_type="Linear", base_channel=8, d_model=64, nhead=4, init_values=1.0, layer_names=list(NAMES), ffn_type="ffn",
               softmax_scale="entropy_invariance", train_avg_length=12185, self_cross_types=None, post_norm=False, pre_norm_query=False)
    mod = TrainableFMT_with_pathway(**cfg)
    mod.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(mod.state_dict()), 26), strict=True)
    mod = mod.train().to(dev)
    sd = {k: torch.nn.Parameter(v.detach().clone()) for k, v in mod.state_dict().items()}
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "views": V, "cases": {}}

    calls = {}
    real = _lib.lib()

    class Counting:
        def __getattr__(self, name):
            if name in KERNELS_PER_CALL:
                calls[name] = calls.get(name, 0) + 1
            return getattr(real, name)

    def count_launches(fn, native):
        calls.clear()
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                if native:
                    _lib._LIB = Counting()
                try:
                    fn()
                finally:
                    _lib._LIB = real
                torch.cuda.synchronize()
            torch_kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                                and not any(o in e.name for o in OURS) and "Memset" not in e.name)
        except Exception as exc:                                                  # the count is a report, never a reason to lose the timings
            _lib._LIB = real
            return {"error": repr(exc)}
        native_kernels = sum(KERNELS_PER_CALL[k] * v for k, v in calls.items())
        return {"native_kernels": native_kernels, "torch_kernels": torch_kernels, "total": native_kernels + torch_kernels}

    for H, W, B in cases:
        g = torch.Generator().manual_seed(H + W)
        feats = {"stage%d" % (k + 1): torch.randn(B, V, c, H // s, W // s, generator=g).to(dev).requires_grad_(True)
                 for k, (c, s) in enumerate(zip(CHS, (8, 4, 2, 1)))}
        cot = {s: torch.randn_like(t) for s, t in feats.items()}
        prev3 = torch.randn(B * V, 16, H // 2, W // 2, device=dev, requires_grad=True)
        lat3 = feats["stage4"].detach().reshape(B * V, 8, H, W).requires_grad_(True)
        red3, sm3 = mod.dim_reduction_3.weight, mod.smooth_3.weight

        def step(out, leaves):
            torch.autograd.backward([out[s] for s in STAGES], [cot[s] for s in STAGES], inputs=leaves)

        def native():
            step(mod(feats), list(feats.values()) + list(mod.parameters()))

        def torch_fp32():
            step(R.fmt(feats, sd, NAMES, dtype=torch.float32), list(feats.values()) + list(sd.values()))

        def native_level3():
            training.FmtPathLevelTrain.apply(prev3, lat3, red3, sm3).backward(cot["stage4"].reshape(B * V, 8, H, W), inputs=[prev3, lat3, red3, sm3])

        def torch_level3():
            y, _ = R.level({"dim_reduction_3.weight": sd["dim_reduction_3.weight"], "smooth_3.weight": sd["smooth_3.weight"]}, 3, prev3, lat3)
            y.backward(cot["stage4"].reshape(B * V, 8, H, W), inputs=[prev3, lat3, sd["dim_reduction_3.weight"], sd["smooth_3.weight"]])

        legs = {"native": native, "torch_fp32": torch_fp32, "native_level3": native_level3, "torch_level3": torch_level3}
        times = {k: [] for k in legs}

        def clear():
            for t in list(feats.values()) + list(mod.parameters()) + list(sd.values()) + [prev3, lat3]:
                t.grad = None

        for fn in legs.values():                         # warm shapes (library searches, position table, allocator)
            fn(); clear(); fn(); clear()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                times[k].append(s.elapsed_time(e))
                clear()
        launches = None if a.no_count else {"native": count_launches(native, True), "torch_fp32": count_launches(torch_fp32, False),
                                            "native_level3": count_launches(native_level3, True), "torch_level3": count_launches(torch_level3, False)}
        clear()
        med = {k: statistics.median(v) for k, v in times.items()}
        r = {"ms_per_step": med, "min_ms": {k: min(v) for k, v in times.items()}, "launches_per_step": launches,
             "speedup_vs_torch_fp32": med["torch_fp32"] / med["native"], "level3_speedup_vs_torch": med["torch_level3"] / med["native_level3"]}
        result["cases"]["%dx%d B=%d" % (H, W, B)] = r
        print("%dx%d B=%d V=%d: native %.3f ms, torch fp32 autograd %.3f ms per step; level 3 alone %.3f vs %.3f ms; launches %s"
              % (H, W, B, V, med["native"], med["torch_fp32"], med["native_level3"], med["torch_level3"], launches), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
