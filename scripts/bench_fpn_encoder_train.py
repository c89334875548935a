#!/usr/bin/env python3
"""Measure one training step (forward + backward) of the native FPN encoder (training.fpn_encoder_forward_train);
needs the MI355X.

    python scripts/bench_fpn_encoder_train.py [--cases 512x640x4,1024x1280x2] [--views 5] [--reps 10] [--out profiles/fpn_encoder_train_bench.json]
                                              [--no-count] [--native-only]

Cases are HxWxB: by default both ends of the shipped multi-scale training list.  One encoder call on B x V views, forward + backward, all 33
parameter gradients (the image gets none).  One process, shapes warmed, legs alternated rep by rep, device events around each leg, median
milliseconds per step:
  native         TrainableFPNEncoder in train mode
  torch_fp32     PyTorch-ROCm autograd over the restatement tests/fpn_encoder_train_ref.py in fp32 with the same weights - the comparator
Also recorded: launches per step (the native C-ABI calls by their kernel count plus the device kernels torch's profiler sees; the
profiler's kernel count for the PyTorch leg) and each leg's allocator peak over what is allocated before the step.  --native-only runs
the native leg alone, a few steps, for a kernel trace taken in a run of its own.  Reads nothing outside the repository.
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

CHS = (8, 16, 32, 64)
KERNELS_PER_CALL = {"mvs_fpn_conv_fwd": 1, "mvs_fpn_bn_leaky_fwd": 3, "mvs_fpn_bn_leaky_bwd": 3, "mvs_fpn_enc_wgrad": 2, "mvs_fpn_enc_dgrad": 4}
OURS = ("conv2d_split_kernel", "fpn_bn_", "fpn_wgrad_kernel", "fmt_partial_reduce_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="512x640x4,1024x1280x2")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-count", action="store_true", help="skip the launch count (torch's profiler)")
    ap.add_argument("--native-only", action="store_true", help="the native leg alone, three steps per case (for a kernel trace)")
    a = ap.parse_args()
    cases = [tuple(int(v) for v in s.split("x")) for s in a.cases.split(",")]
    V = a.views
    import fpn_encoder_train_ref as R
    from mvsformerplusplus_amd import _lib, synth
    from mvsformerplusplus_amd.features import TrainableFPNEncoder
    dev = torch.device("cuda", 0)
    mod = TrainableFPNEncoder(list(CHS))
    mod.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(mod.state_dict()), 26), strict=True)
    mod = mod.train().to(dev)
    sd = {k: (torch.nn.Parameter(v.detach().clone()) if k in R.PARAMS else v.detach().clone()) for k, v in mod.state_dict().items()}
    sd_params = [sd[k] for k in R.PARAMS]
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
        N = B * V
        g = torch.Generator().manual_seed(H + W)
        x = torch.randn(N, 3, H, W, generator=g).to(dev)
        cots = [torch.randn(N, c, H // s, W // s, generator=g).to(dev) for c, s in zip(CHS, (1, 2, 4, 8))]

        def native():
            torch.autograd.backward(mod(x), cots, inputs=list(mod.parameters()))

        def torch_fp32():
            torch.autograd.backward(R.encoder(x, sd, dtype=torch.float32), cots, inputs=sd_params)

        def clear():
            for t in list(mod.parameters()) + sd_params:
                t.grad = None

        if a.native_only:
            for _ in range(3):
                native(); clear()
            torch.cuda.synchronize()
            continue
        legs = {"native": native, "torch_fp32": torch_fp32}
        times = {k: [] for k in legs}
        for fn in legs.values():                         # warm shapes (library searches, allocator)
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
        peaks = {}
        for k, fn in legs.items():                       # allocator peak of one step over what is allocated before it
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peaks[k] = (torch.cuda.max_memory_allocated() - base) / 1e6
            clear()
        launches = None if a.no_count else {k: count_launches(fn, k == "native") for k, fn in legs.items()}
        clear()
        med = {k: statistics.median(v) for k, v in times.items()}
        r = {"ms_per_step": med, "min_ms": {k: min(v) for k, v in times.items()}, "launches_per_step": launches, "peak_mb_over_start": peaks,
             "speedup_vs_torch_fp32": med["torch_fp32"] / med["native"]}
        result["cases"]["%dx%d B=%d" % (H, W, B)] = r
        print("%dx%d B=%d V=%d: native %.3f ms, torch fp32 autograd %.3f ms per step; peaks (MB) %s; launches %s"
              % (H, W, B, V, med["native"], med["torch_fp32"], {k: round(v) for k, v in peaks.items()}, launches), flush=True)
    if a.native_only:
        return
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
