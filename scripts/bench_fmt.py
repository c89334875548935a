#!/usr/bin/env python3
"""Measure the native FMT_with_pathway (mvsformerplusplus_amd.fmt) per reference view; needs the MI355X.

    python scripts/bench_fmt.py [--sizes 1152x1536,1088x1920] [--views 5] [--reps 20] [--out profiles/fmt_bench.json] [--no-count]
    python scripts/bench_fmt.py --model-only          # argument parsing + byte model, no device

One process, shapes warmed, legs alternated rep by rep, device events around each leg, median milliseconds per reference view (B = 1, V
views):
  native      FMT_with_pathway (csrc/fmt_kernels.hip)
  torch_fp32  the restatement of tests/fmt_ref.py in fp32 on PyTorch-ROCm (same weights)
  torch_bf16  the same restatement under torch.autocast(bfloat16), as the reference's test.py:250 runs it
  level3_fused / level3_unfused  the full-resolution pathway level (16 -> 8) for all views: mvs_fmt_path_fwd vs mvs_fmt_merge_fwd +
              mvs_fmt_smooth_fwd (so that the fusion is shown to pay)
Launches per reference view are counted: the native C-ABI calls (each key/value summary is two kernels) plus the device kernels torch's
profiler sees, and the profiler's kernel count for the PyTorch legs.  The byte model (every tensor read once per
consumer and written once, fp32) gives the fraction of the 6.3 TB/s achievable HBM rate each native leg reaches.  Reads nothing outside
the repository.  Profile the kernels in a separate run: rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_fmt.py --reps 5 --no-count
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

HBM = 6.3e12          # achievable HBM3E rate (float4 copy) on the MI355X
CHS = (64, 32, 16, 8)
NAMES = ("self", "cross", "self", "cross")
KERNELS_PER_CALL = {"mvs_fmt_kv_fwd": 2, "mvs_fmt_block_fwd": 1, "mvs_fmt_path_fwd": 1, "mvs_fmt_merge_fwd": 1, "mvs_fmt_smooth_fwd": 1}


def byte_model(H, W, V, names=NAMES):
    """-> {part: bytes} for one reference view with V views, fp32: a token map of one view is T = 64 n 4 bytes.  A key/value summary
    reads its source once; a block reads and writes its tokens; the position table is read by the two launches of each first layer;
    a pathway level reads the coarse map and the lateral and writes its output; `assembly` = the copies into the [B, V, ...] output."""
    n = (H // 8) * (W // 8)
    T = 64 * n * 4
    n_self, n_cross = names.count("self"), names.count("cross")
    ref = n_self * 3 * T + 2 * T
    src = (V - 1) * (n_self * 3 + n_cross * 2) * T + n_cross * T + 2 * T if V > 1 else 0
    rows = {"reference_view_blocks": ref, "source_view_blocks": src, "assembly": 2 * V * T}
    for k, (c, s) in enumerate(zip(CHS[1:], (4, 2, 1)), 1):
        hw, HW = (H // (2 * s)) * (W // (2 * s)), (H // s) * (W // s)
        rows["level%d" % k] = V * 4 * (2 * c * hw + 2 * c * HW)
    rows["total"] = sum(rows.values())
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1152x1536,1088x1920")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-count", action="store_true", help="skip the launch count (torch's profiler; use under rocprofv3)")
    ap.add_argument("--model-only", action="store_true", help="print the byte model and exit (no device needed)")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    V = a.views
    if a.model_only:
        print(json.dumps({"%dx%d" % s: byte_model(s[0], s[1], V) for s in sizes}))
        return
    import fmt_ref as R
    from mvsformerplusplus_amd import _lib, ops, synth
    from mvsformerplusplus_amd.fmt import FMT_with_pathway
    dev = torch.device("cuda", 0)
    cfg = dict(attention_type="Linear", base_channel=8, d_model=64, nhead=4, init_values=1.0, layer_names=list(NAMES), ffn_type="ffn",
               softmax_scale="entropy_invariance", train_avg_length=12185, self_cross_types=None, post_norm=False, pre_norm_query=False)
    mod = FMT_with_pathway(**cfg)
    mod.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(mod.state_dict()), 26), strict=True)
    mod = mod.eval().to(dev)
    # the PyTorch legs' weights are nn.Parameters, like the reference's: autocast then casts each once per forward (its cast cache)
    sd = {k: torch.nn.Parameter(v.detach().clone().to(dev)) for k, v in mod.state_dict().items()}
    w_red, w_sm = mod._params(dev)["level3"]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "views": V, "hbm_rate_used": HBM, "sizes": {}}

    calls = {}
    real = _lib.lib()

    class Counting:
        def __getattr__(self, name):
            if name in KERNELS_PER_CALL:
                calls[name] = calls.get(name, 0) + 1
            return getattr(real, name)

    def count_launches(fn, native):
        """device kernels of one call: torch's (profiler) + the native C-ABI launches (not all visible to the profiler)"""
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
            ours = ("fmt_block_kernel", "fmt_kv_", "conv2d_split_kernel", "conv2d_source_kernel")
            torch_kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                                and not any(o in e.name for o in ours) and "Memset" not in e.name)
        except Exception as exc:                                                  # the count is a report, never a reason to lose the timings
            _lib._LIB = real
            return {"error": repr(exc)}
        native_kernels = sum(KERNELS_PER_CALL[k] * v for k, v in calls.items())
        return {"native_kernels": native_kernels, "torch_kernels": torch_kernels, "total": native_kernels + torch_kernels}

    for H, W in sizes:
        g = torch.Generator().manual_seed(H + W)
        feats = {"stage%d" % (k + 1): torch.randn(1, V, c, H // s, W // s, generator=g).to(dev) for k, (c, s) in enumerate(zip(CHS, (8, 4, 2, 1)))}
        prev3 = torch.randn(V, 16, H // 2, W // 2, device=dev)
        lat3 = feats["stage4"][0]

        def native():
            return mod(feats)

        def torch_fp32():
            return R.fmt(feats, sd, NAMES, dtype=torch.float32)

        def torch_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return R.fmt(feats, sd, NAMES, dtype=torch.float32)

        def level3_fused():
            return ops.fmt_path(prev3, lat3, w_red, w_sm)

        def level3_unfused():
            return ops.fmt_smooth(ops.fmt_merge(prev3, lat3, w_red), w_sm)

        legs = {"native": native, "torch_fp32": torch_fp32, "torch_bf16": torch_bf16, "level3_fused": level3_fused, "level3_unfused": level3_unfused}
        times = {k: [] for k in legs}
        with torch.no_grad():
            for fn in legs.values():                     # warm shapes (library searches, packed weights, position table, allocator)
                fn(); fn()
            torch.cuda.synchronize()
            for _ in range(a.reps):
                for k, fn in legs.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    e.synchronize()
                    times[k].append(s.elapsed_time(e))
            launches = None if a.no_count else {"native": count_launches(native, True), "torch_fp32": count_launches(torch_fp32, False),
                        "torch_bf16": count_launches(torch_bf16, False)}
        model = byte_model(H, W, V)
        med = {k: statistics.median(v) for k, v in times.items()}
        r = {"ms_per_reference_view": med, "min_ms": {k: min(v) for k, v in times.items()}, "launches_per_reference_view": launches,
             "model_bytes": model, "native_hbm_fraction": model["total"] / (med["native"] * 1e-3) / HBM,
             "level3_fused_hbm_fraction": model["level3"] / (med["level3_fused"] * 1e-3) / HBM,
             "speedup_vs_torch_fp32": med["torch_fp32"] / med["native"], "speedup_vs_torch_bf16": med["torch_bf16"] / med["native"],
             "fusion_speedup": med["level3_unfused"] / med["level3_fused"]}
        result["sizes"]["%dx%d" % (H, W)] = r
        print("%dx%d V=%d: native %.3f ms (%.0f%% of HBM by the model, %.2f GB), torch fp32 %.3f, torch bf16 %.3f; level 3 fused %.3f vs unfused "
              "%.3f ms; launches %s" % (H, W, V, med["native"], 100 * r["native_hbm_fraction"], model["total"] / 1e9, med["torch_fp32"],
                                        med["torch_bf16"], med["level3_fused"], med["level3_unfused"], launches), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
