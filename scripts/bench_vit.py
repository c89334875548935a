#!/usr/bin/env python3
"""Measure the native DINOv2 ViT-B/14 (mvsformerplusplus_amd.vit) on B = 1, V views; needs the MI355X.

    python scripts/bench_vit.py [--sizes 36x48,34x60] [--views 5] [--reps 20] [--out profiles/vit_bench.json] [--no-count] [--no-error]
    python scripts/bench_vit.py --model-only          # argument parsing + work and byte models, no device

One process, shapes warmed, legs alternated rep by rep, device events around each leg, median milliseconds per forward (sizes are patch
grids h x w: 36 x 48 = 504 x 672 images, 34 x 60 = 476 x 840), random N(0, 1) images and seeded weights:
  native      DinoVisionTransformer.forward_interval_features (csrc/vitdec_kernels.hip, csrc/vit_attention_kernels.hip)
  torch_fp32  the restatement of tests/vit_ref.py in fp32 on PyTorch-ROCm (same weights, F.scaled_dot_product_attention)
  torch_bf16  the same restatement under torch.autocast(bfloat16), as the reference's test.py:250 runs it
Launches per forward: the native C-ABI calls and the profiler's kernel count for the PyTorch legs.  The work model
counts the MACs of the linear layers and of the attention core; the native path issues three bf16 MFMA terms per product, so the
achieved fraction of the 2 500 TF dense bf16 peak is reported per ISSUED term and per PRODUCT.  The byte model counts every tensor read
once per consumer and written once, plus the packed weights once.  The error of each leg against the fp64 restatement (host, first view
only) is recorded as the worst fraction of a level's range.  Reads nothing outside the repository.  Profile the kernels in a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_vit.py --reps 5 --no-count --no-error --no-torch
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

PEAK_BF16 = 2.5e15    # dense bf16 MFMA peak of the MI355X (FLOP/s)
HBM = 6.3e12          # achievable HBM3E rate (float4 copy)
D, HID, DEPTH, HEADS = 768, 3072, 12, 12
KERNELS_PER_CALL = {"mvs_vit_rows_fwd": 1, "mvs_vit_patches_fwd": 1, "mvs_vit_embed_fwd": 2, "mvs_vit_qkv_fwd": 1, "mvs_vit_attention_fwd": 1,
                    "mvs_vitdec_linear_fwd": 1}
CFG = dict(img_size=518, patch_size=14, init_values=1.0, block_chunks=0, ffn_layer="mlp", use_flash2_dino=False, softmax_scale=None,
           train_avg_length=762, cross_interval_layers=3)


def work_model(h, w, V):
    """-> MACs per part for one forward of V views (one MAC = one product of the fp32-equivalent arithmetic); `issued` counts what the
    kernels run: every view padded to npad rows, K = 588 padded to 640, the keys padded to the step of 32."""
    n, T = h * w, h * w + 1
    Tp = (T + 31) // 32 * 32
    per_token = D * 3 * D + D * D + 2 * D * HID
    rows = {"linears": DEPTH * V * T * per_token, "attention": DEPTH * V * HEADS * T * T * 64 * 2, "patch_embed": V * n * 588 * D,
            "issued_linears": DEPTH * V * Tp * per_token, "issued_attention": DEPTH * V * HEADS * Tp * Tp * 64 * 2, "issued_patch_embed": V * n * 640 * D,
            "qkv_n2304": DEPTH * V * Tp * D * 3 * D}
    rows["products"] = rows["linears"] + rows["attention"] + rows["patch_embed"]
    rows["issued_products"] = rows["issued_linears"] + rows["issued_attention"] + rows["issued_patch_embed"]
    return rows


def byte_model(h, w, V):
    """-> bytes per part for one forward: T = npad 768 4 bytes (a token tensor of one view, fp32 or packed-split)."""
    n = h * w
    Tp = (n + 1 + 31) // 32 * 32
    T = Tp * D * 4
    # per block and view: norm1 (r 1 w 1), qkv (r 1 w 3), attention (r 3 w 1), proj (r 2 w 1), norm2 (r 1 w 1), fc1 (r 1 w 4), fc2 (r 5 w 1)
    rows = {"blocks": DEPTH * V * 26 * T, "packed_weights": DEPTH * (4 * D * D + 2 * D * HID) * 4 + 640 * D * 4,
            "embed_and_norm": V * (3 * h * w * 196 * 4 + n * 640 * 4 * 2 + 3 * T)}
    rows["total"] = sum(rows.values())
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="36x48,34x60")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-count", action="store_true", help="skip the launch count (torch's profiler; use under rocprofv3)")
    ap.add_argument("--no-torch", action="store_true", help="native leg only (kernel profiling)")
    ap.add_argument("--no-error", action="store_true", help="skip the fp64 comparison on the host")
    ap.add_argument("--model-only", action="store_true", help="print the work and byte models and exit (no device needed)")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    V = a.views
    if a.model_only:
        print(json.dumps({"%dx%d" % s: {"macs": work_model(s[0], s[1], V), "bytes": byte_model(s[0], s[1], V)} for s in sizes}))
        return
    import vit_ref as R
    from mvsformerplusplus_amd import _lib, synth
    from mvsformerplusplus_amd.vit import vit_base
    dev = torch.device("cuda", 0)
    mod = vit_base(**CFG)
    host_sd = synth.seeded_state_dict(synth.state_dict_manifest(mod.state_dict()), 28)
    g = torch.Generator().manual_seed(2828)
    for key in ("pos_embed", "cls_token"):                       # synth's fan-in rule makes them negligible: N(0, 1) as in fixture F28
        host_sd[key] = torch.randn(host_sd[key].shape, generator=g)
    mod.load_state_dict(host_sd, strict=True)
    mod = mod.eval().to(dev)
    # the PyTorch legs' weights are nn.Parameters, like the reference's: autocast then casts each once per forward (its cast cache)
    sd = {k: torch.nn.Parameter(v.detach().clone().to(dev), requires_grad=False) for k, v in host_sd.items()}
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "views": V, "bf16_peak_used": PEAK_BF16, "hbm_rate_used": HBM, "sizes": {}}

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
                                and not any(t in e.name for t in ("vd_", "va_", "vt_", "Memset")))
        except Exception as exc:                                                  # the count is a report, never a reason to lose the timings
            _lib._LIB = real
            return {"error": repr(exc)}
        native_kernels = sum(KERNELS_PER_CALL[k] * v for k, v in calls.items())
        return {"native_kernels": native_kernels, "torch_kernels": torch_kernels, "total": native_kernels + torch_kernels}

    for h, w in sizes:
        img_host = torch.randn(V, 3, 14 * h, 14 * w, generator=torch.Generator().manual_seed(h + w))
        img = img_host.to(dev)

        def native():
            return mod.forward_interval_features(img)

        def torch_fp32():
            return R.vit(img, sd, dtype=torch.float32)

        def torch_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return R.vit(img, sd, dtype=None)

        legs = {"native": native} if a.no_torch else {"native": native, "torch_fp32": torch_fp32, "torch_bf16": torch_bf16}
        times = {k: [] for k in legs}
        with torch.no_grad():
            for fn in legs.values():                     # warm shapes (library searches, packed weights, allocator)
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
            launches = None if a.no_count else {k: count_launches(fn, k == "native") for k, fn in legs.items()}
            errors = None
            if not a.no_error:
                torch.set_num_threads(16)
                ref = R.vit(img_host[:1], host_sd)
                errors = {k: max(float((o[:1].double().cpu() - r).abs().max() / (r.max() - r.min())) for o, r in zip(fn(), ref)) for k, fn in legs.items()}
        macs, nbytes = work_model(h, w, V), byte_model(h, w, V)
        med = {k: statistics.median(v) for k, v in times.items()}
        sec = med["native"] * 1e-3
        r = {"ms_per_forward": med, "min_ms": {k: min(v) for k, v in times.items()}, "launches_per_forward": launches,
             "worst_level_error_vs_fp64_first_view": errors, "model_macs": macs, "model_bytes": nbytes,
             "native_peak_fraction_per_issued_term": 3 * 2 * macs["issued_products"] / sec / PEAK_BF16,
             "native_peak_fraction_per_product": 2 * macs["products"] / sec / PEAK_BF16,
             "native_hbm_fraction": nbytes["total"] / sec / HBM}
        if not a.no_torch:
            r["speedup_vs_torch_fp32"] = med["torch_fp32"] / med["native"]
            r["speedup_vs_torch_bf16"] = med["torch_bf16"] / med["native"]
        result["sizes"]["%dx%d" % (h, w)] = r
        print("%dx%d patches V=%d: %s ms; %.1f GMAC -> %.1f%% of the bf16 peak per issued term, %.1f%% per product; %.2f GB by the byte model "
              "(%.0f%% of HBM); launches %s; error vs fp64 %s" % (h, w, V, {k: round(v, 3) for k, v in med.items()}, macs["products"] / 1e9,
                                                                 100 * r["native_peak_fraction_per_issued_term"], 100 * r["native_peak_fraction_per_product"],
                                                                 nbytes["total"] / 1e9, 100 * r["native_hbm_fraction"], launches, errors), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
