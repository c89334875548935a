#!/usr/bin/env python3
"""Measure the native CrossVITDecoder (mvsformerplusplus_amd.vit_decoder) per reference view; needs the MI355X.

    python scripts/bench_vit_decoder.py [--sizes 36x48,34x60] [--views 5] [--reps 20] [--out profiles/vit_decoder_bench.json] [--no-count]
    python scripts/bench_vit_decoder.py --model-only          # argument parsing + work and byte models, no device

One process, shapes warmed, legs alternated rep by rep, device events around each leg, median milliseconds per reference view (B = 1, V
views; sizes are token maps h x w: 36 x 48 = 1152 x 1536, 34 x 60 = 1088 x 1920):
  native      CrossVITDecoder (csrc/vitdec_kernels.hip)
  torch_fp32  the restatement of tests/vit_decoder_ref.py in fp32 on PyTorch-ROCm (same weights)
  torch_bf16  the same restatement under torch.autocast(bfloat16), as the reference's test.py:250 runs it
Launches per reference view: the native C-ABI calls (the key/value summary is two kernels) and the profiler's kernel count for the
PyTorch legs.  The work model counts the MACs of the GEMMs and convolutions; the native path issues three bf16
MFMA terms per product, so the achieved fraction of the 2 500 TF dense bf16 peak is reported per ISSUED term and per PRODUCT.  The byte
model counts every tensor read once per consumer and written once, plus the packed weights once.  Reads nothing outside the repository.
Profile the kernels in a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_vit_decoder.py --reps 5 --no-count
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
D, HID = 768, 3072
KERNELS_PER_CALL = {"mvs_vitdec_rows_fwd": 1, "mvs_vitdec_linear_fwd": 1, "mvs_vitdec_kv_fwd": 2, "mvs_vitdec_apply_fwd": 1, "mvs_vitdec_conv_fwd": 1}
ARGS = {"dino_cfg": {"cross_interval_layers": 3,
                     "decoder_cfg": {"attention_type": "Linear", "d_model": 768, "nhead": 12, "ffn_type": "ffn", "init_values": 1.0, "prev_values": 0.5,
                                     "post_norm": False, "pre_norm_query": True, "no_combine_norm": False, "self_cross_types": None,
                                     "softmax_scale": "entropy_invariance", "train_avg_length": 762}},
        "out_ch": 64, "vit_ch": 768}


def work_model(h, w, V):
    """-> MACs per part for one reference view with V views (one MAC = one product of the fp32-equivalent arithmetic)."""
    n = h * w
    block_views = 2 + 3 * (V - 1)
    # q, proj, fc1, fc2 per query token; k, v per key token (a cross block's keys are the reference view's: once per block)
    linears = block_views * n * (2 * D * D + 2 * D * HID) + (2 + (3 if V > 1 else 0)) * n * 2 * D * D
    summary = (2 + (3 if V > 1 else 0)) * n * D * 64
    apply_ = block_views * n * D * 65
    rows = {"linears": linears, "kv_summary_and_apply_fp32": summary + apply_, "proj": V * n * 9 * D * 256, "upsampler0": V * n * 16 * 256 * 128,
            "upsampler1": V * 4 * n * 16 * 128 * 64}
    rows["mfma_bf16_products"] = rows["linears"] + rows["proj"] + rows["upsampler0"] + rows["upsampler1"]
    return rows


def byte_model(h, w, V):
    """-> bytes per part, one reference view with V views: T = n 768 4 bytes (a token tensor of one view, fp32 or packed-split)."""
    n = h * w
    T = n * D * 4
    bv = 2 + 3 * (V - 1)
    # per block-view: rows (read x, write x + xn) 3T, q (r 1 w 1), apply (r 1 w 1), proj (r 2 w 1), norm2 (r 1 w 1), fc1 (r 1 w 4), fc2 (r 5 w 1)
    blocks = bv * 22 * T + (2 + (3 if V > 1 else 0)) * 4 * T
    weights = 5 * (4 * D * D + 2 * D * HID) * 4 + (9 * D * 256 + 16 * 256 * 128 + 16 * 128 * 128) * 4
    head = V * (T + n * 256 * 4 * 2 + 4 * n * 128 * 4 * 2 + 16 * n * 64 * 4)
    rows = {"blocks": blocks, "packed_weights": weights, "head": head}
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
    ap.add_argument("--model-only", action="store_true", help="print the work and byte models and exit (no device needed)")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    V = a.views
    if a.model_only:
        print(json.dumps({"%dx%d" % s: {"macs": work_model(s[0], s[1], V), "bytes": byte_model(s[0], s[1], V)} for s in sizes}))
        return
    import vit_decoder_ref as R
    from mvsformerplusplus_amd import _lib, synth
    from mvsformerplusplus_amd.vit_decoder import CrossVITDecoder
    dev = torch.device("cuda", 0)
    mod = CrossVITDecoder(ARGS)
    mod.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(mod.state_dict()), 27), strict=True)
    mod = mod.eval().to(dev)
    # the PyTorch legs' weights are nn.Parameters, like the reference's: autocast then casts each once per forward (its cast cache)
    sd = {k: (torch.nn.Parameter(v.detach().clone().to(dev)) if v.is_floating_point() else v.to(dev)) for k, v in mod.state_dict().items()}
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
                                and "vd_" not in e.name and "Memset" not in e.name)
        except Exception as exc:                                                  # the count is a report, never a reason to lose the timings
            _lib._LIB = real
            return {"error": repr(exc)}
        native_kernels = sum(KERNELS_PER_CALL[k] * v for k, v in calls.items())
        return {"native_kernels": native_kernels, "torch_kernels": torch_kernels, "total": native_kernels + torch_kernels}

    for h, w in sizes:
        g = torch.Generator().manual_seed(h + w)
        x = [(torch.randn(1, V, h * w, D, generator=g) * s).to(dev) for s in (1.0, 30.0, 30.0)]
        shape = [1, V, h, w, D]

        def native():
            return mod(x, vit_shape=shape)

        def torch_fp32():
            return R.vit_decoder(x, sd, shape, dtype=torch.float32)

        def torch_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return R.vit_decoder(x, sd, shape, dtype=None)

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
        macs, nbytes = work_model(h, w, V), byte_model(h, w, V)
        med = {k: statistics.median(v) for k, v in times.items()}
        sec = med["native"] * 1e-3
        r = {"ms_per_reference_view": med, "min_ms": {k: min(v) for k, v in times.items()}, "launches_per_reference_view": launches,
             "model_macs": macs, "model_bytes": nbytes,
             "native_peak_fraction_per_issued_term": 3 * 2 * macs["mfma_bf16_products"] / sec / PEAK_BF16,
             "native_peak_fraction_per_product": 2 * macs["mfma_bf16_products"] / sec / PEAK_BF16,
             "native_hbm_fraction": nbytes["total"] / sec / HBM}
        if not a.no_torch:
            r["speedup_vs_torch_fp32"] = med["torch_fp32"] / med["native"]
            r["speedup_vs_torch_bf16"] = med["torch_bf16"] / med["native"]
        result["sizes"]["%dx%d" % (h, w)] = r
        print("%dx%d tokens V=%d: %s ms; %.1f GMAC -> %.1f%% of the bf16 peak per issued term, %.1f%% per product; %.2f GB by the byte model "
              "(%.0f%% of HBM); launches %s" % (h, w, V, {k: round(v, 3) for k, v in med.items()}, macs["mfma_bf16_products"] / 1e9,
                                               100 * r["native_peak_fraction_per_issued_term"], 100 * r["native_peak_fraction_per_product"],
                                               nbytes["total"] / 1e9, 100 * r["native_hbm_fraction"], launches), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
