#!/usr/bin/env python3
"""Measure the native FPN encoder + decoder (mvsformerplusplus_amd.features) per view; needs the MI355X.

    python scripts/bench_fpn.py [--sizes 1152x1536,1088x1920] [--reps 20] [--out profiles/fpn_bench.json]

One process, shapes warmed, legs alternated rep by rep, device events around each leg, median milliseconds per view (N = 1):
  native      FPNEncoder + FPNDecoder (csrc/fpn_kernels.hip)
  torch_fp32  the restatement of tests/fpn_ref.py in fp32 on PyTorch-ROCm (same weights)
  torch_bf16  the same restatement under torch.autocast(bfloat16), as the reference's test.py:250 runs it
  last_fused / last_unfused  the decoder's last level alone: mvs_fpn_merge_conv_fwd vs mvs_fpn_merge_fwd at full resolution + the 3x3
              convolution (so that the fusion is shown to pay)
The byte model (each tensor written once and read once per consumer, fp32, intra3 never formed) gives the
fraction of the 6.3 TB/s achievable HBM rate each native leg reaches.  Reads nothing outside the repository.
Profile the kernels in a separate run: rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_fpn.py --reps 5
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
ENC = (("conv00", 3, 8, 7, 1), ("conv01", 8, 8, 5, 1), ("downsample1", 8, 16, 5, 2), ("conv10", 16, 16, 3, 1), ("conv11", 16, 16, 3, 1),
       ("downsample2", 16, 32, 5, 2), ("conv20", 32, 32, 3, 1), ("conv21", 32, 32, 3, 1), ("downsample3", 32, 64, 3, 2),
       ("conv30", 64, 64, 3, 1), ("conv31", 64, 64, 3, 1))


def byte_model(H, W):
    """-> ({layer: (bytes, MACs)}, encoder total, decoder total) for one view, fp32 tensors, written once and read once per consumer."""
    rows, h, w = {}, H, W
    for name, ci, co, k, s in ENC:
        oh, ow = (h - 1) // s + 1, (w - 1) // s + 1
        rows[name] = (4 * (ci * h * w + co * oh * ow), co * ci * k * k * oh * ow)
        h, w = oh, ow
    lv = [(H // 8, W // 8), (H // 4, W // 4), (H // 2, W // 2), (H, W)]
    rows["out0"] = (4 * (64 + 64) * lv[0][0] * lv[0][1], 64 * 64 * lv[0][0] * lv[0][1])
    for k, (clat, co) in zip((1, 2), ((32, 32), (16, 16))):
        (ph, pw), (fh, fw) = lv[k - 1], lv[k]
        rows["merge%d" % k] = (4 * (64 * ph * pw + clat * fh * fw + 64 * fh * fw), 64 * clat * fh * fw)
        rows["out%d" % k] = (4 * (64 + co) * fh * fw, co * 64 * 9 * fh * fw)
    (ph, pw), (fh, fw) = lv[2], lv[3]
    rows["last_fused"] = (4 * (64 * ph * pw + 8 * fh * fw + 8 * fh * fw), (64 * 8 + 8 * 64 * 9) * fh * fw)
    enc = tuple(sum(rows[n][i] for n, *_ in ENC) for i in (0, 1))
    dec = tuple(sum(rows[n][i] for n in ("out0", "merge1", "out1", "merge2", "out2", "last_fused")) for i in (0, 1))
    return rows, enc, dec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1152x1536,1088x1920")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fpn_ref as R
    from mvsformerplusplus_amd import ops, synth
    from mvsformerplusplus_amd.features import FPNDecoder, FPNEncoder
    dev = torch.device("cuda", 0)
    enc, dec = FPNEncoder([8, 16, 32, 64]), FPNDecoder([8, 16, 32, 64])
    for m, seed in ((enc, 25), (dec, 26)):
        m.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(m.state_dict()), seed), strict=True)
    enc, dec = enc.eval().to(dev), dec.eval().to(dev)
    sde = {k: v.to(dev) for k, v in enc.state_dict().items()}
    sdd = {k: v.to(dev) for k, v in dec.state_dict().items()}
    pd = dec._params(dev)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "hbm_rate_used": HBM, "sizes": {}}

    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
        intra2 = torch.randn(1, 64, H // 2, W // 2, device=dev)
        conv01 = torch.randn(1, 8, H, W, device=dev)

        def native():
            e = enc(x)
            return dec(*e)

        def torch_fp32():
            e = R.encoder(x, sde, dtype=torch.float32)
            return R.decoder(*e, sdd, dtype=torch.float32)

        def torch_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                e = R.encoder(x, sde, dtype=torch.float32)
                return R.decoder(*e, sdd, dtype=torch.float32)

        def last_fused():
            return ops.fpn_merge_conv(intra2, conv01, *pd["inner3"], *pd["out3"], 8, ops.FPN_ACT_SWISH)

        def last_unfused():
            t = ops.fpn_merge(intra2, conv01, *pd["inner3"])
            return ops.fpn_conv(t, *pd["out3"], 8, 3, 1, ops.FPN_ACT_SWISH)

        legs = {"native": native, "torch_fp32": torch_fp32, "torch_bf16": torch_bf16, "last_fused": last_fused, "last_unfused": last_unfused}
        times = {k: [] for k in legs}
        with torch.no_grad():
            for fn in legs.values():                     # warm shapes (MIOpen searches, packed weights, allocator)
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
        rows, eb, db = byte_model(H, W)
        med = {k: statistics.median(v) for k, v in times.items()}
        model_bytes = eb[0] + db[0]
        r = {"ms_per_view": med, "min_ms": {k: min(v) for k, v in times.items()},
             "ms_per_reference_view": {"V5": {k: 5 * med[k] for k in ("native", "torch_fp32", "torch_bf16")},
                                       "V20": {k: 20 * med[k] for k in ("native", "torch_fp32", "torch_bf16")}},
             "model_bytes_per_view": model_bytes, "model_gmac_per_view": {"encoder": eb[1] / 1e9, "decoder": db[1] / 1e9},
             "native_hbm_fraction": model_bytes / (med["native"] * 1e-3) / HBM,
             "last_level_model_bytes": rows["last_fused"][0],
             "last_fused_hbm_fraction": rows["last_fused"][0] / (med["last_fused"] * 1e-3) / HBM,
             "speedup_vs_torch_fp32": med["torch_fp32"] / med["native"], "speedup_vs_torch_bf16": med["torch_bf16"] / med["native"],
             "fusion_speedup": med["last_unfused"] / med["last_fused"],
             "layer_model": {k: {"MB": v[0] / 1e6, "GMAC": v[1] / 1e9} for k, v in rows.items()}}
        result["sizes"][size] = r
        print("%s: native %.3f ms/view (%.0f%% of HBM by the model, %.2f GB), torch fp32 %.3f, torch bf16 %.3f; last level fused %.3f vs "
              "unfused %.3f ms" % (size, med["native"], 100 * r["native_hbm_fraction"], model_bytes / 1e9, med["torch_fp32"], med["torch_bf16"],
                                   med["last_fused"], med["last_unfused"]), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
