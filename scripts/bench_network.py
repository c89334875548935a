#!/usr/bin/env python3
"""Measure the native DINOv2MVSNet forward (mvsformerplusplus_amd.network) per reference view; needs the MI355X.

    python scripts/bench_network.py [--sizes 1152x1536,1088x1920] [--views 5] [--reps 10] [--out profiles/network_bench.json] [--no-count]
    python scripts/bench_network.py --glue-only [--reps 20]        # the two glue kernels and PyTorch's, for a kernel trace

One process, both legs warmed on every shape, legs alternated rep by rep, device events around each forward, median milliseconds.
Weights are seeded (synth.seeded_state_dict over the network's own manifest, the FMT pathway scaled as in fixture F29); images are U(0, 1),
cameras synth.make_cameras, depth_values the DTU range.  The settings are tests/golden/f29_network_args.json (the shipped arch.args).
  native      DINOv2MVSNet.forward: resize_bicubic, ViT + decoder, the FPN once on all V views, resize_bilinear_add, FMT, the cascade
  comparator  the route the previous release ran under patch_all, restated here (the reference's Python is not on the GPU machine): the
              SAME native modules driven the way DINOv2_mvsformer_model.py:68-179 drives them - F.interpolate bicubic / bilinear, the FPN
              once per view in a Python loop, the PyTorch add, torch.stack, and the reference's stage loop (range functions, 3D positions,
              fusions[i], nearest-resized confidences accumulated by PyTorch)
Launches per forward: every device kernel the profiler sees during one call.  The two legs' refined depths are compared (they differ by
the bicubic coordinate rounding and the cascade's fused prologue only).  The glue kernels are timed in isolation with events (--glue-only
too); for kernel times take a trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bench_network.py --glue-only
and read resize_bicubic_kernel / add_kernel against upsample_bicubic2d_out_frame / the elementwise add in <dir>/*kernel_stats.csv.
Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_network(dev):
    from mvsformerplusplus_amd import DINOv2MVSNet, synth
    args = json.load(open(os.path.join(ROOT, "tests", "golden", "f29_network_args.json")))
    net = DINOv2MVSNet(args)
    sd = synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 29)
    for k in sd:                                  # the linear pathway at unit gain, as in fixture F29 (features stay O(1))
        if k.startswith("FMT_module.dim_reduction_"):
            sd[k] = sd[k] * 0.7071
        elif k.startswith("FMT_module.smooth_"):
            sd[k] = sd[k] * 0.2
    net.load_state_dict(sd, strict=True)
    return net.eval().to(dev)


def comparator(net, imgs, proj_matrices, depth_values, tmp=(5.0, 5.0, 5.0, 1.0)):
    """DINOv2_mvsformer_model.py:68-179 (eval branch) over the native modules: what patch_all(reference model) executes."""
    import mvsformerplusplus_amd as M
    B, V, H, W = imgs.shape[0], imgs.shape[1], imgs.shape[3], imgs.shape[4]
    vit_h, vit_w = net.vit_size(H, W)
    vit_imgs = F.interpolate(imgs.reshape(B * V, 3, H, W), (vit_h, vit_w), mode="bicubic", align_corners=False)
    vit_out = [v.reshape(B, V, -1, 768) for v in net.vit.forward_interval_features(vit_imgs)]
    vit_feat = net.decoder_vit.forward(vit_out, Fmats=None, vit_shape=[B, V, vit_h // 14, vit_w // 14, 768])
    if vit_feat.shape[2] != H // 8 or vit_feat.shape[3] != W // 8:
        vit_feat = F.interpolate(vit_feat, size=(H // 8, W // 8), mode="bilinear", align_corners=False)
    feats = [[], [], [], []]
    for vi in range(V):
        conv01, conv11, conv21, conv31 = net.encoder(imgs[:, vi])
        conv31 = conv31 + vit_feat[vi].unsqueeze(0)
        for k, f in enumerate(net.decoder.forward(conv01, conv11, conv21, conv31)):
            feats[k].append(f)
    features = net.FMT_module.forward({"stage%d" % (k + 1): torch.stack(f, dim=1) for k, f in enumerate(feats)})
    outputs, stage = {}, {}
    rng = [None] * 4
    prob_maps = torch.zeros([B, H, W], dtype=torch.float32, device=imgs.device)
    for s in range(len(net.ndepths)):
        proj = proj_matrices["stage%d" % (s + 1)]
        feat = features["stage%d" % (s + 1)]
        h, w = feat.shape[-2:]
        if s == 0:
            hyp = M.init_inverse_range(depth_values, net.ndepths[s], imgs.device, imgs.dtype, h, w)
        else:
            hyp = M.schedule_inverse_range(stage["depth"].detach(), stage["depth_values"], net.ndepths[s], net.depth_interals_ratio[s], h, w)
        pos = None
        if net.cost_reg_type[s] != "Normal" and net.use_pe3d:
            pos, *rng = M.get_position_3d(B, h, w, proj[:, 0, 1, :3, :3], hyp, depth_min=depth_values.min(), depth_max=depth_values.max(),
                                          height_min=rng[0], height_max=rng[1], width_min=rng[2], width_max=rng[3], normalize=True)
        stage = net.fusions[s].forward(feat, proj, hyp, tmp=tmp[s], position3d=pos)
        outputs["stage%d" % (s + 1)] = stage
        conf = stage["photometric_confidence"]
        if conf.shape[1] != H or conf.shape[2] != W:
            conf = F.interpolate(conf.unsqueeze(1), [H, W], mode="nearest").squeeze(1)
        prob_maps += conf
        outputs.update(stage)
    outputs["refined_depth"] = stage["depth"]
    outputs["photometric_confidence"] = prob_maps / len(net.ndepths)
    return outputs


def timed(legs, reps):
    times = {k: [] for k in legs}
    for fn in legs.values():                     # warm shapes: code objects, packed weights, position tables, allocator pools
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
    return times


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memset" not in e.name and "Memcpy" not in e.name)
    except Exception as exc:                     # the count is a report, never a reason to lose the timings
        return repr(exc)


def glue(dev, H, W, V, reps, net):
    """The glue alone at the product's shapes: milliseconds per call, native against PyTorch, by device events."""
    from mvsformerplusplus_amd import ops
    imgs = torch.rand(V, 3, H, W, device=dev)
    vit_h, vit_w = net.vit_size(H, W)
    base, x = torch.randn(V, 64, H // 8, W // 8, device=dev), torch.randn(V, 64, H // 8, W // 8, device=dev)
    xs = torch.randn(V, 64, H // 16, W // 16, device=dev)
    legs = {"resize_bicubic": lambda: ops.resize_bicubic(imgs, vit_h, vit_w),
            "torch_bicubic": lambda: F.interpolate(imgs, (vit_h, vit_w), mode="bicubic", align_corners=False),
            "resize_bilinear_add_same_size": lambda: ops.resize_bilinear_add(base, x),
            "torch_add": lambda: base + x,
            "resize_bilinear_add_x2": lambda: ops.resize_bilinear_add(base, xs),
            "torch_bilinear_x2_add": lambda: base + F.interpolate(xs, base.shape[-2:], mode="bilinear", align_corners=False)}
    t = timed(legs, reps)
    out_bytes = V * 3 * vit_h * vit_w * 4
    return {"ms": {k: statistics.median(v) for k, v in t.items()}, "bicubic_bytes_written": out_bytes, "bicubic_bytes_source": V * 3 * H * W * 4,
            "add_bytes": 3 * base.numel() * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1152x1536,1088x1920")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-count", action="store_true", help="skip the launch count (torch's profiler; use under rocprofv3)")
    ap.add_argument("--glue-only", action="store_true", help="run only the glue kernels and PyTorch's counterparts (kernel trace)")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    V = a.views
    if not torch.cuda.is_available():
        raise SystemExit("bench_network.py measures on the MI355X: no ROCm device is visible")
    from mvsformerplusplus_amd import synth
    dev = torch.device("cuda", 0)
    net = build_network(dev)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "views": V, "sizes": {}}
    with torch.no_grad():
        for H, W in sizes:
            r = {"glue": glue(dev, H, W, V, max(a.reps, 20), net)}
            if not a.glue_only:
                imgs = torch.rand(1, V, 3, H, W, generator=torch.Generator().manual_seed(H + W)).to(dev)
                projs = {k: v.to(dev) for k, v in synth.stage_proj_matrices(synth.make_cameras(V, H, W, baseline=30.0, rot_deg=1.0, seed=1), 4).items()}
                dv = torch.arange(425.0, 425.0 + 2.65 * 191.5, 2.65)[None].to(dev)
                legs = {"native": lambda: net(imgs, projs, dv), "comparator": lambda: comparator(net, imgs, projs, dv)}
                t = timed(legs, a.reps)
                med = {k: statistics.median(v) for k, v in t.items()}
                da, db = legs["native"]()["refined_depth"], legs["comparator"]()["refined_depth"]
                r.update({"ms_per_reference_view": med, "min_ms": {k: min(v) for k, v in t.items()},
                          "speedup_vs_comparator": med["comparator"] / med["native"],
                          "launches_per_forward": None if a.no_count else {k: count_kernels(fn) for k, fn in legs.items()},
                          "refined_depth_relative_l1_between_legs": float(((da - db).abs() / db.abs()).mean())})
            result["sizes"]["%dx%d" % (H, W)] = r
            print("%dx%d V=%d: %s" % (H, W, V, json.dumps(r)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
