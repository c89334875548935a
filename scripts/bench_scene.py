#!/usr/bin/env python3
"""Measure a scene's depth inference end to end (mvsformerplusplus_amd.scene); needs the MI355X.

    python scripts/bench_scene.py [--views 49] [--size 1152x1536] [--num-view 5] [--reps 3] [--out profiles/scene_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/bench_scene.py --trace     # a run of its own
    python scripts/bench_scene.py --parse-trace <dir>                                                   # the ViT's share of a forward

A synthetic scene (seeded 1200 x 1600 JPEGs, a ring of cameras, pair.txt with 10 sources per view) is written to a temporary folder and
run through the same native network (tests/golden/f29_network_args.json, seeded weights) in three modes, alternated rep by rep after one
warm pass each; seconds per scene are wall time from the first decode to the last file written:
  baseline    the reference's loop restated over the native network: per sample, every one of its V images is decoded, resized and
              normalised on the host (PIL's bilinear resize stands in for cv2.resize, torch for torchvision's transforms) by 4 loader
              threads running ahead (the DataLoader's 4 workers), uploaded, the forward is bracketed by two synchronisations, the outputs
              are copied back and written by the same thread (save_pfm, np.save, write_cam, the JPEG from the de-normalised floats)
  driver      scene.infer_scene(vit_cache=False): each image decoded and prepared once, outputs packed on the device, a writer thread
  driver+vit  scene.infer_scene(vit_cache=True): the frozen ViT once per image as well
--trace runs three phases separated by marker launches (depth_outputs_pack_kernel on an 8 x 8 map, which no forward uses): K forwards,
K x vit_levels of the sample's views (the bicubic resize + the ViT), K forwards with the levels handed in; --parse-trace sums the kernel
durations per phase from the kernel trace.  Reads nothing outside the repository."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MARKER = "depth_outputs_pack_kernel"


def write_scene(folder, n_views, src_h=1200, src_w=1600, seed=0):
    from PIL import Image
    from mvsformerplusplus_amd import data_io
    rng = np.random.default_rng(seed)
    for sub in ("images", "cams"):
        os.makedirs(os.path.join(folder, sub), exist_ok=True)
    for v in range(n_views):
        low = Image.fromarray(rng.integers(0, 256, (src_h // 8, src_w // 8, 3), dtype=np.uint8))
        low.resize((src_w, src_h), Image.BICUBIC).save(os.path.join(folder, "images", "%08d.jpg" % v), quality=92)
        ang = 0.01 * (v - n_views / 2)
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0] = np.eye(4)
        cam[0, :3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        cam[0, :3, 3] = [-20.0 * (v - n_views / 2), 0.0, 0.0]
        cam[1, :3, :3] = [[2892.33, 0, 823.2], [0, 2883.18, 619.07], [0, 0, 1]]
        cam[1, 3] = [425.0, 2.5, 192, 905.0]                    # a third token: 192 planes of 2.5
        data_io.write_cam(os.path.join(folder, "cams", "%08d_cam.txt" % v), cam)
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write("%d\n" % n_views)
        for v in range(n_views):
            near = sorted((u for u in range(n_views) if u != v), key=lambda u: (abs(u - v), u))[:10]
            f.write("%d\n%d %s\n" % (v, len(near), " ".join("%d %.2f" % (u, 100.0 - abs(u - v)) for u in near)))


def baseline_loop(net, scan_folder, outdir, num_view, numdepth, interval_scale, H, W, dev):
    """test.py:184-321 over general_eval.MVSDataset, restated: per-sample decode + host preprocessing of all V images, no caches."""
    from PIL import Image
    from mvsformerplusplus_amd import data_io, ops, scene
    samples = scene.scene_samples(scan_folder, num_view, numdepth, interval_scale, H, W, "dtu")
    mean = torch.tensor(ops.IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(ops.IMAGENET_STD).view(3, 1, 1)
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(outdir, sub), exist_ok=True)

    def load(s):
        imgs = []
        for path in s["images"]:
            img = np.array(Image.open(path).convert("RGB"))
            img = np.asarray(Image.fromarray(img).resize((W, H), Image.BILINEAR))
            imgs.append(torch.from_numpy(img).permute(2, 0, 1).contiguous().float().div(255).sub_(mean).div_(std))
        return (torch.stack(imgs)[None], {k: torch.from_numpy(v)[None] for k, v in s["proj_matrices"].items()},
                torch.from_numpy(s["depth_values"])[None])

    with ThreadPoolExecutor(max_workers=4) as pool, torch.no_grad():
        pending = [pool.submit(load, s) for s in samples[:8]]              # 4 workers x prefetch_factor 2
        for i, s in enumerate(samples):
            imgs, projs, dv = pending.pop(0).result()
            if i + 8 < len(samples):
                pending.append(pool.submit(load, samples[i + 8]))
            torch.cuda.synchronize()
            imgs_d = imgs.to(dev)
            out = net(imgs_d, {k: v.to(dev) for k, v in projs.items()}, dv.to(dev))
            torch.cuda.synchronize()
            depth, conf = out["refined_depth"][0].cpu().numpy(), out["photometric_confidence"][0].cpu().numpy()
            name = "%08d" % s["ref"]
            data_io.save_pfm(os.path.join(outdir, "depth_est", name + ".pfm"), depth)
            data_io.save_confidence(os.path.join(outdir, "confidence", name + ".npy"), conf)
            data_io.write_cam(os.path.join(outdir, "cams", name + "_cam.txt"), s["proj_matrices"]["stage4"][0])
            img = (imgs_d[0, 0] * std.to(dev) + mean.to(dev)).permute(1, 2, 0).cpu().numpy()
            Image.fromarray(np.clip(img * 255, 0, 255).astype(np.uint8)).save(os.path.join(outdir, "images", name + ".jpg"), quality=95)
    return len(samples)


def trace(net, dev, H, W, V, reps):
    from mvsformerplusplus_amd import ops, synth
    imgs = torch.rand(1, V, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    projs = {k: v.to(dev) for k, v in synth.stage_proj_matrices(synth.make_cameras(V, H, W, baseline=30.0, rot_deg=1.0, seed=1), 4).items()}
    dv = torch.arange(425.0, 425.0 + 2.65 * 191.5, 2.65)[None].to(dev)
    one = torch.ones(8, 8, device=dev)
    with torch.no_grad():
        levels = [t[None] for t in net.vit_levels(imgs[0])]
        for _ in range(2):                                                  # warm every shape
            net(imgs, projs, dv)
            net(imgs, projs, dv, vit_levels=levels)
        torch.cuda.synchronize()
        for phase in (lambda: net(imgs, projs, dv), lambda: net.vit_levels(imgs[0]), lambda: net(imgs, projs, dv, vit_levels=levels)):
            ops.depth_outputs_pack(one, one)
            for _ in range(reps):
                phase()
            torch.cuda.synchronize()
        ops.depth_outputs_pack(one, one)
        torch.cuda.synchronize()
    print("trace phases done: %d x forward | vit_levels | forward(vit_levels=), separated by %s" % (reps, MARKER))


def parse_trace(folder, reps):
    files = sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s (rocprofv3 --kernel-trace --output-format csv)" % folder)
    rows = []
    for path in files:
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[2]]
    if len(marks) < 4:
        raise SystemExit("expected 4 marker launches (%s) in the trace, found %d" % (MARKER, len(marks)))
    marks = marks[-4:]
    phases = []
    for a, b in zip(marks[:-1], marks[1:]):
        seg = rows[a + 1:b]
        phases.append({"kernel_ms": sum(e - s for s, e, _ in seg) / 1e6 / reps, "launches": len(seg) / reps})
    full, vit, cached = phases
    res = {"forward_kernel_ms": full["kernel_ms"], "vit_levels_kernel_ms": vit["kernel_ms"], "forward_with_levels_kernel_ms": cached["kernel_ms"],
           "launches": [p["launches"] for p in phases], "vit_share_of_forward": vit["kernel_ms"] / full["kernel_ms"],
           "share_by_difference": 1.0 - cached["kernel_ms"] / full["kernel_ms"]}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1152x1536")
    ap.add_argument("--num-view", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parse-trace", metavar="DIR", default=None)
    ap.add_argument("--trace-reps", type=int, default=5)
    a = ap.parse_args()
    if a.parse_trace:
        parse_trace(a.parse_trace, a.trace_reps)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py measures on the MI355X: no ROCm device is visible")
    from bench_network import build_network
    from mvsformerplusplus_amd import scene
    H, W = (int(v) for v in a.size.split("x"))
    dev = torch.device("cuda", 0)
    net = build_network(dev)
    if a.trace:
        trace(net, dev, H, W, a.num_view, a.trace_reps)
        return
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_scene(os.path.join(tmp, "in", "scan"), a.views)
        print("synthetic scene of %d views written in %.1f s" % (a.views, time.perf_counter() - t0), flush=True)
        kw = dict(dataset="dtu", num_view=a.num_view, numdepth=192, interval_scale=1.06, max_h=H, max_w=W, device=dev)
        stats = {}

        def run(mode, tag):
            out = os.path.join(tmp, "out_%s_%s" % (mode, tag))
            torch.cuda.synchronize()
            t = time.perf_counter()
            if mode == "baseline":
                baseline_loop(net, os.path.join(tmp, "in", "scan"), os.path.join(out, "scan"), a.num_view, 192, 1.06, H, W, dev)
            else:
                st = {}
                scene.infer_scene(net, os.path.join(tmp, "in"), ["scan"], out, vit_cache=mode == "driver+vit", stats=st, **kw)
                stats[mode] = st
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            if tag != "0" or mode == "baseline":                           # rep 0 of the two driver modes is compared below
                shutil.rmtree(out, ignore_errors=True)
            return dt

        modes = ("baseline", "driver", "driver+vit")
        for m in modes:
            print("warm %s: %.2f s" % (m, run(m, "warm")), flush=True)
        times = {m: [] for m in modes}
        for rep in range(a.reps):
            for m in modes:
                times[m].append(run(m, str(rep)))
            print("rep %d: %s" % (rep, {m: round(times[m][-1], 3) for m in modes}), flush=True)
        # the files of the two driver modes are byte-identical (the ViT cache changes nothing)
        same = all(open(os.path.join(tmp, "out_driver_0", "scan", sub, n), "rb").read() == open(os.path.join(tmp, "out_driver+vit_0", "scan", sub, n), "rb").read()
                   for sub in ("depth_est", "confidence") for n in sorted(os.listdir(os.path.join(tmp, "out_driver_0", "scan", sub))))
        res = {"device": torch.cuda.get_device_name(0), "views": a.views, "size": a.size, "num_view": a.num_view, "reps": a.reps,
               "seconds_per_scene": {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in times.items()},
               "driver_files_identical_with_and_without_vit_cache": same,
               "driver_stats": {m: {k: v for k, v in st.items() if k != "wall"} for m, st in stats.items()}}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
