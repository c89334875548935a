#!/usr/bin/env python3
"""Measure the Gipuma route (mvsformerplusplus_amd/gipuma.py) on synthetic scenes; needs the MI355X.

    python scripts/bench_gipuma.py [--scenes dtu,tt] [--reps 2] [--out profiles/gipuma_bench.json]

Scenes (tests/gipuma_cases.make_scene geometry): "dtu" = 49 views at 1152x1600, "tt" = 150 views at 1056x1920.  Per scene:
  * end to end: fuse_scene_gipuma on a written scene folder (PFM depths, uint8 confidences, JPEG images), warmed up once, then
    `reps` timed runs: wall, decode, decode_wait, write and GPU seconds (device events around each reference view's launch and
    compaction), vertex count;
  * device only: the views uploaded from host tensors (H2D + prepare kernel, events) and the N fusion launches timed with events
    per reference view (median / max of the per-view milliseconds), `reps` times.
Profile the kernels in a separate run: rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_gipuma.py --scenes dtu --reps 1
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = {"dtu": (49, 1152, 1600), "tt": (150, 1056, 1920)}


def write_folder(root, sc):
    from PIL import Image
    from mvsformerplusplus_amd import data_io
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    g = np.random.default_rng(5)

    def one(v):
        nm = "%08d" % v
        data_io.save_pfm(os.path.join(root, "depth_est", nm + ".pfm"), sc["depth"][v])
        np.save(os.path.join(root, "confidence", nm + ".npy"), np.random.default_rng(v).integers(100, 256, sc["depth"][v].shape).astype(np.uint8))
        data_io.write_cam(os.path.join(root, "cams", nm + "_cam.txt"), sc["cams"][v])
        Image.fromarray(sc["rgb"][v]).save(os.path.join(root, "images", nm + ".jpg"), quality=95)
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(one, range(sc["depth"].shape[0])))
    del g


def bench_scene(name, reps, tmp):
    import torch
    import gipuma_cases as GC
    from mvsformerplusplus_amd import gipuma as G
    V, H, W = SCENES[name]
    t0 = time.perf_counter()
    sc = GC.make_scene(V, H, W, seed=11)
    folder = os.path.join(tmp, name)
    write_folder(folder, sc)
    out = {"views": V, "height": H, "width": W, "setup_s": time.perf_counter() - t0,
           "device_bytes": V * H * W * 9 + 32 * V * (V + 1), "params": dict(GC.PARAMS, prob_threshold=0.5)}
    dev = torch.device("cuda:0")
    G.fuse_scene_gipuma(folder, os.path.join(tmp, name + ".ply"), device=dev)          # warm-up
    runs = []
    for _ in range(reps):
        st = {}
        G.fuse_scene_gipuma(folder, os.path.join(tmp, name + ".ply"), device=dev, stats=st)
        runs.append(st)
    out["end_to_end"] = runs
    # device only: upload + prepare, then the fusion launches
    host = [(torch.from_numpy(sc["depth"][v]).pin_memory(), torch.from_numpy(sc["rgb"][v]).pin_memory()) for v in range(V)]
    dev_runs = []
    for _ in range(reps):
        fz = G.GipumaFuser(sc["cams"], H, W, dev, **GC.fuser_kwargs(GC.PARAMS))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for v, (d, c) in enumerate(host):
            fz.set_view(v, d.to(dev, non_blocking=True), c.to(dev, non_blocking=True))
        e1.record()
        torch.cuda.synchronize()
        up_wall = time.perf_counter() - t0
        events = []
        t0 = time.perf_counter()
        fz.run(events=events)
        torch.cuda.synchronize()
        run_wall = time.perf_counter() - t0
        per_view = np.array([a.elapsed_time(b) for a, b in events])
        n = int(fz.accumulator.finalize()["counts"].sum())
        dev_runs.append({"upload_gpu_ms": e0.elapsed_time(e1), "upload_wall_s": up_wall, "fuse_gpu_ms": float(per_view.sum()),
                         "fuse_wall_s": run_wall, "per_view_ms_median": float(np.median(per_view)), "per_view_ms_min": float(per_view.min()),
                         "per_view_ms_max": float(per_view.max()), "vertices": n})
        del fz
    out["device_only"] = dev_runs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dtu,tt")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gipuma: needs the MI355X (no GPU found)")
    res = {"device": torch.cuda.get_device_name(0), "scenes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            res["scenes"][name] = bench_scene(name, a.reps, tmp)
            r = res["scenes"][name]
            print(name, json.dumps({"end_to_end": r["end_to_end"][-1], "device_only": r["device_only"][-1]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
