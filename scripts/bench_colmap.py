#!/usr/bin/env python3
"""Measure colmap2mvsnet (mvsformerplusplus_amd/colmap2mvsnet.py) on synthetic COLMAP models; needs the MI355X.

    python scripts/bench_colmap.py [--models tt,large] [--reps 3] [--out profiles/colmap_bench.json]
    python scripts/bench_colmap.py --reference DIR      # CPU only: the reference's calc_score on a small model, one core

Models (synth.make_colmap_model, ring layout, heavy-tailed tracks up to 60 long): "tt" = 300 images with about 8 k observations
per image (Tanks and Temples-shaped), "large" = 2000 images with about 8 k observations per image.  Per model:
  * end to end: convert() on a written .bin model (reading, device work, cams / pair.txt / image copies), warmed up once, then
    `reps` timed runs;
  * device only: Observations (upload, id lookup), depth_bounds (depth kernel + sorts), score_matrix (CSR build + the five
    launches) and select_views, each timed with device events, `reps` times;
  * the number of co-visible pairs and observations.
Per-kernel times come from a separate run: rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_colmap.py --reps 1
"""
import argparse
import json
import os
import runpy
import shutil
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"tt": dict(n_images=300, n_points=500000, seed=1, tail=1.5, max_track=60),
          "large": dict(n_images=2000, n_points=3300000, seed=2, tail=1.5, max_track=60)}


def write_dense(root, model):
    from mvsformerplusplus_amd import colmap
    colmap.write_model(model, os.path.join(root, "sparse"), ".bin")
    os.makedirs(os.path.join(root, "images_col"), exist_ok=True)
    for name in model.images.names:
        with open(os.path.join(root, "images_col", name), "wb") as f:
            f.write(b"\xff\xd8" + name.encode())


def device_passes(model, reps):
    import torch
    from mvsformerplusplus_amd import colmap, colmap2mvsnet as CM
    E = colmap.extrinsics(model.images)
    out = []
    for _ in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        torch.cuda.synchronize()
        ev[0].record()
        obs = CM.Observations(model, "cuda:0")
        xyz = torch.from_numpy(model.points3D.xyz).cuda()
        ev[1].record()
        CM.depth_bounds(obs, xyz, E)
        ev[2].record()
        S = CM.score_matrix(obs, xyz, E)
        ev[3].record()
        CM.select_views(S)
        ev[4].record()
        torch.cuda.synchronize()
        out.append({k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(("observations_ms", "depths_ms", "scores_ms", "ranking_ms"))})
    pairs = int((S > 0).sum()) // 2
    return out[1:], pairs


def bench(name, reps):
    from mvsformerplusplus_amd import colmap2mvsnet as CM, synth
    t = time.time()
    model = synth.make_colmap_model(**MODELS[name])
    gen_s = time.time() - t
    n, m = len(model.images), len(model.images.point3D_ids)
    root = tempfile.mkdtemp()
    try:
        write_dense(root, model)
        passes, pairs = device_passes(model, reps)
        CM.convert(root, device="cuda:0")
        walls = []
        for _ in range(reps):
            t = time.time()
            CM.convert(root, device="cuda:0")
            walls.append(time.time() - t)
        t = time.time()
        from mvsformerplusplus_amd import colmap
        colmap.read_model(os.path.join(root, "sparse"))
        read_s = time.time() - t
    finally:
        shutil.rmtree(root)
    med = lambda k: float(np.median([p[k] for p in passes]))
    return {"model": name, "images": n, "points": len(model.points3D), "observations": m, "obs_per_image": m / n,
            "max_track": int(np.diff(model.points3D.track_ptr).max()), "covisible_pairs": pairs, "generate_s": gen_s,
            "read_model_s": read_s, "end_to_end_s": walls, "end_to_end_median_s": float(np.median(walls)),
            "device_median_ms": {k: med(k) for k in passes[0]}, "device_runs": passes}


def reference_calc_score(ref_dir, n_images, n_points):
    """The reference's own script on a written model, in this process: np.asscalar and a stub cv2 shimmed, its process pool
    replaced by an in-process map on one core that times calc_score over all pairs."""
    from mvsformerplusplus_amd import synth
    model = synth.make_colmap_model(n_images, n_points, seed=1, tail=1.5, max_track=60)
    root = tempfile.mkdtemp()
    timing = {}

    class OneCorePool:
        def __init__(self, processes=None):
            pass

        def map(self, fn, queue):
            t = time.time()
            r = [fn(q) for q in queue]
            timing["calc_score_s"] = time.time() - t
            timing["pairs"] = len(queue)
            return r

    import multiprocessing as mp
    saved = mp.Pool
    try:
        write_dense(root, model)
        np.asscalar = lambda a: a.item()
        sys.modules["cv2"] = types.ModuleType("cv2")
        mp.Pool = OneCorePool
        argv, sys.argv = sys.argv, ["colmap2mvsnet.py", "--dense_folder", root]
        try:
            runpy.run_path(os.path.join(ref_dir, "colmap2mvsnet.py"), run_name="__main__")
        finally:
            sys.argv = argv
    finally:
        mp.Pool = saved
        del np.asscalar
        sys.modules.pop("cv2", None)
        shutil.rmtree(root)
    m = len(model.images.point3D_ids)
    return dict(timing, images=n_images, observations=m, obs_per_image=m / n_images, seconds_per_pair=timing["calc_score_s"] / timing["pairs"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="tt,large")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None, help="reference source tree: time its calc_score on the CPU instead")
    a = ap.parse_args()
    if a.reference:
        res = {"reference_cpu": [reference_calc_score(a.reference, 24, 8000), reference_calc_score(a.reference, 40, 30000)]}
    else:
        import torch
        res = {"device": torch.cuda.get_device_name(0), "models": [bench(k, a.reps) for k in a.models.split(",")]}
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
