#!/usr/bin/env python3
"""Measure the point-cloud step (mvsformerplusplus_amd/pointcloud.py) on the MI355X; prints one JSON line per measurement and
writes them all to --out.

    python scripts/bench_pointcloud.py --out profiles/pointcloud_bench.json

1. GPU ms per reference view, filter alone and filter + compaction, at the Tanks&Temples shape (1920x1056, 9 sources, dpcd)
   and the cfg2 shape (1152x1536, 10 sources, pcd): CUDA events over --iters back-to-back views after --warmup.
2. A synthetic 40-view scene written to local disk (PFM depth, uint8 .npy confidence, cams, JPEG images), fused by fuse_scene:
   wall time split into decode (worker CPU seconds and the time the main thread waited for them), GPU (events) and PLY write.
3. The same kind of scene through a reference-style loop: the oracle's torch restatement of the filter (oracle/fusion_ref.py),
   numpy masking, the reference's per-point tuple loop and structured-array PLY (test.py:414-442); on a smaller scene
   (--ref-views) because that loop is slow.  The oracle runs on --reference-device: "cpu" by default, because on the MI355X
   stack measured here its broadcast 4x4 matmuls over [1,9,1056,1920] batches stopped with an illegal memory access inside
   torch; the host-side part (masking, tuple loop, PLY) does not depend on where the filter ran.
   --reference-only runs this leg alone (no GPU needed with the CPU oracle); --skip-reference leaves it out.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvsformerplusplus_amd import data_io, pointcloud as PC, synth  # noqa: E402


def per_view_ms(h, w, nsrc, method, warmup, iters):
    dev = torch.device("cuda", 0)
    s = synth.make_fusion_scene(nsrc + 1, h, w, seed=5)
    d, c, cams, rgb = (s[k].to(dev) for k in ("depth", "conf", "cams", "rgb"))
    srcs = list(range(1, nsrc + 1))
    gate = PC.conf_gate(c[0], 0.5, True).float()
    sgate = torch.stack([PC.conf_gate(c[i], 0.5, False) for i in srcs]).float() if method == "pcd" else None
    sd, sc = d[srcs].contiguous(), cams[srcs].contiguous()
    acc = PC.PointCloudAccumulator(dev, capacity=(warmup + iters + 1) * h * w)
    from mvsformerplusplus_amd import ops
    res = {}
    for label, fn in (("filter", lambda: ops.fusion_filter(method == "dpcd", d[0:1], sd[None], cams[0:1], sc[None], ref_conf=gate[None],
                                                           srcs_conf=None if sgate is None else sgate[None], conf_thresh=0.5,
                                                           p0=1.0 if method == "pcd" else 4.0, p1=0.01 if method == "pcd" else 1300.0,
                                                           vthresh=2)),
                      ("filter+compaction", lambda: acc.add_view(d[0], gate, sd, sgate, cams[0], sc, rgb[0], method))):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[label] = a.elapsed_time(b) / iters
    kept = int(acc.finalize()["counts"][0])
    out = {"what": "per_view_gpu_ms", "shape": [h, w], "sources": nsrc, "method": method, "filter_ms": round(res["filter"], 4),
           "filter_compaction_ms": round(res["filter+compaction"], 4), "compaction_ms": round(res["filter+compaction"] - res["filter"], 4),
           "kept_fraction": round(kept / (h * w), 4), "iters": iters}
    # compaction alone: three launches per view
    pts = torch.randn(3, h, w, device=dev)
    acc2 = PC.PointCloudAccumulator(dev, capacity=h * w)
    m = torch.rand(h, w, device=dev) < out["kept_fraction"]
    for _ in range(warmup):
        acc2._counter.zero_()
        ops.pointcloud_append(m, pts, rgb[0], acc2._records, acc2._counter)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        acc2._counter.zero_()
        ops.pointcloud_append(m, pts, rgb[0], acc2._records, acc2._counter)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / iters
    kept = int(m.sum())
    nbytes = 2 * h * w + kept * (12 + 3 + 15)
    out.update(compaction_alone_ms=round(ms, 4), compaction_bytes=nbytes, compaction_GBps=round(nbytes / ms / 1e6, 1))
    return out


def write_scene(root, V, h, w, nsrc, seed=7):
    from PIL import Image
    s = synth.make_fusion_scene(V, h, w, seed=seed)
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for v in range(V):
        data_io.save_pfm(os.path.join(root, "depth_est", "%08d.pfm" % v), s["depth"][v].numpy())
        np.save(os.path.join(root, "confidence", "%08d.npy" % v), s["conf"][v].numpy())
        data_io.write_cam(os.path.join(root, "cams", "%08d_cam.txt" % v), s["cams"][v].numpy())
        Image.fromarray(s["rgb"][v].numpy()).save(os.path.join(root, "images", "%08d.jpg" % v), quality=95)
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write("%d\n" % V)
        for v in range(V):
            srcs = [(v + k) % V for k in range(1, nsrc + 1)]             # local neighbours, wrapping
            f.write("%d\n%d %s\n" % (v, len(srcs), " ".join("%d %.1f" % (x, 100.0 - i) for i, x in enumerate(srcs))))


def scene_fuse(root, method, V):
    st = {}
    t0 = time.perf_counter()
    res = PC.fuse_scene(root, plyfilename=os.path.join(root, "scene.ply"), method=method, convention="dtu", device="cuda:0", stats=st)
    wall = time.perf_counter() - t0
    return {"what": "scene_fuse_scene", "views": V, "method": method, "wall_s": round(wall, 3), "decode_cpu_s": round(st["decode"], 3),
            "decode_wait_s": round(st["decode_wait"], 3), "gpu_s": round(st["gpu"], 4), "write_s": round(st["write"], 3),
            "vertices": st["vertices"], "flushes": st["flushes"]}


def reference_style(root, method, V, nsrc, device="cpu"):
    """The reference's loop shape: per view, read every map again, filter with the torch restatement on the device, copy points
    and mask to the host, boolean-index, then the tuple loop over all vertices and a structured array (plyfile's body)."""
    from oracle import fusion_ref as R
    dev = torch.device(device)
    grids = R.get_pixel_grids
    R.get_pixel_grids = lambda h, w, dtype=torch.float32: grids(h, w, dtype).to(dev)   # the reference builds its pixel grid with .cuda() (fusion.py:8-13)
    t0 = time.perf_counter()
    t_load = t_filter = 0.0
    views = {}
    for ref, srcs in data_io.read_pair_file(os.path.join(root, "pair.txt"), "dtu"):
        srcs = srcs[:10]
        a = time.perf_counter()
        ld = lambda v: (np.ascontiguousarray(data_io.read_pfm(os.path.join(root, "depth_est", "%08d.pfm" % v))[0]),
                        np.load(os.path.join(root, "confidence", "%08d.npy" % v)), PC._cam(os.path.join(root, "cams", "%08d_cam.txt" % v)))
        rd, rc, rcam = ld(ref)
        ss = [ld(s) for s in srcs]
        img = data_io.read_img(os.path.join(root, "images", "%08d.jpg" % ref)).astype(np.float32) / 255.0
        b = time.perf_counter()
        t_load += b - a
        T = lambda x: torch.from_numpy(np.asarray(x)).to(dev)
        sd = T(np.stack([s[0] for s in ss]))[None, :, None]
        scam = T(np.stack([s[2] for s in ss]))[None]
        if method == "pcd":
            o = R.filter_depth(T(rd)[None, None], T(rc / 255)[None], sd, T(np.stack([s[1] for s in ss]))[None], T(rcam)[None], scam,
                               conf_thresh=0.5, thres_disp=1.0, thres_view=2)
        else:
            o = R.dynamic_filter_depth(T(rd)[None, None], T(rc / 255)[None], sd, T(rcam)[None], scam, conf_thresh=0.5)
        points_np = o["points"].cpu().numpy()
        mask_np = o["mask"].cpu().numpy().astype(bool)
        t_filter += time.perf_counter() - b
        p_f = np.stack([points_np[0, k][mask_np[0, 0]] for k in range(3)], -1)
        c_f = np.stack([img.transpose(2, 0, 1)[k][mask_np[0, 0]] for k in range(3)], -1) * 255
        views[str(ref)] = (p_f, c_f.astype(np.uint8))
    a = time.perf_counter()
    p_all, c_all = [np.concatenate([v[k] for v in views.values()], axis=0) for k in range(2)]
    vertexs = np.array([tuple(v) for v in p_all], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    vertex_colors = np.array([tuple(v) for v in c_all], dtype=[("red", "u1"), ("green", "u1"), ("blue", "u1")])
    vertex_all = np.empty(len(vertexs), vertexs.dtype.descr + vertex_colors.dtype.descr)
    for prop in vertexs.dtype.names:
        vertex_all[prop] = vertexs[prop]
    for prop in vertex_colors.dtype.names:
        vertex_all[prop] = vertex_colors[prop]
    data_io.write_ply_records(os.path.join(root, "ref_style.ply"), vertex_all)
    t_ply = time.perf_counter() - a
    return {"what": "scene_reference_style", "views": V, "method": method, "oracle_device": str(dev), "wall_s": round(time.perf_counter() - t0, 3),
            "load_s": round(t_load, 3), "filter_and_copy_s": round(t_filter, 3), "tuple_loop_and_ply_s": round(t_ply, 3),
            "vertices": int(len(vertex_all))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--views", type=int, default=40)
    p.add_argument("--ref-views", type=int, default=3)
    p.add_argument("--h", type=int, default=1056)
    p.add_argument("--w", type=int, default=1920)
    p.add_argument("--tmp", default=None, help="local-disk folder for the synthetic scenes (default: a temporary directory)")
    p.add_argument("--out", default=None)
    p.add_argument("--reference-device", default="cpu")
    p.add_argument("--reference-only", action="store_true")
    p.add_argument("--skip-reference", action="store_true")
    a = p.parse_args()
    results = []
    emit = lambda r: (results.append(r), print(json.dumps(r), flush=True))
    if a.reference_only:
        with tempfile.TemporaryDirectory(dir=a.tmp) as root:
            write_scene(root, a.ref_views, a.h, a.w, 9)
            emit(reference_style(root, "dpcd", a.ref_views, 9, a.reference_device))
        save(a.out, results, "reference-style leg, oracle on %s" % a.reference_device)
        return
    assert torch.cuda.is_available(), "bench_pointcloud needs the MI355X"
    emit(per_view_ms(1056, 1920, 9, "dpcd", a.warmup, a.iters))
    emit(per_view_ms(1152, 1536, 10, "pcd", a.warmup, a.iters))
    with tempfile.TemporaryDirectory(dir=a.tmp) as root:
        t0 = time.perf_counter()
        write_scene(root, a.views, a.h, a.w, 9)
        print("scene of %d views written in %.1f s" % (a.views, time.perf_counter() - t0), flush=True)
        scene_fuse(root, "dpcd", a.views)                                    # warm (allocator, code objects, page cache)
        emit(scene_fuse(root, "dpcd", a.views))
        emit(scene_fuse(root, "pcd", a.views))
    with tempfile.TemporaryDirectory(dir=a.tmp) as root:
        write_scene(root, a.ref_views, a.h, a.w, 9)
        emit(scene_fuse(root, "dpcd", a.ref_views))
        if not a.skip_reference:
            emit(reference_style(root, "dpcd", a.ref_views, 9, a.reference_device))
    save(a.out, results, torch.cuda.get_device_name(0))


def save(path, results, device):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump({"device": device, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
