"""A scene's depth maps as ONE coloured point cloud by cross-view consistency: the reference's default route,
``--filter_method gipuma`` of test.py / test_tt.py, which runs misc/gipuma.py's probability filter and conversion and then the
external CUDA program fusibile.  Here the whole route runs on the device (csrc/gipuma_kernels.hip); the contract the kernels
implement is DESIGN.md section 4.8.

Every view of the scene takes part (the images in images/, sorted by file name), not the pair file's sources.  All views'
filtered depths and packed colours stay on the device with one `used` map per view; the reference views are fused one launch
each, in order, on one stream: the pixels an emitted vertex used are marked, and later reference views skip marked pixels.
Each launch writes its view's mask / points / colours, and the point-cloud compaction (csrc/pointcloud_kernels.hip, through
pointcloud.PointCloudAccumulator) appends them as PLY records.

    fuser = GipumaFuser(cams, h, w, device)
    for v in range(N): fuser.set_view(v, depth, rgb, keep)      # device tensors; keep = probability gate
    fuser.run()
    fuser.accumulator.write_ply("scan1.ply")

The PLY is the binary xyz + rgb file data_io.write_ply writes.  fusibile also writes normals, but the reference hands it fake
constant normals ((1, 1, 1) / sqrt(3) wherever the depth is positive), so they carry nothing and are left out; no normal test is
made (the reference's normal_thresh = 360 passes every normal).

``fuse_scene_gipuma`` is the scene driver and ``python -m mvsformerplusplus_amd.gipuma`` its command line.
"""
from __future__ import annotations

import argparse
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import data_io, ops
from .pointcloud import PointCloudAccumulator, conf_gate, _cam

def check_normal_thresh(normal_thresh: float) -> None:
    """No normal test is implemented (the reference's normals are fake): only thresholds every normal passes are accepted."""
    if not float(normal_thresh) >= 180.0:
        raise ValueError("normal_thresh = %r: the Gipuma route implements no normal test (the reference writes fake normals and "
                         "passes normal_thresh = 360); values below 180 would need one" % (normal_thresh,))


class GipumaFuser:
    """Device-resident state of one scene's Gipuma fusion: N views of h x w, cameras cams [N,2,4,4] (0 = extrinsic, 1 = intrinsic,
    as everywhere).  set_view() fills a view's slot; fuse_view() / run() enqueue the fusion launches and append each reference
    view's vertices to `accumulator` (a PointCloudAccumulator; no host synchronisation).

    Device bytes: 9 per pixel and view (fp32 depth, packed colour, used mark) + 32 * N * (N + 1) of camera constants, + one
    [h,w] byte per pixel and view more with return_skipped (the used[r] each launch read, a diagnostic)."""

    def __init__(self, cams, h: int, w: int, device, *, disp_threshold: float = 0.2, num_consistent: float = 3.0,
                 depth_min: float = 0.001, depth_max: float = 100000.0, normal_thresh: float = 360.0, capacity: int = 1 << 24,
                 return_skipped: bool = False, accumulator: Optional[PointCloudAccumulator] = None):
        check_normal_thresh(normal_thresh)
        self.device = torch.device(device)
        views, pairs = ops.gipuma_prepare_cams(cams)
        self.n, self.h, self.w = views.shape[0], int(h), int(w)
        n, h, w = self.n, self.h, self.w
        self.view_consts, self.pair_consts = views.to(self.device), pairs.to(self.device)
        self.params = dict(depth_min=float(depth_min), depth_max=float(depth_max), disp_thresh=float(disp_threshold),
                           num_consistent=float(num_consistent))
        self.depths = torch.zeros(n, h, w, dtype=torch.float32, device=self.device)
        self.colors = torch.zeros(n, h, w, dtype=torch.int32, device=self.device)
        self.used = torch.zeros(n, h, w, dtype=torch.uint8, device=self.device)
        self.skipped = torch.zeros(n, h, w, dtype=torch.uint8, device=self.device) if return_skipped else None
        self._mask = torch.empty(h, w, dtype=torch.uint8, device=self.device)
        self._points = torch.empty(3, h, w, dtype=torch.float32, device=self.device)
        self._rgb = torch.empty(h, w, 3, dtype=torch.uint8, device=self.device)
        self.accumulator = accumulator if accumulator is not None else PointCloudAccumulator(self.device, capacity)

    def set_view(self, v: int, depth: torch.Tensor, rgb: torch.Tensor, keep: Optional[torch.Tensor] = None) -> None:
        """View v's slot: depth [h,w] (fp32), rgb [h,w,3] uint8, keep [h,w] bool (the probability gate; None = keep all), all on
        the fuser's device.  Depths where keep is false become 0 (misc/gipuma.py:177-179)."""
        if tuple(depth.shape[-2:]) != (self.h, self.w) or tuple(rgb.shape) != (self.h, self.w, 3):
            raise ValueError("GipumaFuser.set_view: view %d is %s / %s, the scene is %dx%d" % (v, tuple(depth.shape), tuple(rgb.shape), self.h, self.w))
        ops.gipuma_prepare_view(depth, keep, rgb, self.depths[v], self.colors[v])

    def fuse_view(self, r: int) -> Dict[str, torch.Tensor]:
        """Enqueue reference view r's launch and its compaction.  -> the view's mask / points / rgb buffers (overwritten by the
        next call: read them before, e.g. with .cpu())."""
        ops.gipuma_fuse_view(self.depths, self.colors, self.used, self.view_consts, self.pair_consts, r, mask=self._mask,
                             points=self._points, rgb=self._rgb, skipped=None if self.skipped is None else self.skipped[r], **self.params)
        self.accumulator.append(self._mask, self._points, self._rgb)
        return {"mask": self._mask, "points": self._points, "rgb": self._rgb}

    def run(self, on_view: Optional[Callable[[int, Dict[str, torch.Tensor]], None]] = None, events: Optional[list] = None) -> None:
        """Every view as reference view, in slot order.  events (list, optional): a (start, end) CUDA event pair per view is appended."""
        for r in range(self.n):
            if events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            out = self.fuse_view(r)
            if events is not None:
                ev[1].record()
                events.append(ev)
            if on_view is not None:
                on_view(r, out)


def _decode(scan_folder: str, name: str, pin: bool):
    """Worker thread: one view's depth, confidence and image -> host tensors (pinned for a device upload)."""
    t0 = time.perf_counter()
    prefix = os.path.splitext(name)[0]
    dpath = os.path.join(scan_folder, "depth_est", prefix + ".pfm")
    depth = np.ascontiguousarray(data_io.read_pfm(dpath)[0], dtype=np.float32)
    cpath = os.path.join(scan_folder, "confidence", prefix + ".npy")
    conf = np.load(cpath)
    if conf.shape != depth.shape:
        raise ValueError("%s: confidence map %s does not match the depth map %s" % (cpath, conf.shape, depth.shape))
    ipath = os.path.join(scan_folder, "images", name)
    img = data_io.read_img(ipath)
    if img.shape[:2] != depth.shape:
        raise ValueError("%s: image size %dx%d differs from the depth map's %dx%d" % (ipath, img.shape[1], img.shape[0], depth.shape[1], depth.shape[0]))
    out = {"depth": torch.from_numpy(depth), "conf": torch.from_numpy(np.ascontiguousarray(conf)), "rgb": torch.from_numpy(img)}
    if pin:
        out = {k: t.pin_memory() for k, t in out.items()}
    return out, time.perf_counter() - t0


def scene_view_names(scan_folder: str) -> List[str]:
    """The view set: every image in images/ (hidden files skipped), sorted by file name.  The reference takes os.listdir order and
    leaves the order to fusibile; sorting is this project's choice, so that the output does not depend on the file system.  A
    depth map in depth_est/ without an image is an error (the reference would silently drop the view)."""
    names = data_io.gipuma_view_names(scan_folder)
    if not names:
        raise ValueError("%s: images/ holds no view" % scan_folder)
    prefixes = {os.path.splitext(n)[0] for n in names}
    dfolder = os.path.join(scan_folder, "depth_est")
    if os.path.isdir(dfolder):
        for f in sorted(os.listdir(dfolder)):
            stem, ext = os.path.splitext(f)
            if ext == ".pfm" and not stem.endswith("_prob_filtered") and stem not in prefixes:
                raise ValueError("%s: depth map %s has no image in images/" % (scan_folder, f))
    return names


def fuse_scene_gipuma(scan_folder: str, plyfilename: Optional[str] = None, *, prob_threshold: float = 0.5, disp_threshold: float = 0.2,
                      num_consistent: float = 3.0, depth_min: float = 0.001, depth_max: float = 100000.0, normal_thresh: float = 360.0,
                      device=None, workers: int = 4, stats: Optional[dict] = None, return_skipped: bool = False,
                      capacity: int = 1 << 24, on_view=None) -> Dict[str, np.ndarray]:
    """gipuma_filter of misc/gipuma.py:208-229 for one scene (probability filter, conversion, fusibile), on the device.

    Each view's depth, confidence, camera and image is decoded once on `workers` (<= 4) threads and uploaded as it arrives; the
    probability gate is pointcloud.conf_gate(conf, prob_threshold, divide_uint8=True) (uint8 / 255 in float64, other maps in their
    own dtype, strict >).  Then every view is fused as reference view in sorted-name order.
    -> {"xyz" [N,3] float32, "rgb" [N,3] uint8, "counts" (vertices per reference view), "views" (ids, int64, when every name is
    numeric; else the names)}, plus "skipped" [V,H,W] uint8 (the used map each launch read) with return_skipped.
    stats (optional dict) receives wall / decode / decode_wait / gpu / write seconds, views, vertices, flushes (as fuse_scene).
    on_view (optional) is called as on_view(view index, {"mask", "points", "rgb"}) after each launch is enqueued."""
    check_normal_thresh(normal_thresh)
    device = torch.device(device if device is not None else "cuda")
    on_gpu = device.type == "cuda"
    t_wall = time.perf_counter()
    names = scene_view_names(scan_folder)
    # cameras first (small text files): the fuser's constants need every view's
    cams = np.stack([_cam(os.path.join(scan_folder, "cams", os.path.splitext(n)[0] + "_cam.txt")) for n in names])
    fuser, shape, t_decode, t_wait = None, None, 0.0, 0.0
    with ThreadPoolExecutor(max_workers=max(1, min(4, int(workers)))) as pool:
        futures = [pool.submit(_decode, scan_folder, n, on_gpu) for n in names]
        for v, fut in enumerate(futures):                  # upload each view as it arrives, in order
            t0 = time.perf_counter()
            host, dt = fut.result()
            t_wait += time.perf_counter() - t0
            t_decode += dt
            shape = shape or tuple(host["depth"].shape)
            if tuple(host["depth"].shape) != shape:
                raise ValueError("%s: view %s's depth map %s differs in size from the scene's %s" % (scan_folder, names[v], tuple(host["depth"].shape), shape))
            if fuser is None:
                fuser = GipumaFuser(cams, shape[0], shape[1], device, disp_threshold=disp_threshold, num_consistent=num_consistent,
                                    depth_min=depth_min, depth_max=depth_max, normal_thresh=normal_thresh, capacity=capacity,
                                    return_skipped=return_skipped)
            d = {k: t.to(device, non_blocking=True) for k, t in host.items()}
            fuser.set_view(v, d["depth"], d["rgb"], conf_gate(d["conf"], prob_threshold, divide_uint8=True))
    events = [] if (on_gpu and stats is not None) else None
    fuser.run(on_view=on_view, events=events)
    res = fuser.accumulator.finalize()
    t_write = 0.0
    if plyfilename:
        t0 = time.perf_counter()
        fuser.accumulator.write_ply(plyfilename)
        t_write = time.perf_counter() - t0
    prefixes = [os.path.splitext(n)[0] for n in names]
    res["views"] = np.array([int(p) for p in prefixes], dtype=np.int64) if all(p.isdigit() for p in prefixes) else np.array(prefixes)
    if return_skipped:
        res["skipped"] = fuser.skipped.cpu().numpy()
    if stats is not None:
        if on_gpu:
            torch.cuda.synchronize(device)
        stats.update(wall=time.perf_counter() - t_wall, decode=t_decode, decode_wait=t_wait, write=t_write, views=len(names),
                     vertices=int(res["xyz"].shape[0]), flushes=fuser.accumulator.flushes,
                     gpu=sum(a.elapsed_time(b) for a, b in events) / 1e3 if events else float("nan"))
    return res


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Fuse a scene's depth maps into one coloured point cloud (binary PLY) by cross-view "
                                            "consistency: the gipuma step of the reference's test.py / test_tt.py, on the device")
    p.add_argument("--scan_folder", required=True, help="the scene's output folder: depth_est/, confidence/, cams/, images/")
    p.add_argument("--plyfilename", required=True)
    p.add_argument("--prob_threshold", type=float, default=0.5, help="prob confidence, for the gipuma route")
    p.add_argument("--disp_threshold", type=float, default=0.2, help="threshold of disparity, for the gipuma route")
    p.add_argument("--num_consistent", type=float, default=3, help="threshold of num view, for the gipuma route")
    p.add_argument("--depth_min", type=float, default=0.001)
    p.add_argument("--depth_max", type=float, default=100000.0)
    p.add_argument("--normal_thresh", type=float, default=360.0)
    p.add_argument("--device", default="cuda")
    a = p.parse_args(argv)
    st = {}
    res = fuse_scene_gipuma(a.scan_folder, a.plyfilename, prob_threshold=a.prob_threshold, disp_threshold=a.disp_threshold,
                            num_consistent=a.num_consistent, depth_min=a.depth_min, depth_max=a.depth_max, normal_thresh=a.normal_thresh,
                            device=a.device, stats=st)
    for vid, n in zip(res["views"], res["counts"]):
        print("ref-view %s: %d points" % (vid, n))
    print("saving the final model to %s (%d vertices, %.2f s)" % (a.plyfilename, res["xyz"].shape[0], st["wall"]))


if __name__ == "__main__":
    main()
