"""A scene's filtered depth maps as ONE coloured point cloud (binary PLY): the last step of the reference's evaluation pipeline,
``filter_depth`` / ``dynamic_filter_depth`` of test.py (:387-442 / :445-517) and test_tt.py, selected there by
``--filter_method pcd|dpcd`` ("back-project -> PLY via plyfile").

Per reference view the HIP filter (csrc/fusion_kernels.hip) writes the final mask and the world points; the HIP compaction
(csrc/pointcloud_kernels.hip) appends the kept pixels, row-major, as packed 15-byte PLY vertex records to a device-resident scene
buffer.  Nothing synchronises per view: the host only tracks an upper bound on the record count (the pixels enqueued since the
last flush) and copies the buffer out when the next view could overflow it.

    acc = PointCloudAccumulator("cuda:0")
    for each reference view:  acc.add_view(ref_depth, ref_conf, srcs_depth, srcs_conf, ref_cam, srcs_cam, rgb, method="dpcd")
    acc.write_ply("scan1.ply")

``fuse_scene`` is the whole driver (pair file, decoding on a small thread pool, device-resident maps) and
``python -m mvsformerplusplus_amd.pointcloud`` its command line.
"""
from __future__ import annotations

import argparse
import os
import time
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import data_io, ops

REC = ops.PLY_RECORD_BYTES
METHODS = ("pcd", "dpcd")
CONVENTIONS = ("dtu", "tt")


def _vertices(records: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    v = records.view(data_io.PLY_VERTEX_DTYPE)
    return (np.stack([v[c] for c in "xyz"], -1).astype(np.float32),
            np.stack([v[c] for c in ("red", "green", "blue")], -1).astype(np.uint8))


class PointCloudAccumulator:
    """Device-resident PLY body of one scene, views appended in call order.

    capacity: records the device buffer holds (15 bytes each; the default, 2**24, is 240 MB).  A view larger than the buffer
    grows it."""

    def __init__(self, device, capacity: int = 1 << 24):
        self.device = torch.device(device)
        if not 1 <= int(capacity) < 1 << 31:
            raise ValueError("PointCloudAccumulator: capacity must be in [1, 2**31)")
        self.capacity = int(capacity)
        self._records = torch.empty(self.capacity * REC, dtype=torch.uint8, device=self.device)
        self._counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._view_counts = torch.zeros(64, dtype=torch.int32, device=self.device)
        self._nviews = 0
        self._bound = 0                   # upper bound on the records in the device buffer (pixels appended since the last flush)
        self._chunks: List[np.ndarray] = []
        self.flushes = 0

    # ---- compaction ----
    def append(self, mask: torch.Tensor, points: torch.Tensor, rgb: torch.Tensor) -> None:
        """One view: mask [h,w] (bool / uint8), points [3,h,w] fp32, rgb [h,w,3] uint8, all on the accumulator's device."""
        h, w = mask.shape[-2:]
        hw = int(h) * int(w)
        if hw > self.capacity:
            self._flush()
            self.capacity = hw
            self._records = torch.empty(hw * REC, dtype=torch.uint8, device=self.device)
        elif self._bound + hw > self.capacity:
            self._flush()
        if self._nviews == self._view_counts.numel():
            self._view_counts = torch.cat([self._view_counts, torch.zeros_like(self._view_counts)])
        ops.pointcloud_append(mask, points, rgb, self._records, self._counter, self._view_counts, self._nviews)
        self._nviews += 1
        self._bound += hw

    def add_view(self, ref_depth, ref_conf, srcs_depth, srcs_conf, ref_cam, srcs_cam, rgb, method: str = "dpcd", *, conf: float = 0.5,
                 thres_view: int = 2, thres_disp: float = 1.0, dist_base: float = 4.0, rel_diff_base: float = 1300.0) -> Dict[str, torch.Tensor]:
        """Filter one reference view (test.py:393-409 for "pcd", :455-483 for "dpcd") and append its kept pixels.  Maps as in
        fusion.filter_depth: ref_depth [h,w] (or [1,1,h,w]), ref_conf [h,w], srcs_depth [v,h,w] (or [1,v,1,h,w]), srcs_conf [v,h,w]
        (pcd only; None = no gating), cameras [2,4,4] / [v,2,4,4]; rgb [h,w,3] uint8.  Confidences are compared with `conf`
        as they are given.  Returns the filter's outputs (depth, geo_mask, mask [1,h,w], points [1,3,h,w])."""
        if method not in METHODS:
            raise ValueError("add_view: method must be 'pcd' or 'dpcd', not %r" % (method,))
        h, w = ref_depth.shape[-2:]
        rd = ops._f32c(ref_depth).reshape(1, h, w)
        sd = ops._f32c(srcs_depth).reshape(1, -1, h, w)
        v = sd.shape[1]
        rcf = ops._f32c(ref_conf).reshape(1, h, w)
        rc, sc = ops._f32c(ref_cam).reshape(1, 2, 4, 4), ops._f32c(srcs_cam).reshape(1, v, 2, 4, 4)
        if method == "pcd":
            scf = None if srcs_conf is None else ops._f32c(srcs_conf).reshape(1, v, h, w)
            out = ops.fusion_filter(False, rd, sd, rc, sc, ref_conf=rcf, srcs_conf=scf, conf_thresh=conf, p0=thres_disp, p1=0.01,
                                    vthresh=thres_view)
        else:
            out = ops.fusion_filter(True, rd, sd, rc, sc, ref_conf=rcf, conf_thresh=conf, p0=dist_base, p1=rel_diff_base)
        self.append(out["mask"][0], out["points"][0], rgb)
        return out

    # ---- results ----
    def _flush(self) -> None:
        if self._bound == 0:
            return
        n = int(self._counter.item()) & 0xffffffff                  # synchronises with the stream
        if n > self.capacity:
            raise RuntimeError("PointCloudAccumulator: %d records overflowed the buffer of %d" % (n, self.capacity))
        chunk = self._records[:n * REC].cpu().numpy()
        self._chunks.append(chunk if self._records.is_cuda else chunk.copy())       # .cpu() of a host buffer is the buffer itself
        self._counter.zero_()
        self._bound = 0
        self.flushes += 1

    def records(self) -> np.ndarray:
        """The packed PLY body so far (uint8 [N*15]); synchronises."""
        self._flush()
        if len(self._chunks) != 1:
            self._chunks = [np.concatenate(self._chunks) if self._chunks else np.zeros(0, np.uint8)]
        return self._chunks[0]

    def finalize(self) -> Dict[str, np.ndarray]:
        """-> {"xyz": [N,3] float32, "rgb": [N,3] uint8, "counts": [views] int64 (kept pixels per view, call order)}."""
        rec = self.records()
        xyz, rgb = _vertices(rec)
        counts = self._view_counts[:self._nviews].cpu().numpy().astype(np.int64)
        return {"xyz": xyz, "rgb": rgb, "counts": counts}

    def write_ply(self, path: str) -> int:
        """Write the binary PLY (data_io.ply_header + the records as they are); -> the vertex count."""
        rec = self.records()
        data_io.write_ply_records(path, rec)
        return rec.size // REC


# ---------------------------------------------------------------- the scene driver
def _min_passing(passing: np.ndarray) -> int:
    """passing[c] for c = 0..255 (monotone) -> the smallest passing value (256: none)."""
    idx = np.flatnonzero(passing)
    return int(idx[0]) if idx.size else 256


def conf_gate(conf: torch.Tensor, thresh: float, divide_uint8: bool) -> torch.Tensor:
    """The reference's confidence test as a 0/1 map (bool), exactly as it decides it:
      * a float map: ``conf > thresh`` in the map's precision (test.py:389 / :454 on float32 tensors);
      * a uint8 map divided by 255 (the reference view, test.py:354-355; the sources under test_tt.py): ``conf / 255 > thresh``
        in float64, the dtype numpy's division hands to torch;
      * a uint8 map not divided (the sources under test.py, :389-392): ``conf > thresh`` with the uint8 values promoted to float32."""
    if conf.dtype != torch.uint8:
        return conf > thresh
    c = np.arange(256)
    passing = (c / 255.0 > thresh) if divide_uint8 else (c.astype(np.float32) > np.float32(thresh))
    k = _min_passing(passing)
    return conf >= k if k < 256 else torch.zeros_like(conf, dtype=torch.bool)


def scene_views(scan_folder: str, pair_folder: Optional[str] = None, convention: str = "dtu",
                n_src_views: int = 10) -> List[Tuple[int, List[int]]]:
    """The reference views of a scene in the order the drivers emit them, each with the sources that have a camera file.
    convention "dtu": pair.txt, first `n_src_views` sources (test.py:327-338); "tt": new_pair.txt, else pair.txt, padded / cut to
    fusion_view = n_src_views (test_tt.py:142-156, :353-357).  A source whose cams/<id>_cam.txt is missing is skipped
    (test.py:356-357).  The drivers collect the views in a dict keyed by the reference id (test.py:424, :428): a repeated
    reference keeps its first place and its last entry's data."""
    pair_folder = pair_folder or scan_folder
    if convention == "tt":
        pf = os.path.join(pair_folder, "new_pair.txt")
        if not os.path.exists(pf):
            pf = os.path.join(pair_folder, "pair.txt")
    elif convention == "dtu":
        pf = os.path.join(pair_folder, "pair.txt")
    else:
        raise ValueError("convention must be 'dtu' or 'tt', not %r" % (convention,))
    views: "OrderedDict[int, List[int]]" = OrderedDict()
    for ref, srcs in data_io.read_pair_file(pf, convention, n_src_views):
        srcs = srcs[:n_src_views]
        views[ref] = [s for s in srcs if os.path.exists(os.path.join(scan_folder, "cams", "{:0>8}_cam.txt".format(s)))]
    return list(views.items())


def _cam(path: str) -> np.ndarray:
    K, E = data_io.read_camera_parameters(path)
    cam = np.zeros((2, 4, 4), dtype=np.float32)
    cam[0] = E
    cam[1, :3, :3] = K
    cam[1, 3, 3] = 1.0
    return cam


def _decode(scan_folder: str, vid: int, with_image: bool, pin: bool):
    """Worker thread: one view's depth, confidence, camera (and image) -> host tensors (pinned for a device upload)."""
    t0 = time.perf_counter()
    name = "{:0>8}".format(vid)
    depth = np.ascontiguousarray(data_io.read_pfm(os.path.join(scan_folder, "depth_est", name + ".pfm"))[0], dtype=np.float32)
    conf = np.load(os.path.join(scan_folder, "confidence", name + ".npy"))
    if conf.shape != depth.shape:
        raise ValueError("%s: confidence map %s does not match the depth map %s" % (os.path.join(scan_folder, "confidence", name + ".npy"),
                                                                                   conf.shape, depth.shape))
    if conf.dtype != np.uint8:
        conf = conf.astype(np.float32)
    out = {"depth": torch.from_numpy(depth), "conf": torch.from_numpy(np.ascontiguousarray(conf)),
           "cam": torch.from_numpy(_cam(os.path.join(scan_folder, "cams", name + "_cam.txt")))}
    if with_image:
        path = os.path.join(scan_folder, "images", name + ".jpg")
        img = data_io.read_img(path)
        if img.shape[:2] != depth.shape:
            raise ValueError("%s: image size %dx%d differs from the depth map's %dx%d" % (path, img.shape[1], img.shape[0], depth.shape[1], depth.shape[0]))
        out["rgb"] = torch.from_numpy(img)
    if pin:
        out = {k: t.pin_memory() for k, t in out.items()}
    return out, time.perf_counter() - t0


def fuse_scene(scan_folder: str, pair_folder: Optional[str] = None, plyfilename: Optional[str] = None, method: str = "dpcd",
               convention: str = "dtu", conf: float = 0.5, thres_view: int = 2, thres_disp: float = 1.0, dist_base: float = 4.0,
               rel_diff_base: float = 1300.0, n_src_views: int = 10, device=None, capacity: int = 1 << 24, workers: int = 4,
               lookahead: int = 4, stats: Optional[dict] = None, on_view=None) -> Dict[str, np.ndarray]:
    """filter_depth / dynamic_filter_depth of test.py (convention "dtu") or test_tt.py ("tt") for one scene: every reference
    view filtered on the device, its kept pixels appended to one point cloud, written to `plyfilename` (when given).

    Each view's depth, confidence, camera and image is read at most once, on a pool of `workers` (<= 4) threads running
    `lookahead` reference views ahead of the device; depth and confidence stay on the device while a later reference view
    still uses them.  Confidence maps follow the reference per convention: the reference view's map is divided by 255 when
    it is uint8; the sources' maps only under "tt" (conf_gate).  "pcd" gates source depths by their confidence, "dpcd" does
    not.  -> {"xyz", "rgb", "counts" (per reference view), "views" (reference ids, emission order)}.
    stats (optional dict) receives wall / decode / decode_wait / gpu / write seconds (gpu from events, read at the end).
    on_view (optional) is called as on_view(ref_id, filter outputs) after each view is enqueued (inspection; no sync here)."""
    if method not in METHODS:
        raise ValueError("method must be 'pcd' or 'dpcd', not %r" % (method,))
    device = torch.device(device if device is not None else "cuda")
    on_gpu = device.type == "cuda"
    t_wall = time.perf_counter()
    plan = scene_views(scan_folder, pair_folder, convention, n_src_views)
    first, last = {}, {}
    for i, (ref, srcs) in enumerate(plan):
        for vid in [ref] + srcs:
            first.setdefault(vid, i)
            last[vid] = i
    is_ref = {ref for ref, _ in plan}
    order = sorted(first, key=lambda k: (first[k], k != plan[first[k]][0]))      # decode in order of first use
    acc = PointCloudAccumulator(device, capacity)
    resident: Dict[int, dict] = {}
    futures: Dict[int, object] = {}
    t_decode, t_wait, events, shape = 0.0, 0.0, [], None
    with ThreadPoolExecutor(max_workers=max(1, min(4, int(workers)))) as pool:
        nxt = 0
        for i, (ref, srcs) in enumerate(plan):
            while nxt < len(order) and first[order[nxt]] <= i + lookahead:
                vid = order[nxt]
                futures[vid] = pool.submit(_decode, scan_folder, vid, vid in is_ref, on_gpu)
                nxt += 1
            for vid in [ref] + srcs:
                if vid in resident:
                    continue
                t0 = time.perf_counter()
                host, dt = futures.pop(vid).result()
                t_wait += time.perf_counter() - t0
                t_decode += dt
                shape = shape or tuple(host["depth"].shape)
                if tuple(host["depth"].shape) != shape:
                    raise ValueError("%s: view %d's depth map %s differs in size from the scene's %s" % (scan_folder, vid, tuple(host["depth"].shape), shape))
                d = {k: t.to(device, non_blocking=True) for k, t in host.items()}
                if method == "pcd":
                    d["src_gate"] = conf_gate(d["conf"], conf, divide_uint8=convention == "tt")
                resident[vid] = d
            if not srcs:
                raise ValueError("%s: reference view %d has no source view with a camera file" % (scan_folder, ref))
            r = resident[ref]
            if on_gpu and stats is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            out = acc.add_view(r["depth"], conf_gate(r["conf"], conf, divide_uint8=True).float(),
                         torch.stack([resident[s]["depth"] for s in srcs]),
                         torch.stack([resident[s]["src_gate"] for s in srcs]).float() if method == "pcd" else None,
                         r["cam"], torch.stack([resident[s]["cam"] for s in srcs]), r["rgb"], method,
                         conf=0.5, thres_view=thres_view, thres_disp=thres_disp, dist_base=dist_base, rel_diff_base=rel_diff_base)
            if on_gpu and stats is not None:
                ev[1].record()
                events.append(ev)
            if on_view is not None:
                on_view(ref, out)
            for vid in [ref] + srcs:
                if last[vid] == i:
                    resident.pop(vid, None)
    res = acc.finalize()
    t_write = 0.0
    if plyfilename:
        t0 = time.perf_counter()
        acc.write_ply(plyfilename)
        t_write = time.perf_counter() - t0
    res["views"] = np.array([ref for ref, _ in plan], dtype=np.int64)
    if stats is not None:
        if on_gpu:
            torch.cuda.synchronize(device)
        stats.update(wall=time.perf_counter() - t_wall, decode=t_decode, decode_wait=t_wait, write=t_write, views=len(plan),
                     vertices=int(res["xyz"].shape[0]), flushes=acc.flushes,
                     gpu=sum(a.elapsed_time(b) for a, b in events) / 1e3 if events else float("nan"))
    return res


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Fuse a scene's filtered depth maps into one coloured point cloud (binary PLY), "
                                            "the pcd / dpcd step of the reference's test.py / test_tt.py")
    p.add_argument("--scan_folder", required=True, help="the scene's output folder: depth_est/, confidence/, cams/, images/")
    p.add_argument("--pair_folder", default=None, help="folder of pair.txt / new_pair.txt (default: scan_folder)")
    p.add_argument("--plyfilename", required=True)
    p.add_argument("--filter_method", default="dpcd", choices=METHODS)
    p.add_argument("--convention", default="dtu", choices=CONVENTIONS, help="dtu = test.py, tt = test_tt.py")
    p.add_argument("--conf", type=float, default=0.5, help="prob confidence")
    p.add_argument("--thres_view", type=int, default=2, help="threshold of num view")
    p.add_argument("--thres_disp", type=float, default=1.0, help="threshold of disparity")
    p.add_argument("--dist_base", type=float, default=4.0)
    p.add_argument("--rel_diff_base", type=float, default=1300)
    p.add_argument("--fusion_view", type=int, default=10, help="source views per reference view (tt: views incl. the reference)")
    p.add_argument("--device", default="cuda")
    a = p.parse_args(argv)
    st = {}
    res = fuse_scene(a.scan_folder, a.pair_folder, a.plyfilename, method=a.filter_method, convention=a.convention, conf=a.conf,
                     thres_view=a.thres_view, thres_disp=a.thres_disp, dist_base=a.dist_base, rel_diff_base=a.rel_diff_base,
                     n_src_views=a.fusion_view, device=a.device, stats=st)
    for vid, n in zip(res["views"], res["counts"]):
        print("ref-view %08d: %d points" % (vid, n))
    print("saving the final model to %s (%d vertices, %.2f s)" % (a.plyfilename, res["xyz"].shape[0], st["wall"]))


if __name__ == "__main__":
    main()
