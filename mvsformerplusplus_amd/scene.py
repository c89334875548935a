"""A scene's depth inference, natively: a folder of ``images/``, ``cams/`` and ``pair.txt`` in, the folder of
``depth_est/``, ``confidence/``, ``cams/`` and ``images/`` out that ``pointcloud.fuse_scene`` / ``gipuma.fuse_scene_gipuma`` read - the
reference's ``save_depth`` (test.py:184-321) over ``MVSDataset`` (datasets/general_eval.py, ``mode="test"``).

    scene_samples(scan_folder, num_view, numdepth, interval_scale, max_h, max_w, dataset)
        the dataset contract on the host, numpy fp32 in the reference's operation order: one entry per pair.txt line that has source
        views, with every stage's projection matrices and the depth values, bit-equal to the reference's
    infer_scene(net, testpath, scans, outdir, ...)
        the driver: each image is decoded, uploaded and prepared (csrc/scene_kernels.hip) ONCE per scene into a view cache - the
        reference does it once per sample the image takes part in -, and with ``vit_cache`` the frozen ViT runs once per image too
    python -m mvsformerplusplus_amd.scene --config ... --resume ... --testpath ... --outdir ...       test.py's flags

Out of scope, each refused or skipped with a message: ``stage3`` configs, batches of more than one sample, DTU's ground-truth metrics
(``depth_metric.txt``).  ``fix_res`` is accepted and ignored: ``scale_mvs_input`` always resizes to max_w x max_h, so the reference's
second resize never fires.
"""
from __future__ import annotations

import argparse
import json
import os
import queue
import shutil
import threading
import time
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import data_io, ops

DATASETS = ("dtu", "tt", "eth3d", "general")
STAGES = ("stage1", "stage2", "stage3", "stage4")
TT_PAD = 4                      # rows replicated above and below a "tt" image (general_eval.py:115-116); its principal point moves with them


# ---------------------------------------------------------------- the dataset contract (general_eval.py:38-262, mode="test")
def read_pairs(pair_file: str, num_view: int):
    """build_list (general_eval.py:56-71): [(ref_view, src_views)] for every viewpoint that has sources; a list shorter than ``num_view``
    is padded with its first source up to ``num_view`` entries, then ``num_view - 1`` are kept (the reference's fill-and-truncate)."""
    metas = []
    with open(pair_file) as f:
        num_viewpoint = int(f.readline())
        for _ in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if len(src_views) > 0:
                if len(src_views) < num_view:
                    src_views += [src_views[0]] * (num_view - len(src_views))
                metas.append((ref_view, src_views[:num_view - 1]))
    return metas


def cam_filename(scan_folder: str, vid: int, dataset: str, use_short_range: bool = False) -> str:
    """general_eval.py:170-178: "tt" reads cams/ (or short_range_cameras/cams_<scan.lower()>/ next to the scene); every other dataset
    prefers cams_1/ and falls back to cams/."""
    name = "{:0>8}_cam.txt".format(vid)
    if dataset == "tt":
        if use_short_range:
            testpath, scan = os.path.split(os.path.normpath(scan_folder))
            return os.path.join(testpath, "short_range_cameras", "cams_{}".format(scan.lower()), name)
        return os.path.join(scan_folder, "cams", name)
    path = os.path.join(scan_folder, "cams_1", name)
    return path if os.path.exists(path) else os.path.join(scan_folder, "cams", name)


def read_cam_file(filename: str, interval_scale: float, ndepths: int, dataset: str):
    """general_eval.py:80-110 -> (intrinsics fp32 [3,3] with rows 0-1 divided by 4, extrinsics fp32 [4,4], depth_min, depth_interval)."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
    if dataset == "tt":
        intrinsics[1, 2] += TT_PAD
    intrinsics[:2, :] /= 4.0
    tokens = lines[11].split()
    depth_min = float(tokens[0])
    depth_interval = 2.5 if "cams_1" in filename else float(tokens[1])
    if len(tokens) >= 3:
        depth_max = depth_min + int(float(tokens[2])) * depth_interval
        depth_interval = (depth_max - depth_min) / ndepths
    if dataset == "eth3d":
        depth_max = float(tokens[1])
        depth_interval = (depth_max - depth_min) / ndepths
    depth_interval *= interval_scale
    return intrinsics, extrinsics, depth_min, depth_interval


def image_size(path: str):
    """(h, w) of an image file from its header (nothing is decoded)."""
    from PIL import Image
    with Image.open(path) as img:
        w, h = img.size
    return h, w


def scene_samples(scan_folder: str, num_view: int = 5, numdepth: int = 192, interval_scale: float = 1.06, max_h: int = 864,
                  max_w: int = 1152, dataset: str = "dtu", use_short_range: bool = False, fix_res: bool = False,
                  stage3: bool = False) -> List[dict]:
    """MVSDataset.__getitem__ (general_eval.py:154-262) for every sample of one scene, without the images:
    [{"ref", "view_ids", "proj_matrices": {"stageK": fp32 [V,2,4,4]}, "depth_values": fp32 [D], "depth_min", "depth_interval",
    "images": [path per view], "filename": "<scan>/{}/<ref:08d>{}"}].  ``fix_res`` is ignored (see the module docstring)."""
    if dataset not in DATASETS:
        raise ValueError("dataset must be one of %s, not %r" % (", ".join(DATASETS), dataset))
    if stage3:
        raise NotImplementedError("stage3 configs (three stages, the 1/4 .. 1/1 projection matrices) are not supported by the scene driver")
    if num_view < 2:
        raise ValueError("num_view must be at least 2 (the reference view and one source); got %d" % num_view)
    scan = os.path.basename(os.path.normpath(scan_folder))
    sizes, samples = {}, []
    for ref_view, src_views in read_pairs(os.path.join(scan_folder, "pair.txt"), num_view):
        view_ids = [ref_view] + src_views
        proj_matrices, images, depth_values, ref_range = [], [], None, None
        for i, vid in enumerate(view_ids):
            img_filename = os.path.join(scan_folder, "images", "{:0>8}.jpg".format(vid))
            if vid not in sizes:
                sizes[vid] = image_size(img_filename)
            h, w = sizes[vid]
            if dataset == "tt":
                h += 2 * TT_PAD
            intrinsics, extrinsics, depth_min, depth_interval = read_cam_file(cam_filename(scan_folder, vid, dataset, use_short_range),
                                                                              interval_scale, numdepth, dataset)
            scale_w = 1.0 * max_w / w                           # scale_mvs_input (general_eval.py:120-131): always to max_w x max_h
            scale_h = 1.0 * max_h / h
            intrinsics[0, :] *= scale_w
            intrinsics[1, :] *= scale_h
            proj_mat = np.zeros(shape=(2, 4, 4), dtype=np.float32)
            proj_mat[0, :4, :4] = extrinsics
            proj_mat[1, :3, :3] = intrinsics
            proj_matrices.append(proj_mat)
            images.append(img_filename)
            if i == 0:
                depth_values = np.arange(depth_min, depth_interval * (numdepth - 0.5) + depth_min, depth_interval, dtype=np.float32)
                ref_range = (depth_min, depth_interval)
        proj_matrices = np.stack(proj_matrices)
        ms = {}
        for name, factor in zip(STAGES, (0.5, None, 2, 4)):
            ms[name] = proj_matrices.copy()
            if factor is not None:
                ms[name][:, 1, :2, :] = proj_matrices[:, 1, :2, :] * factor
        samples.append({"ref": ref_view, "view_ids": view_ids, "proj_matrices": ms, "depth_values": depth_values, "depth_min": ref_range[0],
                        "depth_interval": ref_range[1], "images": images, "filename": scan + "/{}/" + "{:0>8}".format(ref_view) + "{}"})
    return samples


# ---------------------------------------------------------------- the driver
def decode_image(path: str) -> np.ndarray:
    """-> uint8 RGB [h, w, 3] (general_eval.py:112-114; the "tt" pad is the prepare kernel's)."""
    return data_io.read_img(path)


class ViewCache:
    """The prepared views of a scene, least recently used first: view id -> {"planar" fp32 [3,H,W], "rgb" uint8 [H,W,3], "levels" (the ViT's
    levels, or None), "event"}.  ``budget`` bytes (None: unbounded); an insert evicts the least recently used entries that the running
    sample does not hold until the cache fits again (one entry always stays)."""

    def __init__(self, budget: Optional[int] = None):
        self.budget = budget
        self.entries: "OrderedDict[int, dict]" = OrderedDict()
        self.bytes = 0
        self.hits = self.misses = self.evictions = 0

    @staticmethod
    def _size(entry: dict) -> int:
        ts = [entry["planar"], entry["rgb"]] + list(entry.get("levels") or [])
        return sum(t.numel() * t.element_size() for t in ts)

    def get(self, vid: int) -> Optional[dict]:
        entry = self.entries.get(vid)
        if entry is None:
            self.misses += 1
            return None
        self.entries.move_to_end(vid)
        self.hits += 1
        return entry

    def grow(self, vid: int) -> None:
        """An entry gained tensors (its ViT levels): account for them."""
        self.bytes += self._size(self.entries[vid]) - self.entries[vid]["bytes"]
        self.entries[vid]["bytes"] = self._size(self.entries[vid])

    def put(self, vid: int, entry: dict, held: Sequence[int] = ()) -> None:
        entry["bytes"] = self._size(entry)
        self.entries[vid] = entry
        self.bytes += entry["bytes"]
        self.trim(tuple(held) + (vid,))

    def trim(self, held: Sequence[int] = ()) -> None:
        if self.budget is None:
            return
        for old in list(self.entries):
            if self.bytes <= self.budget or len(self.entries) <= 1:
                break
            if old in held:
                continue
            self.bytes -= self.entries.pop(old)["bytes"]
            self.evictions += 1


def _write_pfm_rows(filename: str, rows: np.ndarray) -> None:
    """rows fp32 [H, W], the BOTTOM row first: the file data_io.save_pfm writes for the unflipped map."""
    with open(filename, "wb") as f:
        f.write(b"Pf\n")
        f.write(("%d %d\n" % (rows.shape[1], rows.shape[0])).encode("utf-8"))
        f.write(("%f\n" % -1).encode("utf-8"))               # little endian
        rows.astype("<f4", copy=False).tofile(f)


def _write_sample(folder: str, name: str, H: int, W: int, staging: np.ndarray, cam: np.ndarray) -> None:
    from PIL import Image
    n = H * W
    _write_pfm_rows(os.path.join(folder, "depth_est", name + ".pfm"), staging[:4 * n].view(np.float32).reshape(H, W))
    np.save(os.path.join(folder, "confidence", name + ".npy"), staging[4 * n:5 * n].reshape(H, W))
    data_io.write_cam(os.path.join(folder, "cams", name + "_cam.txt"), cam)
    Image.fromarray(staging[5 * n:8 * n].reshape(H, W, 3)).save(os.path.join(folder, "images", name + ".jpg"), quality=95)


def infer_scene(net: Callable, testpath: str, scans: Sequence[str], outdir: str, *, dataset: str = "dtu", num_view: int = 5,
                numdepth: int = 192, interval_scale: float = 1.06, max_h: int = 864, max_w: int = 1152,
                tmps: Sequence[float] = (5.0, 5.0, 5.0, 1.0), combine_reg_conf: bool = False, use_short_range: bool = False,
                fix_res: bool = False, stage3: bool = False, vit_cache: Optional[bool] = None, cache_bytes: Optional[int] = None, device=None,
                workers: int = 8, lookahead: int = 2, ring: int = 4, decoder: Callable[[str], np.ndarray] = decode_image,
                stats: Optional[dict] = None) -> Dict[str, List[int]]:
    """save_depth (test.py:184-321) for the scenes ``scans`` under ``testpath``: per sample ``net(imgs [1,V,3,H,W], proj_matrices,
    depth_values, tmp)`` and ``<outdir>/<scan>/depth_est/%08d.pfm``, ``confidence/%08d.npy`` (uint8), ``cams/%08d_cam.txt`` (the stage-4
    reference camera) and ``images/%08d.jpg`` (the resized image), plus the scene's ``pair.txt``.  -> {scan: [reference view ids]}.

    ``net``: a ``DINOv2MVSNet`` in eval mode on ``device`` (or any callable with its forward's signature).  Each image is decoded (on a pool
    of at most 16 ``workers`` threads, ``lookahead`` samples ahead), uploaded and prepared once per scene on a side stream into a ``ViewCache``
    of ``cache_bytes`` (None: every view of the scene stays); a sample's images are gathered from it into one reused buffer.  ``vit_cache``:
    the ViT's levels are computed once per view (``net.vit_levels``) and kept in the cache as well - bit-identical outputs, 28 % less time
    per scene at num_view 5; None (the default) = on where the network offers ``vit_levels``.  The outputs are packed on the device,
    copied into a ring of ``ring`` pinned buffers and written by a writer thread; the host waits for the device only where a ring slot
    comes round again.  ``stats`` (a dict) receives wall seconds, decode / cache / eviction counts per call."""
    if dataset not in DATASETS:
        raise ValueError("dataset must be one of %s, not %r" % (", ".join(DATASETS), dataset))
    device = torch.device(device if device is not None else "cuda")
    on_gpu = device.type == "cuda"
    if vit_cache is None:
        vit_cache = hasattr(net, "vit_levels")
    if vit_cache and not hasattr(net, "vit_levels"):
        raise ValueError("vit_cache=True needs a network with vit_levels() and forward(..., vit_levels=) (DINOv2MVSNet)")
    H, W = int(max_h), int(max_w)
    pad = TT_PAD if dataset == "tt" else 0
    tmp = [float(t) for t in tmps]
    t_wall = time.perf_counter()
    table = ops.normalise_table().to(device)
    main = torch.cuda.current_stream(device) if on_gpu else None
    side = torch.cuda.Stream(device) if on_gpu else None
    nbytes = 8 * H * W                                                  # 4 depth + 1 confidence + 3 image bytes per pixel
    slots = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=on_gpu) for _ in range(max(2, int(ring)))]
    free: "queue.Queue[int]" = queue.Queue()
    for k in range(len(slots)):
        free.put(k)
    jobs: "queue.Queue" = queue.Queue()
    failure: List[BaseException] = []

    def writer():
        while True:
            job = jobs.get()
            if job is None:
                return
            k, event, folder, name, cam = job
            try:
                if not failure:
                    if event is not None:
                        event.synchronize()
                    _write_sample(folder, name, H, W, slots[k].numpy(), cam)
            except BaseException as e:                                 # reported by the main thread
                failure.append(e)
            finally:
                free.put(k)

    thread = threading.Thread(target=writer, name="mvs-scene-writer", daemon=True)
    thread.start()
    if dataset == "dtu":
        print("infer_scene: DTU's ground-truth depth metrics (depth_metric.txt) are not computed; depth maps and confidences are written as usual")
    done: Dict[str, List[int]] = {}
    counts = {"decodes": 0, "samples": 0, "hits": 0, "misses": 0, "evictions": 0, "vit_views": 0}
    imgs = torch.empty(1, num_view, 3, H, W, dtype=torch.float32, device=device)
    staging = torch.empty(nbytes, dtype=torch.uint8, device=device)
    try:
        with ThreadPoolExecutor(max_workers=max(1, min(16, int(workers)))) as pool, torch.no_grad():
            for scan in scans:
                scan_folder = os.path.join(testpath, scan)
                samples = scene_samples(scan_folder, num_view, numdepth, interval_scale, H, W, dataset, use_short_range, fix_res, stage3)
                folder = os.path.join(outdir, scan)
                for sub in ("depth_est", "confidence", "cams", "images"):
                    os.makedirs(os.path.join(folder, sub), exist_ok=True)
                shutil.copyfile(os.path.join(scan_folder, "pair.txt"), os.path.join(folder, "pair.txt"))
                paths = {vid: p for s in samples for vid, p in zip(s["view_ids"], s["images"])}
                # every sample's projection matrices in one upload; one depth_values tensor per distinct range (the cascade's "auto"
                # policy decides, and synchronises, once per tensor object)
                projs = torch.from_numpy(np.stack([np.stack([s["proj_matrices"][k] for k in STAGES]) for s in samples])) if samples else None
                if samples and on_gpu:
                    projs = projs.pin_memory().to(device, non_blocking=True)
                ranges: Dict[tuple, torch.Tensor] = {}
                cache = ViewCache(cache_bytes)
                futures: Dict[int, object] = {}

                def fetch(vid):
                    img = np.ascontiguousarray(decoder(paths[vid]))
                    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                        raise ValueError("%s: the decoder must return uint8 RGB [h, w, 3]; got %s %s" % (paths[vid], img.dtype, img.shape))
                    t = torch.from_numpy(img)
                    return t.pin_memory() if on_gpu else t

                def submit(vid):
                    counts["decodes"] += 1                              # counted here, on the issuing thread
                    futures[vid] = pool.submit(fetch, vid)

                for i, s in enumerate(samples):
                    if failure:
                        raise failure[0]
                    for ahead in samples[i:i + 1 + max(0, int(lookahead))]:
                        for vid in ahead["view_ids"]:
                            if vid not in cache.entries and vid not in futures:
                                submit(vid)
                    vids = s["view_ids"]
                    for k, vid in enumerate(vids):
                        entry = cache.get(vid)
                        if entry is None:
                            if vid not in futures:                      # evicted between the look-ahead and its use
                                submit(vid)
                            host = futures.pop(vid).result()
                            if on_gpu:
                                with torch.cuda.stream(side):
                                    raw = host.to(device, non_blocking=True)
                                    planar, rgb = ops.image_prepare(raw, H, W, table, pad)
                                    event = torch.cuda.Event()
                                    event.record(side)
                                for t in (planar, rgb):
                                    t.record_stream(main)               # allocated on the side stream, read on the caller's
                                entry = {"planar": planar, "rgb": rgb, "levels": None, "event": event}
                            else:
                                planar, rgb = ops.image_prepare(host, H, W, table, pad)
                                entry = {"planar": planar, "rgb": rgb, "levels": None, "event": None}
                            cache.put(vid, entry, held=vids)
                        if entry["event"] is not None:
                            main.wait_event(entry["event"])
                        if vit_cache and entry["levels"] is None:
                            entry["levels"] = [t[0] for t in net.vit_levels(entry["planar"].unsqueeze(0))]
                            counts["vit_views"] += 1
                            cache.grow(vid)
                            cache.trim(vids)
                        imgs[0, k].copy_(entry["planar"])
                    held = [cache.entries[v] for v in vids]
                    key = (s["depth_min"], s["depth_interval"])
                    if key not in ranges:
                        dv = torch.from_numpy(s["depth_values"])[None]
                        ranges[key] = dv.pin_memory().to(device, non_blocking=True) if on_gpu else dv
                    pm = {name: projs[i, k][None] for k, name in enumerate(STAGES)}
                    if vit_cache:
                        levels = [torch.stack([e["levels"][l] for e in held])[None] for l in range(len(held[0]["levels"]))]
                        out = net(imgs, pm, ranges[key], tmp, vit_levels=levels)
                    else:
                        out = net(imgs, pm, ranges[key], tmp)
                    depth, conf = out["refined_depth"], out["photometric_confidence"]
                    if depth.shape[0] != 1 or tuple(depth.shape[-2:]) != (H, W):
                        raise ValueError("the network returned refined_depth %s for one %d x %d sample" % (tuple(depth.shape), H, W))
                    reg = out["stage4"]["photometric_confidence"][0] if combine_reg_conf else None
                    ops.depth_outputs_pack(depth[0], conf[0], reg, out=staging[:5 * H * W])
                    staging[5 * H * W:].copy_(held[0]["rgb"].reshape(-1))
                    slot = free.get()                                   # waits for the writer only when the ring has come round
                    if failure:
                        raise failure[0]
                    slots[slot].copy_(staging, non_blocking=True)
                    event = None
                    if on_gpu:
                        event = torch.cuda.Event()
                        event.record(main)
                    jobs.put((slot, event, folder, "{:0>8}".format(s["ref"]), s["proj_matrices"]["stage4"][0].copy()))
                    counts["samples"] += 1
                done[scan] = [s["ref"] for s in samples]
                for name in ("hits", "misses", "evictions"):
                    counts[name] += getattr(cache, name)
    finally:
        jobs.put(None)
        thread.join()
    if failure:
        raise failure[0]
    if on_gpu:
        torch.cuda.synchronize(device)
    if stats is not None:
        stats.update(counts, wall=time.perf_counter() - t_wall)
    return done


# ---------------------------------------------------------------- the command line (test.py's flags)
def _int_list(text):
    return [int(x) for x in str(text).split(",") if x != ""]


def _float_list(text):
    return [float(x) for x in str(text).split(",") if x != ""]


def load_network(config: str, resume: Optional[str], device, ndepths: Optional[str] = None, depth_interals_ratio: Optional[str] = None):
    """The native network of a reference config (JSON, ``arch.args``) with a released checkpoint loaded."""
    from .network import DINOv2MVSNet
    with open(config) as f:
        cfg = json.load(f)
    if cfg.get("data_loader") and cfg["data_loader"][0].get("args", {}).get("stage3", False):
        raise NotImplementedError("stage3 configs are not supported by the scene driver")
    args = dict(cfg["arch"]["args"])
    if ndepths:
        args["ndepths"] = _int_list(ndepths)
    if depth_interals_ratio:
        args["depth_interals_ratio"] = _float_list(depth_interals_ratio)
    net = DINOv2MVSNet(args)
    if resume:
        net.load_checkpoint(resume)
    return net.to(device).eval()


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Depth inference over scenes of images/, cams/ and pair.txt: the save_depth step of the reference's "
                                            "test.py on the device, optionally followed by the point-cloud fusion")
    p.add_argument("--config", required=True, help="the reference's JSON config (arch.args is read)")
    p.add_argument("--resume", default=None, help="a released checkpoint")
    p.add_argument("--dataset", default="dtu", choices=DATASETS)
    p.add_argument("--testpath", help="folder of scenes")
    p.add_argument("--testpath_single_scene", help="one scene's folder")
    p.add_argument("--testlist", help="text file of scene names, one per line")
    p.add_argument("--outdir", required=True, help="output folder; _<max_w>x<max_h> is appended, as test.py does")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--numdepth", type=int, default=192)
    p.add_argument("--ndepths", type=str, default=None)
    p.add_argument("--depth_interals_ratio", type=str, default=None)
    p.add_argument("--interval_scale", type=float, required=True)
    p.add_argument("--num_view", type=int, default=5)
    p.add_argument("--max_h", type=int, default=864)
    p.add_argument("--max_w", type=int, default=1152)
    p.add_argument("--fix_res", action="store_true", help="accepted and ignored: every image is resized to max_w x max_h anyway")
    p.add_argument("--tmps", default="5,5,5,1", type=str)
    p.add_argument("--combine_reg_conf", action="store_true")
    p.add_argument("--use_short_range", action="store_true")
    p.add_argument("--filter_method", type=str, default="none", choices=["none", "pcd", "dpcd", "gipuma"])
    p.add_argument("--conf", type=float, default=0.5)
    p.add_argument("--thres_view", type=int, default=2)
    p.add_argument("--thres_disp", type=float, default=1.0)
    p.add_argument("--dist_base", type=float, default=4.0)
    p.add_argument("--rel_diff_base", type=float, default=1300)
    p.add_argument("--prob_threshold", type=float, default=0.5)
    p.add_argument("--disp_threshold", type=float, default=0.2)
    p.add_argument("--num_consistent", type=float, default=3)
    p.add_argument("--no_vit_cache", action="store_true", help="run the frozen ViT once per sample, as the reference does, instead of once per image")
    p.add_argument("--cache_gb", type=float, default=None, help="byte budget of the view cache (default: a scene's views all stay)")
    p.add_argument("--device", default="cuda")
    a = p.parse_args(argv)
    if a.batch_size != 1:
        raise NotImplementedError("the scene driver runs one sample per forward (--batch_size 1)")
    if a.testpath_single_scene:
        a.testpath = os.path.dirname(os.path.normpath(a.testpath_single_scene))
        scans = [os.path.basename(os.path.normpath(a.testpath_single_scene))]
    elif a.testlist and a.testlist != "all":
        with open(a.testlist) as f:
            scans = [line.strip() for line in f if line.strip()]
    else:
        scans = sorted(d for d in os.listdir(a.testpath) if os.path.exists(os.path.join(a.testpath, d, "pair.txt")))
    outdir = a.outdir + "_%dx%d" % (a.max_w, a.max_h)
    net = load_network(a.config, a.resume, a.device, a.ndepths, a.depth_interals_ratio)
    st = {}
    infer_scene(net, a.testpath, scans, outdir, dataset=a.dataset, num_view=a.num_view, numdepth=a.numdepth, interval_scale=a.interval_scale,
                max_h=a.max_h, max_w=a.max_w, tmps=_float_list(a.tmps), combine_reg_conf=a.combine_reg_conf,
                use_short_range=a.use_short_range, fix_res=a.fix_res, vit_cache=not a.no_vit_cache,
                cache_bytes=None if a.cache_gb is None else int(a.cache_gb * (1 << 30)), device=a.device, stats=st)
    print("depth maps of %d samples (%d images decoded) in %.2f s -> %s" % (st["samples"], st["decodes"], st["wall"], outdir))
    for scan in scans:
        folder, ply = os.path.join(outdir, scan), os.path.join(outdir, scan + ".ply")
        if a.filter_method in ("pcd", "dpcd"):
            from . import pointcloud
            res = pointcloud.fuse_scene(folder, os.path.join(a.testpath, scan), ply, method=a.filter_method,
                                        convention="tt" if a.dataset == "tt" else "dtu", conf=a.conf, thres_view=a.thres_view,
                                        thres_disp=a.thres_disp, dist_base=a.dist_base, rel_diff_base=a.rel_diff_base, device=a.device)
            print("%s: %d vertices" % (ply, res["xyz"].shape[0]))
        elif a.filter_method == "gipuma":
            from . import gipuma
            res = gipuma.fuse_scene_gipuma(folder, ply, prob_threshold=a.prob_threshold, disp_threshold=a.disp_threshold,
                                           num_consistent=a.num_consistent, device=a.device)
            print("%s: %d vertices" % (ply, res["xyz"].shape[0]))


if __name__ == "__main__":
    main()
