"""COLMAP model -> MVSNet input folder (`cams/%08d_cam.txt`, `pair.txt`, `images/%08d.jpg`): the reference's colmap2mvsnet.py
with its view selection and depth values on the device.

    python -m mvsformerplusplus_amd.colmap2mvsnet --dense_folder D [--max_d 256] [--interval_scale 1] [--theta0 5]
                                                  [--sigma1 1] [--sigma2 10] [--test] [--convert_format]

The model is read from D/sparse (.bin when present, else .txt), the images from D/images_col.  Differences from the reference,
each deliberate: it runs on numpy 2 without OpenCV; cos is clamped to [-1, 1] and a point at a camera centre contributes 0
(the reference yields NaN); an image without a valid observation or a point id missing from points3D raises ValueError; --test
computes and prints but writes nothing; --convert_format re-encodes with PIL at JPEG quality 95; no process pool; equal scores
are listed by descending view index.
"""
from __future__ import annotations

import argparse
import os
import shutil
from typing import Dict, Tuple

import numpy as np
import torch

from . import colmap, ops

MAX_OBSERVATIONS = 2 ** 31 - 1
PAIR_COUNT = 10


def _default_device() -> str:
    return "cuda:0"


def check_sizes(n_images: int, n_obs: int) -> None:
    """The flag and score matrices take 9 N^2 bytes; observation indices are 32-bit on the device."""
    if n_images < 1:
        raise ValueError("the model has no registered image")
    if n_images > ops.COLMAP_MAX_IMAGES:
        raise ValueError("%d images: at most %d are supported (the flag and score matrices take 9 * N^2 = %d bytes)"
                         % (n_images, ops.COLMAP_MAX_IMAGES, 9 * n_images * n_images))
    if n_obs > MAX_OBSERVATIONS:
        raise ValueError("%d observations: fewer than 2^31 = %d are supported" % (n_obs, MAX_OBSERVATIONS + 1))


class Observations:
    """The model's valid observations on `device`: image index and dense point index (position in points3D's file order) of every
    point3D_ids entry other than -1, in file order, duplicates kept."""

    def __init__(self, model: colmap.Model, device):
        im, pt = model.images, model.points3D
        n, m, p = len(im), len(im.point3D_ids), len(pt)
        check_sizes(n, m)
        self.n_images, self.n_points = n, p
        pid = torch.from_numpy(im.point3D_ids).to(device)
        img = torch.repeat_interleave(torch.arange(n, device=device), torch.from_numpy(np.diff(im.obs_ptr)).to(device))
        valid = pid != -1
        pid, img = pid[valid], img[valid]
        if pid.numel() and p == 0:
            raise ValueError("point3D id %d of image %r is not in points3D (points3D is empty)" % (int(pid[0]), im.names[int(img[0])]))
        if p:
            sids, order = torch.sort(torch.from_numpy(pt.ids).to(device))
            if p > 1 and bool((sids[1:] == sids[:-1]).any()):
                raise ValueError("points3D holds a point id twice")
            pos = torch.searchsorted(sids, pid).clamp_(max=p - 1)
            found = sids[pos] == pid
            if not bool(found.all()):
                k = int(torch.nonzero(~found)[0, 0])
                raise ValueError("point3D id %d of image %r is not in points3D" % (int(pid[k]), im.names[int(img[k])]))
            dense = order[pos]
        else:
            dense = pid
        self.counts = torch.bincount(img, minlength=n).cpu().numpy()
        empty = np.nonzero(self.counts == 0)[0]
        if len(empty):
            raise ValueError("image %r (id %d) has no valid observation: its depth range is undefined"
                             % (im.names[empty[0]], int(im.ids[empty[0]])))
        self.img, self.pt = img, dense
        self.device = torch.device(device)


def depth_bounds(obs: Observations, xyz: torch.Tensor, E: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(depth_min, depth_max) per image: zs = z of every valid entry under [R|t], sorted; zs[int(n * .01)], zs[int(n * .99)]
    (colmap2mvsnet.py:344-357)."""
    erow = torch.from_numpy(np.ascontiguousarray(E[:, 2, :])).to(obs.device)
    z = ops.colmap_depths(obs.img.to(torch.int32), obs.pt.to(torch.int32), xyz, erow)
    # per-image ascending order: a stable sort by z, then a stable sort by image
    p1 = torch.sort(z, stable=True).indices
    p2 = torch.sort(obs.img[p1], stable=True).indices
    zs = z[p1[p2]]
    n = obs.counts.astype(np.int64)
    start = np.cumsum(n) - n
    lo = start + (n.astype(np.float64) * .01).astype(np.int64)       # int(len(zs) * .01): a float product, truncated
    hi = start + (n.astype(np.float64) * .99).astype(np.int64)
    at = torch.from_numpy(np.stack([lo, hi])).to(obs.device)
    b = zs[at].cpu().numpy()
    return b[0], b[1]


def score_matrix(obs: Observations, xyz: torch.Tensor, E: np.ndarray, theta0: float = 5, sigma1: float = 1, sigma2: float = 10) -> torch.Tensor:
    """score [N, N] fp64 on the device (colmap2mvsnet.py:378-410; the kernel's header comment states the definition)."""
    n, p = obs.n_images, obs.n_points
    dev = obs.device
    if obs.img.numel() == 0:
        return torch.zeros(n, n, dtype=torch.float64, device=dev)
    key = obs.img * max(p, 1) + obs.pt
    ukey, mult = torch.unique(key, sorted=True, return_counts=True)
    uimg, upt = ukey // max(p, 1), ukey % max(p, 1)
    img_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    img_ptr[1:] = torch.cumsum(torch.bincount(uimg, minlength=n), 0)
    track_len = torch.bincount(upt, minlength=p)
    pt_ptr = torch.zeros(p + 1, dtype=torch.int64, device=dev)
    pt_ptr[1:] = torch.cumsum(track_len, 0)
    pt_imgs = uimg[torch.sort(upt, stable=True).indices]         # ascending images per point: ukey is sorted by (image, point)
    max_pairs = min(n * (n - 1) // 2, int((track_len * (track_len - 1) // 2).sum()))
    centres = torch.from_numpy(colmap.camera_centres(E)).to(dev)
    i32 = lambda t: t.to(torch.int32)
    return ops.colmap_scores(i32(img_ptr), i32(upt), i32(mult), i32(pt_ptr), i32(pt_imgs), xyz, centres, theta0=float(theta0),
                             den1=2 * float(sigma1) ** 2, den2=2 * float(sigma2) ** 2, max_pairs=max_pairs)


def select_views(score: torch.Tensor, k: int = PAIR_COUNT) -> Tuple[np.ndarray, np.ndarray]:
    """Per row the min(k, N) largest scores, diagonal included; ties by descending view index (a stable descending sort of the
    reversed row).  Returns (views int64 [N, k'], scores fp64 [N, k'])."""
    n = score.shape[0]
    vals, idx = torch.sort(score.flip(1), dim=1, descending=True, stable=True)
    k = min(k, n)
    return (n - 1 - idx[:, :k]).cpu().numpy(), vals[:, :k].cpu().numpy()


def inverse_depth_count(K: np.ndarray, E: np.ndarray, depth_min: float, depth_max: float) -> float:
    """Depth count for max_d == 0 (colmap2mvsnet.py:360-373), the reference's expressions in its order."""
    image_r, image_t = E[0:3, 0:3], E[0:3, 3]
    p1 = [K[0, 2], K[1, 2], 1]
    p2 = [K[0, 2] + 1, K[1, 2], 1]
    P1 = np.matmul(np.linalg.inv(K), p1) * depth_min
    P1 = np.matmul(np.linalg.inv(image_r), (P1 - image_t))
    P2 = np.matmul(np.linalg.inv(K), p2) * depth_min
    P2 = np.matmul(np.linalg.inv(image_r), (P2 - image_t))
    return (1 / depth_min - 1 / depth_max) / (1 / depth_min - 1 / (depth_min + np.linalg.norm(P2 - P1)))


def cam_text(E: np.ndarray, K: np.ndarray, depth_range) -> str:
    """One cams/%08d_cam.txt, byte for byte the reference's (colmap2mvsnet.py:417-434)."""
    s = ["extrinsic\n"]
    for j in range(4):
        s.append("".join(str(np.float64(E[j, k])) + " " for k in range(4)) + "\n")
    s.append("\nintrinsic\n")
    for j in range(3):
        s.append("".join(str(np.float64(K[j, k])) + " " for k in range(3)) + "\n")
    s.append("\n%f %f %f %f\n" % tuple(depth_range))
    return "".join(s)


def pair_text(views: np.ndarray, scores: np.ndarray) -> str:
    """pair.txt, byte for byte the reference's format (colmap2mvsnet.py:436-442)."""
    s = ["%d\n" % len(views)]
    for i in range(len(views)):
        s.append("%d\n%d " % (i, views.shape[1]))
        s.append("".join("%d %f " % (int(v), float(x)) for v, x in zip(views[i], scores[i])))
        s.append("\n")
    return "".join(s)


def convert(dense_folder: str, max_d: int = 256, interval_scale: float = 1, theta0: float = 5, sigma1: float = 1, sigma2: float = 10,
            test: bool = False, convert_format: bool = False, device=None) -> Dict:
    """Convert dense_folder/sparse (+ images_col) into cams/, pair.txt and images/ under dense_folder.  Returns the computed
    values: score [N, N], views / view_scores [N, min(10, N)], depth_ranges [N, 4] (min, interval, count, max), names."""
    device = device or _default_device()
    model = colmap.read_model(os.path.join(dense_folder, "sparse"))
    im = model.images
    n = len(im)
    check_sizes(n, len(im.point3D_ids))
    for cid in np.unique(im.camera_ids):
        if int(cid) not in model.cameras:
            raise ValueError("camera id %d of an image is not in cameras" % int(cid))
    Ks = {cid: colmap.intrinsic(c) for cid, c in model.cameras.items()}
    E = colmap.extrinsics(im)
    obs = Observations(model, device)
    xyz = torch.from_numpy(np.ascontiguousarray(model.points3D.xyz)).to(obs.device)
    score = score_matrix(obs, xyz, E, theta0, sigma1, sigma2)
    dmin, dmax = depth_bounds(obs, xyz, E)
    ranges = []
    for i in range(n):
        lo, hi = float(dmin[i]), float(dmax[i])
        depth_num = inverse_depth_count(Ks[int(im.camera_ids[i])], E[i], lo, hi) if max_d == 0 else max_d
        ranges.append((lo, (hi - lo) / (depth_num - 1) / interval_scale, depth_num, hi))
    views, view_scores = select_views(score)
    out = {"score": score.cpu().numpy(), "views": views, "view_scores": view_scores, "depth_ranges": np.array(ranges, np.float64),
           "names": list(im.names)}
    if test:
        for i in range(n):
            print("%08d %s  depth %f %f %f %f" % ((i, im.names[i]) + tuple(ranges[i])))
            print("    views " + " ".join("%d:%f" % (int(v), float(s)) for v, s in zip(views[i], view_scores[i])))
        return out
    cam_dir, renamed_dir, image_dir = (os.path.join(dense_folder, d) for d in ("cams", "images", "images_col"))
    os.makedirs(cam_dir, exist_ok=True)
    os.makedirs(renamed_dir, exist_ok=True)
    for i in range(n):
        with open(os.path.join(cam_dir, "%08d_cam.txt" % i), "w") as f:
            f.write(cam_text(E[i], Ks[int(im.camera_ids[i])], ranges[i]))
    with open(os.path.join(dense_folder, "pair.txt"), "w") as f:
        f.write(pair_text(views, view_scores))
    for i in range(n):
        src, dst = os.path.join(image_dir, im.names[i]), os.path.join(renamed_dir, "%08d.jpg" % i)
        if convert_format:
            from PIL import Image
            with Image.open(src) as img:
                img.convert("RGB").save(dst, "JPEG", quality=95)
        else:
            shutil.copyfile(src, dst)
    return out


def main(argv=None) -> None:
    parser = argparse.ArgumentParser(description="Convert a COLMAP model into MVSNet cameras, pair.txt and images (on the device)")
    parser.add_argument("--dense_folder", type=str, required=True, help="Project dir: sparse/ (COLMAP model) and images_col/.")
    parser.add_argument("--max_d", type=int, default=256)
    parser.add_argument("--interval_scale", type=float, default=1)
    parser.add_argument("--theta0", type=float, default=5)
    parser.add_argument("--sigma1", type=float, default=1)
    parser.add_argument("--sigma2", type=float, default=10)
    parser.add_argument("--test", action="store_true", default=False, help="If set, compute and print, do not write to file.")
    parser.add_argument("--convert_format", action="store_true", default=False, help="If set, re-encode the images as JPEG.")
    parser.add_argument("--device", type=str, default=None, help="torch device (default cuda:0)")
    a = parser.parse_args(argv)
    convert(a.dense_folder, a.max_d, a.interval_scale, a.theta0, a.sigma1, a.sigma2, a.test, a.convert_format, a.device)


if __name__ == "__main__":
    main()
