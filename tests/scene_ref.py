"""References for the scene tests (tests/test_scene.py, tests/test_scene_gpu.py), numpy only and independent of the package:

  * the dataset arithmetic of datasets/general_eval.py MVSDataset (mode="test") restated line by line: pair list, camera files, intrinsics
    scaling, per-stage projection matrices, depth values;
  * the 8-bit linear resize as integer numpy (the arithmetic the issue states, which is OpenCV's fixed-point INTER_LINEAR path), the "tt"
    edge pad, ToTensor + Normalize, and an fp64 bilinear resize at half-pixel centres with clamped edges;
  * a writer of small synthetic scenes (JPEGs through PIL, camera files, pair.txt).
"""
import os
import warnings

import numpy as np
from PIL import Image

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- the dataset ----------------------------------------------------------------------------------------------------------------------
def _floats(text):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return np.fromstring(text, dtype=np.float32, sep=" ")             # what the reference calls


def build_list(scan_folder, nviews):
    metas = []
    with open(os.path.join(scan_folder, "pair.txt")) as f:
        num_viewpoint = int(f.readline())
        for view_idx in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if len(src_views) > 0:
                if len(src_views) < nviews:
                    src_views += [src_views[0]] * (nviews - len(src_views))
                src_views = src_views[:(nviews - 1)]
                metas.append((ref_view, src_views))
    return metas


def read_cam_file(filename, interval_scale, ndepths, dataset):
    with open(filename) as f:
        lines = f.readlines()
        lines = [line.rstrip() for line in lines]
    extrinsics = _floats(" ".join(lines[1:5])).reshape((4, 4))
    intrinsics = _floats(" ".join(lines[7:10])).reshape((3, 3))
    if dataset == "tt":
        intrinsics[1, 2] += 4
    intrinsics[:2, :] /= 4.0
    depth_min = float(lines[11].split()[0])
    if "cams_1" in filename:
        depth_interval = 2.5
    else:
        depth_interval = float(lines[11].split()[1])
    if len(lines[11].split()) >= 3:
        num_depth = lines[11].split()[2]
        depth_max = depth_min + int(float(num_depth)) * depth_interval
        depth_interval = (depth_max - depth_min) / ndepths
    if dataset == "eth3d":
        depth_max = float(lines[11].split()[1])
        depth_interval = (depth_max - depth_min) / ndepths
    depth_interval *= interval_scale
    return intrinsics, extrinsics, depth_min, depth_interval


def read_img(filename, dataset):
    np_img = np.asarray(Image.open(filename).convert("RGB"))
    if dataset == "tt":
        np_img = np.pad(np_img, ((4, 4), (0, 0), (0, 0)), "edge")
    return np.array(np_img)


def samples(testpath, scan, nviews, ndepths, interval_scale, max_h, max_w, dataset, use_short_range=False, with_images=False):
    """MVSDataset.__getitem__ for every index: [{"view_ids", "proj_matrices" {stage: [V,2,4,4]}, "depth_values" [D], "imgs" [V,3,H,W]}]."""
    out = []
    scan_folder = os.path.join(testpath, scan)
    for ref_view, src_views in build_list(scan_folder, nviews):
        view_ids = [ref_view] + src_views
        imgs, proj_matrices, depth_values = [], [], None
        for i, vid in enumerate(view_ids):
            img_filename = os.path.join(testpath, "{}/images/{:0>8}.jpg".format(scan, vid))
            if dataset == "tt":
                if use_short_range:
                    cam = os.path.join(testpath, "short_range_cameras/cams_{}/{:0>8}_cam.txt".format(scan.lower(), vid))
                else:
                    cam = os.path.join(testpath, "{}/cams/{:0>8}_cam.txt".format(scan, vid))
            else:
                cam = os.path.join(testpath, "{}/cams_1/{:0>8}_cam.txt".format(scan, vid))
                if not os.path.exists(cam):
                    cam = os.path.join(testpath, "{}/cams/{:0>8}_cam.txt".format(scan, vid))
            img = read_img(img_filename, dataset)
            intrinsics, extrinsics, depth_min, depth_interval = read_cam_file(cam, interval_scale, ndepths, dataset)
            h, w = img.shape[:2]
            scale_w = 1.0 * max_w / w
            scale_h = 1.0 * max_h / h
            intrinsics[0, :] *= scale_w
            intrinsics[1, :] *= scale_h
            if with_images:
                imgs.append(normalise(resize_u8(img, max_h, max_w)))
            proj_mat = np.zeros(shape=(2, 4, 4), dtype=np.float32)
            proj_mat[0, :4, :4] = extrinsics
            proj_mat[1, :3, :3] = intrinsics
            proj_matrices.append(proj_mat)
            if i == 0:
                depth_values = np.arange(depth_min, depth_interval * (ndepths - 0.5) + depth_min, depth_interval, dtype=np.float32)
        proj_matrices = np.stack(proj_matrices)
        stage0 = proj_matrices.copy()
        stage0[:, 1, :2, :] = proj_matrices[:, 1, :2, :] * 0.5
        stage1 = proj_matrices.copy()
        stage2 = proj_matrices.copy()
        stage2[:, 1, :2, :] = proj_matrices[:, 1, :2, :] * 2
        stage3 = proj_matrices.copy()
        stage3[:, 1, :2, :] = proj_matrices[:, 1, :2, :] * 4
        out.append({"view_ids": view_ids, "proj_matrices": {"stage1": stage0, "stage2": stage1, "stage3": stage2, "stage4": stage3},
                    "depth_values": depth_values, "imgs": np.stack(imgs) if with_images else None})
    return out


# ---- the image path -------------------------------------------------------------------------------------------------------------------
def _taps(out, size):
    """Per output index of one axis: tap index s and the coefficients (a0, a1), int64."""
    d = np.arange(out, dtype=np.float64)
    f = ((d + 0.5) * (size / out) - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s.astype(np.float32)).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= size - 1
    s = np.where(low, 0, np.where(high, size - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int16).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int16).astype(np.int64)
    return s, a0, a1


def resize_u8(img, H, W):
    """uint8 [h, w, 3] -> uint8 [H, W, 3]: the 8-bit linear resize in integers (the kernel's contract)."""
    h, w = img.shape[:2]
    S = img.astype(np.int64)
    sx, a0, a1 = _taps(W, w)
    sy, b0, b1 = _taps(H, h)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    rows = S[:, sx] * a0[None, :, None] + S[:, sx1] * a1[None, :, None]                     # [h, W, 3]
    r0, r1 = rows[sy], rows[sy1]
    v = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def pad_tt(img, rows=4):
    return np.pad(img, ((rows, rows), (0, 0), (0, 0)), "edge")


def bilinear_f64(img, H, W):
    """fp64 bilinear at half-pixel centres, edges clamped -> float64 [H, W, 3] (not rounded)."""
    h, w = img.shape[:2]
    S = img.astype(np.float64)

    def axis(out, size):
        c = np.clip((np.arange(out) + 0.5) * (size / out) - 0.5, 0, size - 1)
        i0 = np.minimum(np.floor(c).astype(np.int64), size - 1)
        return i0, np.minimum(i0 + 1, size - 1), c - i0

    x0, x1, fx = axis(W, w)
    y0, y1, fy = axis(H, h)
    rows = S[:, x0] * (1 - fx)[None, :, None] + S[:, x1] * fx[None, :, None]
    return rows[y0] * (1 - fy)[:, None, None] + rows[y1] * fy[:, None, None]


def table():
    """ToTensor + Normalize of every byte value as torch evaluates them, fp32 [3, 256] (a torch tensor)."""
    import torch
    u = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1)
    return (u[None].repeat(3, 1).sub_(mean).div_(std)).contiguous()


def normalise(img_u8):
    """uint8 [H, W, 3] -> fp32 [3, H, W]: torchvision's ToTensor (permute, float, div 255) and Normalize (sub_ mean, div_ std) in torch."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    return t.sub_(mean).div_(std).numpy()


# ---- synthetic scenes -----------------------------------------------------------------------------------------------------------------
def write_cam(path, extrinsic, intrinsic, line11):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("extrinsic\n")
        for row in extrinsic:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
        f.write("\nintrinsic\n")
        for row in intrinsic:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
        f.write("\n" + line11 + "\n")


def smooth_image(rng, h, w):
    """A seeded image with structure at several scales (a JPEG of white noise says little about a resize)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph = rng.uniform(0.02, 0.5), rng.uniform(0.02, 0.5), rng.uniform(0, 6.28)
            img[..., c] += rng.uniform(20, 60) * np.sin(fx * xx + fy * yy + ph)
    img += 128 + rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def write_scene(testpath, scan, n_views, h, w, pairs, seed=0, line11=None, cams_1=(), baseline=30.0, focal=None, short_range=False):
    """images/%08d.jpg (seeded, PIL), cams/%08d_cam.txt, pair.txt.  pairs: [(ref, [src, ...])] written with scores.  line11: per view the
    depth line (default "425.0 2.5"); cams_1: view ids that also get a cams_1/ file with another interval."""
    rng = np.random.default_rng(seed)
    folder = os.path.join(testpath, scan)
    os.makedirs(os.path.join(folder, "images"), exist_ok=True)
    focal = focal or 4.0 * 1.2 * w
    for v in range(n_views):
        Image.fromarray(smooth_image(rng, h, w)).save(os.path.join(folder, "images", "{:0>8}.jpg".format(v)), quality=92)
        E = np.eye(4)
        ang = 0.02 * (v - n_views / 2)
        E[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        E[:3, 3] = [-baseline * (v - n_views / 2) + rng.normal(), rng.normal(), rng.normal()]
        K = np.array([[focal + rng.normal(), 0, 2.0 * w + rng.normal()], [0, focal + rng.normal(), 2.0 * h + rng.normal()], [0, 0, 1]])
        l11 = (line11 or {}).get(v, "425.0 2.5")
        write_cam(os.path.join(folder, "cams", "{:0>8}_cam.txt".format(v)), E, K, l11)
        if v in cams_1:
            write_cam(os.path.join(folder, "cams_1", "{:0>8}_cam.txt".format(v)), E, K * [[1.01], [1.02], [1]], "430.5 1.7")
        if short_range:
            write_cam(os.path.join(testpath, "short_range_cameras", "cams_" + scan.lower(), "{:0>8}_cam.txt".format(v)), E, K * [[0.99], [0.98], [1]],
                      "0.4 0.01")
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for ref, srcs in pairs:
            f.write("%d\n" % ref)
            f.write(" ".join(["%d" % len(srcs)] + ["%d %.3f" % (s, 100.0 - k) for k, s in enumerate(srcs)]) + "\n")
    return folder
