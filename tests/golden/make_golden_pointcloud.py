#!/usr/bin/env python3
"""Generate fixture F22 (tests/golden/f22_point_cloud.npz) by IMPORTING the reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointcloud.py

A small scene (6 reference views at 48x64 plus a listed view without a camera) and the point clouds the reference's
``filter_depth`` ("pcd") and ``dynamic_filter_depth`` ("dpcd") make of it under both conventions, test.py ("dtu") and
test_tt.py ("tt").  test.py / test_tt.py cannot be imported (they parse arguments at module level and import cv2 and plyfile),
so their loop bodies are restated below around the reference's own ``misc/fusion.py`` and ``datasets/data_io.read_pfm``; like
f10_fusion in make_golden.py, ``.cuda()`` is patched to a no-op for the duration (the arithmetic is untouched).

What is committed is DATA: the scene's files (depth maps, uint8 confidences, camera and pair texts, images as PNG bytes under
the .jpg names - PIL decodes by content, so the pixels do not depend on a libjpeg version) and, per case, the reference's
final masks and vertex arrays plus the (view, pixel) of every vertex.
"""
import io
import os
import sys
import tempfile

import numpy as np

REF = os.environ.get("MVS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.dont_write_bytecode = True

import torch  # noqa: E402
from PIL import Image  # noqa: E402

import importlib.util  # noqa: E402

# datasets/__init__.py pulls in the training loaders (torchvision); load datasets/data_io.py on its own
_spec = importlib.util.spec_from_file_location("ref_data_io", os.path.join(REF, "datasets", "data_io.py"))
_ref_data_io = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ref_data_io)
read_pfm = _ref_data_io.read_pfm

from mvsformerplusplus_amd import data_io as P  # noqa: E402
from mvsformerplusplus_amd import synth  # noqa: E402

H, W, NV = 48, 64, 6
MISSING = 7                 # listed as a source, has no camera file
CONF, THRES_VIEW, THRES_DISP, DIST_BASE, REL_DIFF_BASE = 0.5, 2, 1.0, 4.0, 1300.0
FUSION_VIEW = 5             # test_tt.py --fusion_view


def scene(seed=22):
    """Depth maps of a tilted plane with a bump seen from 6 cameras (closed form), noise, outliers, holes; uint8 confidences with
    a low-confidence band; smooth RGB images."""
    g = torch.Generator().manual_seed(seed)
    cams = synth.make_cameras(NV, H, W, baseline=30.0, rot_deg=0.0, seed=seed)[0]
    a, b, z0 = 0.15, -0.1, 600.0
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5, torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
    depths = []
    for v in range(NV):
        K, E = cams[v, 1, :3, :3], cams[v, 0]
        C = -E[:3, 3]
        rx, ry = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
        depths.append((z0 + a * C[0] + b * C[1] - C[2]) / (1 - a * rx - b * ry))
    d = torch.stack(depths)
    d = d * (1 + 0.0008 * torch.randn(d.shape, generator=g))
    out = torch.rand(d.shape, generator=g) < 0.05
    d = torch.where(out, d * (1 + 0.05 * torch.randn(d.shape, generator=g)), d)
    d[:, :, :3] = 0.0
    d[2, 30:36, 20:40] = 0.0
    conf = (torch.rand(d.shape, generator=g) * 0.5 + 0.5)
    conf[:, 10:18, :] *= 0.6                                  # a low-confidence band around the threshold
    conf[3, :, 50:] = 0.2
    conf_u8 = (conf.numpy() * 255).astype(np.uint8)           # test.py:284-286
    imgs = []
    for v in range(NV):
        r = (np.arange(W)[None, :] * 4 + v * 20) % 256
        gch = (np.arange(H)[:, None] * 5 + v * 30) % 256
        im = np.stack([np.broadcast_to(r, (H, W)), np.broadcast_to(gch, (H, W)), np.full((H, W), 40 * v)], -1).astype(np.uint8)
        im[::7, ::5] = 255 - im[::7, ::5]
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="PNG")
        imgs.append(np.frombuffer(buf.getvalue(), dtype=np.uint8))
    return d.numpy().astype(np.float32), conf_u8, cams.numpy(), imgs


def pair_texts():
    """dtu pair.txt: every view lists the 5 others (+ the camera-less view); one line without sources (dropped).
    tt new_pair.txt: shorter lists (padded with the first source up to FUSION_VIEW)."""
    dtu = ["%d" % (NV + 1)]
    tt = ["%d" % (NV + 1)]
    for v in range(NV):
        srcs = [s for s in range(NV) if s != v][::-1 if v % 2 else 1]
        if v == 1:
            srcs = srcs[:2] + [MISSING] + srcs[2:]
        dtu += ["%d" % v, "%d " % len(srcs) + " ".join("%d %.1f" % (s, 100.0 - i) for i, s in enumerate(srcs))]
        short = srcs[:2 + v % 3]
        tt += ["%d" % v, "%d " % len(short) + " ".join("%d %.1f" % (s, 50.0 - i) for i, s in enumerate(short))]
    dtu += ["%d" % MISSING, "0"]
    tt += ["%d" % MISSING, "0 "]
    return "\n".join(dtu) + "\n", "\n".join(tt) + "\n"


# ---- restated from test.py / test_tt.py (read_camera_parameters :102-112, read_pair_file :136-146 / tt :142-156, TTDataset) ----
def read_camera_parameters(filename):
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.fromstring(" ".join(lines[1:5]), dtype=np.float32, sep=" ").reshape((4, 4))
    intrinsics = np.fromstring(" ".join(lines[7:10]), dtype=np.float32, sep=" ").reshape((3, 3))
    return intrinsics, extrinsics


def read_img(filename):
    return np.array(Image.open(filename), dtype=np.float32) / 255.


def read_pair_file(filename, nviews=None):
    data = []
    with open(filename) as f:
        num_viewpoint = int(f.readline())
        for _ in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if len(src_views) > 0:
                if nviews is not None:
                    if len(src_views) < nviews:
                        src_views += [src_views[0]] * (nviews - len(src_views))
                    src_views = src_views[:(nviews - 1)]
                data.append((ref_view, src_views))
    return data


def load_sample(scan, id_ref, id_srcs, tt):
    def cam(i):
        K, E = read_camera_parameters(os.path.join(scan, "cams/{:0>8}_cam.txt".format(i)))
        c = np.zeros((2, 4, 4), dtype=np.float32)
        c[0] = E
        c[1, :3, :3] = K
        c[1, 3, 3] = 1.0
        return c
    ref_img = read_img(os.path.join(scan, "images/{:0>8}.jpg".format(id_ref))).transpose([2, 0, 1])
    ref_depth = np.array(read_pfm(os.path.join(scan, "depth_est/{:0>8}.pfm".format(id_ref)))[0], dtype=np.float32)
    confidence = np.load(os.path.join(scan, "confidence/{:0>8}.npy".format(id_ref)))
    if confidence.dtype == np.uint8:
        confidence = confidence / 255
    sd, sc, scam = [], [], []
    for i in id_srcs:
        if not os.path.exists(os.path.join(scan, "cams/{:0>8}_cam.txt".format(i))):
            continue
        scam.append(cam(i))
        sd.append(np.array(read_pfm(os.path.join(scan, "depth_est/{:0>8}.pfm".format(i)))[0], dtype=np.float32))
        c = np.load(os.path.join(scan, "confidence/{:0>8}.npy".format(i)))
        if tt and c.dtype == np.uint8:
            c = c / 255
        sc.append(c)
    # DataLoader(batch_size=1) collation: a leading batch dimension, numpy -> torch with the same dtypes
    t = lambda x: torch.from_numpy(np.asarray(x))[None]
    return {"ref_depth": t(ref_depth[None]), "ref_cam": t(cam(id_ref)), "ref_conf": t(confidence),
            "src_depths": t(np.expand_dims(np.stack(sd), 1)), "src_cams": t(np.stack(scam)), "src_confs": t(np.stack(sc)),
            "ref_img": ref_img[None], "ref_id": id_ref}


def run_driver(scan, method, tt):
    from misc import fusion
    pairs = read_pair_file(os.path.join(scan, "new_pair.txt" if tt else "pair.txt"), FUSION_VIEW if tt else None)
    n_src = FUSION_VIEW if tt else 10
    views = {}
    for id_ref, id_srcs in pairs:
        sample = load_sample(scan, id_ref, id_srcs[:n_src], tt)
        if method == "pcd":                                                                          # test.py:393-409
            for ids in range(sample["src_depths"].size(1)):
                src_prob_mask = sample["src_confs"][:, ids] > CONF
                sample["src_depths"][:, ids, ...] *= src_prob_mask.float()
            prob_mask = sample["ref_conf"] > CONF
            reproj_xyd, in_range = fusion.get_reproj(*[sample[k] for k in ["ref_depth", "src_depths", "ref_cam", "src_cams"]])
            vis_masks, vis_mask = fusion.vis_filter(sample["ref_depth"], reproj_xyd, in_range, THRES_DISP, 0.01, THRES_VIEW)
            ave = fusion.ave_fusion(sample["ref_depth"], reproj_xyd, vis_masks)
            mask = fusion.bin_op_reduce([prob_mask, vis_mask], torch.min)
        else:                                                                                        # test.py:455-483
            dy_range = sample["src_depths"].shape[1] + 1
            prob_mask = sample["ref_conf"] > CONF
            ref_depth = sample["ref_depth"]
            reproj_xyd = fusion.get_reproj_dynamic(*[sample[k] for k in ["ref_depth", "src_depths", "ref_cam", "src_cams"]])
            vis_masks, vis_mask = fusion.vis_filter_dynamic(sample["ref_depth"], reproj_xyd, dist_base=DIST_BASE, rel_diff_base=REL_DIFF_BASE)
            reproj_depth = reproj_xyd[:, :, -1]
            reproj_depth[~vis_mask.squeeze(2)] = 0
            geo_mask_sums = vis_masks.sum(dim=1)
            geo_mask_sum = vis_mask.sum(dim=1)
            ave = (torch.sum(reproj_depth, dim=1, keepdim=True) + ref_depth) / (geo_mask_sum + 1)
            geo_mask = geo_mask_sum >= dy_range
            for i in range(2, dy_range):
                geo_mask = torch.logical_or(geo_mask, geo_mask_sums[:, i - 2] >= i)
            mask = fusion.bin_op_reduce([prob_mask, geo_mask], torch.min)
        idx_img = fusion.get_pixel_grids(*ave.size()[-2:]).unsqueeze(0)
        points = fusion.idx_cam2world(fusion.idx_img2cam(idx_img, ave, sample["ref_cam"]), sample["ref_cam"])[..., :3, 0].permute(0, 3, 1, 2)
        points_np = points.cpu().data.numpy()
        mask_np = mask.cpu().data.numpy().astype(bool)
        ref_img = sample["ref_img"]
        p_f = np.stack([points_np[0, k][mask_np[0, 0]] for k in range(3)], -1)                      # test.py:419-424
        c_f = np.stack([ref_img[0, k][mask_np[0, 0]] for k in range(3)], -1) * 255
        views[str(id_ref)] = (p_f, c_f.astype(np.uint8), mask_np[0, 0], np.flatnonzero(mask_np[0, 0]))
    ids = list(views)
    p_all, c_all = [np.concatenate([views[k][j] for k in ids], axis=0) for j in range(2)]            # test.py:429
    vertexs = np.array([tuple(v) for v in p_all], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])    # test.py:431-432
    vertex_colors = np.array([tuple(v) for v in c_all], dtype=[("red", "u1"), ("green", "u1"), ("blue", "u1")])
    xyz = np.stack([vertexs[k] for k in "xyz"], -1)
    rgb = np.stack([vertex_colors[k] for k in ("red", "green", "blue")], -1)
    vid = np.concatenate([np.full(len(views[k][3]), int(k), np.int32) for k in ids])
    pix = np.concatenate([views[k][3] for k in ids]).astype(np.int32)
    masks = np.stack([views[k][2] for k in ids])
    return {"views": np.array([int(k) for k in ids], np.int32), "masks": masks, "xyz": xyz, "rgb": rgb, "vid": vid, "pix": pix}


def main():
    depth, conf, cams, imgs = scene()
    pair_dtu, pair_tt = pair_texts()
    out = {"depth": depth, "conf": conf, "conf_thresh": np.float32(CONF), "thres_view": np.int32(THRES_VIEW),
           "thres_disp": np.float32(THRES_DISP), "dist_base": np.float32(DIST_BASE), "rel_diff_base": np.float32(REL_DIFF_BASE),
           "fusion_view": np.int32(FUSION_VIEW), "pair_dtu": np.array(pair_dtu), "pair_tt": np.array(pair_tt)}
    for v in range(NV):
        out["img%d" % v] = imgs[v]
    orig = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with tempfile.TemporaryDirectory() as scan:
            for sub in ("depth_est", "confidence", "cams", "images"):
                os.makedirs(os.path.join(scan, sub))
            for v in range(NV):
                P.save_pfm(os.path.join(scan, "depth_est", "%08d.pfm" % v), depth[v])
                np.save(os.path.join(scan, "confidence", "%08d.npy" % v), conf[v])
                P.write_cam(os.path.join(scan, "cams", "%08d_cam.txt" % v), cams[v])
                with open(os.path.join(scan, "cams", "%08d_cam.txt" % v)) as f:
                    out["cam%d" % v] = np.array(f.read())
                with open(os.path.join(scan, "images", "%08d.jpg" % v), "wb") as f:
                    f.write(imgs[v].tobytes())
            with open(os.path.join(scan, "pair.txt"), "w") as f:
                f.write(pair_dtu)
            with open(os.path.join(scan, "new_pair.txt"), "w") as f:
                f.write(pair_tt)
            for method in ("pcd", "dpcd"):
                for conv in ("dtu", "tt"):
                    r = run_driver(scan, method, conv == "tt")
                    print("  %-4s %-3s vertices %6d  kept %s" % (method, conv, len(r["xyz"]), [int(m.sum()) for m in r["masks"]]))
                    for k, a in r.items():
                        out["%s_%s_%s" % (method, conv, k)] = a
    finally:
        torch.Tensor.cuda = orig
    path = os.path.join(HERE, "f22_point_cloud.npz")
    np.savez_compressed(path, **out)
    print("f22_point_cloud.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
