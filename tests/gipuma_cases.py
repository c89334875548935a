"""TEST HELPERS for the Gipuma route (mvsformerplusplus_amd/gipuma.py): synthetic scenes, a device run that records every launch,
and the comparison with the fp64 oracle (gipuma_ref).  Rule, restated from parity_cases.fusion_vs_fp64: where a comparison is
borderline (gipuma_ref), the pixel's decision is not checked; everywhere else the device's decision, colour and marks must equal
the oracle's exactly and its position must lie within POS_REL of it."""
import os

import numpy as np
import torch

import gipuma_ref as R
from mvsformerplusplus_amd import data_io
from mvsformerplusplus_amd.gipuma import GipumaFuser

POS_REL = 1e-5
PARAMS = dict(disp_thresh=0.2, num_consistent=3, depth_min=0.001, depth_max=100000.0)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_scene(V, H, W, seed, outliers=0.15, holes=0.05):
    """V cameras (per-view focal length and rotation) on an arc facing a slanted plane; depth maps = the plane's depth, with
    `outliers` of the pixels scaled by 0.7 / 1.3, `holes` set to 0, a few out of range; random colours.
    -> {"depth" [V,H,W] f32, "rgb" [V,H,W,3] u8, "cams" [V,2,4,4] f32}."""
    g = np.random.default_rng(seed)
    n = np.array([0.1, -0.2, 1.0])
    n /= np.linalg.norm(n)
    h0 = 6.0
    cams = np.zeros((V, 2, 4, 4), np.float32)
    depth = np.zeros((V, H, W), np.float32)
    for v in range(V):
        f = W * g.uniform(0.9, 1.3)
        K = np.array([[f, 0, W / 2 + g.uniform(-1, 1)], [0, f * g.uniform(0.98, 1.02), H / 2 + g.uniform(-1, 1)], [0, 0, 1]])
        ang = 2 * np.pi * v / max(V, 1) * 0.25
        C = np.array([0.6 * np.sin(ang) + g.uniform(-0.05, 0.05), 0.4 * np.cos(ang) - 0.2, g.uniform(-0.2, 0.2)])
        Rm = _rot(g.uniform(-0.05, 0.05), -0.08 * np.sin(ang), g.uniform(-0.1, 0.1))
        E = np.eye(4)
        E[:3, :3] = Rm
        E[:3, 3] = -Rm @ C
        cams[v, 0] = E
        cams[v, 1, :3, :3] = K
        cams[v, 1, 3, :] = [0.5, 0.01, 192, 10.0]              # the depth-range slot the cam files carry
        K32, E32 = cams[v, 1, :3, :3].astype(np.float64), cams[v, 0].astype(np.float64)
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        ray_c = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K32).T
        ray_w = ray_c @ E32[:3, :3]                            # R^T ray
        Cw = -E32[:3, :3].T @ E32[:3, 3]
        lam = (h0 - n @ Cw) / (ray_w @ n)
        depth[v] = lam.astype(np.float32)
    u = g.random((V, H, W))
    depth = np.where(u < outliers / 2, depth * np.float32(0.7), depth)
    depth = np.where((u >= outliers / 2) & (u < outliers), depth * np.float32(1.3), depth)
    depth = np.where(g.random((V, H, W)) < holes, np.float32(0), depth)
    depth = np.where(g.random((V, H, W)) < 0.005, np.float32(2e5), depth).astype(np.float32)
    rgb = g.integers(0, 256, (V, H, W, 3)).astype(np.uint8)
    return {"depth": depth, "rgb": rgb, "cams": cams}


def fuser_kwargs(params):
    return dict(disp_threshold=params["disp_thresh"], num_consistent=params["num_consistent"], depth_min=params["depth_min"],
                depth_max=params["depth_max"])


def run_device(scene, device, params, capacity=1 << 22):
    """The scene through GipumaFuser on `device` (depths taken as already filtered) -> per-view masks / points / rgb, skipped,
    final used maps, the records' xyz / rgb and per-view counts."""
    dev = torch.device(device)
    V, H, W = scene["depth"].shape
    fz = GipumaFuser(scene["cams"], H, W, dev, return_skipped=True, capacity=capacity, **fuser_kwargs(params))
    for v in range(V):
        fz.set_view(v, torch.from_numpy(scene["depth"][v]).to(dev), torch.from_numpy(scene["rgb"][v]).to(dev))
    views = []
    fz.run(on_view=lambda r, out: views.append({k: t.cpu().numpy().copy() for k, t in out.items()}))
    fin = fz.accumulator.finalize()
    return {"views": views, "skipped": fz.skipped.cpu().numpy(), "used": fz.used.cpu().numpy(), "xyz": fin["xyz"], "rgb": fin["rgb"],
            "counts": fin["counts"]}


def _pos_ok(got, want):
    err = np.linalg.norm(got.astype(np.float64) - want, axis=-1)
    return err <= POS_REL * np.maximum(np.linalg.norm(want, axis=-1), 1.0)


def check_vs_oracle(scene, dev, params, pixels_per_view=None, seed=0, check_marks=True):
    """Each view r checked in isolation against the oracle run with the device's own skipped[r]; with check_marks, skipped[r]
    must equal the marks of the non-borderline accepted pixels of views < r.  -> (borderline pixels, evaluated pixels)."""
    V, H, W = scene["depth"].shape
    cams = R.cameras(scene["cams"])
    g = np.random.default_rng(seed)
    marked = np.zeros((V, H * W), bool)
    unsure = np.zeros((V, H * W), bool)
    nb = ne = 0
    off = 0
    for r in range(V):
        out = dev["views"][r]
        mask = out["mask"].reshape(-1).astype(bool)
        pix = None if pixels_per_view is None else np.sort(g.choice(H * W, min(pixels_per_view, H * W), replace=False))
        o = R.fuse_view(r, scene["depth"], scene["rgb"], cams, dev["skipped"][r].astype(bool), params, pixels=pix)
        sk = dev["skipped"][r].reshape(-1).astype(bool)
        if check_marks:
            ok = ~unsure[r]
            assert np.array_equal(sk[ok], marked[r][ok]), ("skipped[%d] differs from the marks of views < %d at %d pixels" %
                                                           (r, r, int((sk[ok] != marked[r][ok]).sum())))
        sure = ~o["border"]
        nb += int(o["border"].sum())
        ne += int(len(o["pix"]))
        dm = mask[o["pix"]]
        bad = sure & (dm != o["accepted"])
        assert not bad.any(), "view %d: %d decided pixels differ from fp64 (first flat %d)" % (r, int(bad.sum()), int(o["pix"][bad][0]))
        # the view's records: its kept pixels in row-major order
        cnt = int(dev["counts"][r])
        assert cnt == int(mask.sum())
        kept = np.flatnonzero(mask)
        xyz, rgb = dev["xyz"][off:off + cnt], dev["rgb"][off:off + cnt]
        off += cnt
        pts = out["points"].reshape(3, -1)[:, kept].T
        assert xyz.tobytes() == pts.astype(np.float32).tobytes() and np.array_equal(rgb, out["rgb"].reshape(-1, 3)[kept])
        acc = sure & o["accepted"]
        rank = np.searchsorted(kept, o["pix"][acc])
        assert _pos_ok(xyz[rank], o["pos"][acc]).all(), "view %d: positions beyond %g of fp64" % (r, POS_REL)
        assert np.array_equal(rgb[rank].astype(np.int64), o["rgb"][acc]), "view %d: colours differ" % r
        if check_marks:
            for c, _, flat in o["marks"]:
                if c > r:
                    marked[c][flat] = True
            for c, flat in o["marks_border"]:
                if c > r:
                    unsure[c][flat] = True
    assert off == dev["xyz"].shape[0]
    return nb, ne


def check_exact_scene(scene, dev, params):
    """A scene with no borderline comparison: the oracle's own run (its own used maps) equals the device's: accepted sets,
    records in order (positions within POS_REL, colours exact), skipped and final used maps."""
    outs, used = R.fuse_scene(scene["depth"], scene["rgb"], R.cameras(scene["cams"]), params)
    assert sum(int(o["border"].sum()) for o in outs) == 0, "the scene has borderline comparisons"
    pos = np.concatenate([o["pos"][o["accepted"]] for o in outs])
    rgb = np.concatenate([o["rgb"][o["accepted"]] for o in outs])
    for r, o in enumerate(outs):
        assert np.array_equal(dev["views"][r]["mask"].reshape(-1).astype(bool), o["accepted"]), "view %d accepted set" % r
        assert np.array_equal(dev["skipped"][r].astype(bool), o["skipped"]), "view %d skipped" % r
    assert dev["counts"].tolist() == [int(o["accepted"].sum()) for o in outs]
    assert np.array_equal(dev["used"].astype(bool), used)
    assert dev["xyz"].shape[0] == pos.shape[0] and _pos_ok(dev["xyz"], pos).all()
    assert np.array_equal(dev["rgb"].astype(np.int64), rgb)
    return sum(int(o["accepted"].sum()) for o in outs)


def write_scene_folder(root, scene, conf=None, names=None):
    """depth_est/*.pfm, confidence/*.npy (uint8 255 unless given), cams/*_cam.txt, images/*.png-bytes-as-.jpg."""
    from PIL import Image
    V = scene["depth"].shape[0]
    names = names or ["%08d" % v for v in range(V)]
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for v, nm in enumerate(names):
        data_io.save_pfm(os.path.join(root, "depth_est", nm + ".pfm"), scene["depth"][v])
        np.save(os.path.join(root, "confidence", nm + ".npy"), conf[v] if conf is not None else np.full(scene["depth"][v].shape, 255, np.uint8))
        data_io.write_cam(os.path.join(root, "cams", nm + "_cam.txt"), scene["cams"][v])
        Image.fromarray(scene["rgb"][v]).save(os.path.join(root, "images", nm + ".jpg"), format="PNG")
    return names
