"""CPU: the Gipuma route (mvsformerplusplus_amd/gipuma.py, csrc/gipuma_kernels.hip on the host emulator) - fixture F23's file
formats (tests/golden/make_golden_gipuma.py, generated from the reference's misc/gipuma.py), the fusion against the fp64 oracle
(tests/gipuma_ref.py) on small scenes with no borderline comparison, the contract's edge cases, and the scene driver / CLI."""
import os

import numpy as np
import pytest
import torch

import gipuma_cases as GC
import gipuma_ref as R
from mvsformerplusplus_amd import data_io, gipuma as G

from conftest import GOLDEN

# (views, height, width, num_consistent, seed): scenes whose fp64 run has no borderline comparison (asserted)
EXACT_SCENES = [(2, 24, 32, 1, 10), (3, 20, 26, 2, 12), (4, 24, 32, 3, 23), (5, 15, 21, 3, 23), (7, 5, 7, 2, 11), (8, 13, 19, 3, 34),
                (10, 7, 5, 2, 11), (12, 9, 11, 3, 13), (6, 11, 13, 1, 14)]


def load_f23():
    return dict(np.load(os.path.join(GOLDEN, "f23_gipuma_formats.npz")))


def materialise_f23(fx, root):
    for k, v in fx.items():
        if k.startswith("in/"):
            p = os.path.join(root, k[3:])
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(v.tobytes())


def test_f23_export_bytes(tmp_path):
    """probability filter + mvsnet_to_gipuma: every file byte-equal to the reference's (.P, .dmb, _prob_filtered.pfm, images)."""
    fx = load_f23()
    materialise_f23(fx, str(tmp_path))
    names = data_io.export_gipuma_folder(str(tmp_path), str(tmp_path / "points_mvsnet"), float(fx["prob_threshold"]), write_filtered=True)
    assert names == ["%08d.jpg" % v for v in range(4)]
    outs = [k for k in fx if k.startswith("out/")]
    assert len(outs) == 4 + 4 + 4 + 8
    for k in outs:
        got = open(os.path.join(str(tmp_path), k[4:]), "rb").read()
        assert got == fx[k].tobytes(), k


def test_f23_export_without_filtered_maps(tmp_path):
    fx = load_f23()
    materialise_f23(fx, str(tmp_path))
    data_io.export_gipuma_folder(str(tmp_path), str(tmp_path / "p"), float(fx["prob_threshold"]))
    assert not any(f.endswith("_prob_filtered.pfm") for f in os.listdir(tmp_path / "depth_est"))
    assert open(tmp_path / "p" / "2333__00000002" / "disp.dmb", "rb").read() == fx["out/points_mvsnet/2333__00000002/disp.dmb"].tobytes()


def test_dmb_roundtrip(tmp_path):
    g = np.random.default_rng(0)
    for shape in ((7, 5), (6, 9, 3)):
        a = g.standard_normal(shape).astype(np.float32)
        p = str(tmp_path / "a.dmb")
        data_io.write_gipuma_dmb(p, a)
        raw = open(p, "rb").read()
        assert np.frombuffer(raw[:16], "<i4").tolist() == [1, shape[0], shape[1], shape[2] if len(shape) == 3 else 1]
        b = data_io.read_gipuma_dmb(p)
        assert b.shape == shape and b.tobytes() == a.tobytes()
    fx = load_f23()
    p = str(tmp_path / "n.dmb")
    open(p, "wb").write(fx["out/points_mvsnet/2333__00000001/normals.dmb"].tobytes())
    nm = data_io.read_gipuma_dmb(p)
    assert nm.shape == (24, 32, 3) and set(np.unique(nm).tolist()) <= {0.0, float(np.float32(1 / 1.732050808))}


@pytest.mark.parametrize("V,H,W,nc,seed", EXACT_SCENES)
def test_exact_scene(emu, V, H, W, nc, seed):
    """No borderline comparison: accepted sets, skipped / used maps and records (in order) equal the oracle's own run."""
    sc = GC.make_scene(V, H, W, seed)
    params = dict(GC.PARAMS, num_consistent=nc)
    dev = GC.run_device(sc, emu, params)
    assert GC.check_exact_scene(sc, dev, params) > 0
    assert GC.check_vs_oracle(sc, dev, params) == (0, V * H * W)


def test_borderline_scene_per_view(emu):
    """A scene with borderline comparisons: each view checked in isolation through the device's skipped[r], and skipped[r]
    against the marks of the decided pixels of earlier views."""
    sc = GC.make_scene(12, 17, 23, 4)
    dev = GC.run_device(sc, emu, GC.PARAMS)
    nb, ne = GC.check_vs_oracle(sc, dev, GC.PARAMS)
    assert 0 < nb <= 0.01 * ne


# ---------------------------------------------------------------- edge cases on scenes with exact arithmetic
def _cams(views):
    """views: [(f, (cx, cy, cz))]: K = diag(f, f, 1), E = [I | -C]."""
    cams = np.zeros((len(views), 2, 4, 4), np.float32)
    for i, (f, C) in enumerate(views):
        cams[i, 0] = np.eye(4)
        cams[i, 0, :3, 3] = -np.asarray(C, np.float32)
        cams[i, 1, :3, :3] = np.diag([f, f, 1.0])
        cams[i, 1, 3, 3] = 1.0
    return cams


def _scene(depths, cams, H=4, W=8):
    V = len(depths)
    d = np.stack([np.broadcast_to(np.asarray(x, np.float32), (H, W)) for x in depths]).astype(np.float32)
    rgb = np.zeros((V, H, W, 3), np.uint8)
    rgb[..., 0] = np.arange(W, dtype=np.uint8) * 10 + np.arange(V, dtype=np.uint8)[:, None, None]
    rgb[..., 1] = np.arange(H, dtype=np.uint8)[:, None] * 40 + 1
    rgb[..., 2] = 200 + np.arange(V, dtype=np.uint8)[:, None, None]
    return {"depth": np.ascontiguousarray(d), "rgb": rgb, "cams": cams}


def _p(**kw):
    return dict(GC.PARAMS, **kw)


def _shift_scene():
    """4 views at depth 2, centres (0.25, -0.25) apart in x / y: view c sees reference pixel (x, y) at (x, y) + (C_r - C_c) / 2,
    an odd multiple of 1/8 pixel off the grid in both directions - every floor and bound is decisive."""
    return _scene([2, 2, 2, 2], _cams([(1, (0.25 * c, -0.25 * c, 0)) for c in range(4)]))


@pytest.mark.parametrize("nc,emits", [(3, True), (2.5, True), (3.5, False), (4, False)])
def test_num_consistent_edge(emu, nc, emits):
    """Pixel (x = 7) of view 0 sees all three other views: n = 3 against num_consistent = n (or n - 0.5) and n + 1."""
    sc = _shift_scene()
    dev = GC.run_device(sc, emu, _p(num_consistent=nc))
    assert bool(dev["views"][0]["mask"][0, 7]) == emits
    if emits:
        GC.check_exact_scene(sc, dev, _p(num_consistent=nc))


def test_shift_scene_values(emu):
    """Hand-derived vertex of view 0, pixel (7, 0)."""
    sc = _shift_scene()
    dev = GC.run_device(sc, emu, _p(num_consistent=3))
    # u = 7 - 0.125 c for c = 1..3: colour and depth read at the rounded texel 7, back-projected at the truncated pixel 6
    m = dev["views"][0]["mask"]
    assert m[0, 7] == 1 and dev["views"][0]["rgb"][0, 7].tolist() == [(70 + 71 + 72 + 73) // 4, 1, (200 + 201 + 202 + 203) // 4]
    p = dev["views"][0]["points"][:, 0, 7]
    # X = (14, 0, 2); X_c = back-projection of (6, 0) at depth 2 from C_c = (0.25 c, -0.25 c, 0): (12 + 0.25 c, -0.25 c, 2);
    # the sum over (n + 1)
    assert p.tolist() == [(14 + 12.25 + 12.5 + 12.75) / 4, -1.5 / 4, 2]
    assert dev["used"][1:, 0, 6].all()


@pytest.mark.parametrize("thr,consistent", [(0.25, False), (float(np.nextafter(np.float32(0.25), np.float32(1))), True)])
def test_disparity_at_threshold(emu, thr, consistent):
    """f b = 1, z = 2, d_c = 4: |f b / z - f b / d_c| = 0.25 exactly; the test is strict."""
    sc = _scene([2, 4], _cams([(1, (0, 0, 0)), (1, (1, 0, 0))]))
    dev = GC.run_device(sc, emu, _p(disp_thresh=thr, num_consistent=1))
    assert (dev["counts"][0] > 0) == consistent
    assert (dev["counts"][1] > 0) == consistent


def test_clamped_texel(emu):
    """u = W - 0.5 rounds to texel W, clamped to W - 1; the colour shows which texel was read."""
    sc = _scene([2, 2], _cams([(1, (0, 0, 0)), (1, (-1, 0, 0))]))          # u = x + 0.5
    dev = GC.run_device(sc, emu, _p(num_consistent=1))
    m, rgb = dev["views"][0]["mask"], dev["views"][0]["rgb"]
    assert m[:, 7].all()
    assert rgb[0, 7, 0] == (70 + 71) // 2                                     # texel 7 of view 1 (colour 71), not 8
    assert rgb[0, 3, 0] == (30 + 41) // 2                                     # texel 4 of view 1
    assert dev["used"][1][:, 7].all()


def test_z_not_positive(emu):
    """View 1 sees view 0's pixels behind itself (z = -100) at in-image coordinates with a small disparity: rejected."""
    cams = _cams([(0.01, (0, 0, 0)), (1, (500, 300, 102))])
    sc = _scene([2, 1000], cams)
    dev = GC.run_device(sc, emu, _p(num_consistent=1))
    assert dev["counts"].tolist() == [0, 0]
    assert not dev["used"].any()


def test_marked_reference_pixel(emu):
    """Pixels of view 1 marked by view 0's vertices are skipped by view 1's launch (and reported in skipped[1])."""
    sc = _shift_scene()
    params = _p(num_consistent=1)
    dev = GC.run_device(sc, emu, params)
    assert dev["skipped"][1].any() and not dev["skipped"][0].any()
    assert not (dev["views"][1]["mask"].astype(bool) & dev["skipped"][1].astype(bool)).any()
    GC.check_exact_scene(sc, dev, params)


def test_view_without_partner(emu):
    """View 3 is at depth 0.4, consistent with no other view: it emits nothing and receives no mark."""
    sc = _scene([2, 2, 2, 0.4], _cams([(1, (0.25 * c, -0.25 * c, 0)) for c in range(4)]))
    params = _p(num_consistent=1)
    dev = GC.run_device(sc, emu, params)
    assert dev["counts"][3] == 0 and not dev["used"][3].any() and dev["counts"][0] > 0
    GC.check_exact_scene(sc, dev, params)


def test_depth_range(emu):
    """Reference and source depths outside [depth_min, depth_max] take no part; the bounds themselves are inside."""
    sc = _shift_scene()
    d = sc["depth"]
    d[0, 0, :] = np.float32(1.0)        # below
    d[0, 1, :] = np.float32(1.6)        # == fp32(depth_min), above depth_min = 1.6 itself: inside
    d[0, 2, :] = np.float32(3.5)        # above
    d[2, 3, :] = np.float32(3.5)        # a source above
    d[3, 1, :] = np.float32(3.2)        # a source at fp32(depth_max), below 3.2 itself: inside
    params = _p(num_consistent=1, depth_min=1.6, depth_max=3.2)
    dev = GC.run_device(sc, emu, params)
    m0 = dev["views"][0]["mask"]
    assert not m0[0].any() and not m0[2].any() and m0[1].any()
    GC.check_exact_scene(sc, dev, params)
    params = _p(num_consistent=1, depth_min=float(np.float32(1.6)) * (1 + 1e-12), depth_max=3.2)
    dev = GC.run_device(sc, emu, params)
    assert not dev["views"][0]["mask"][1].any()
    GC.check_exact_scene(sc, dev, params)


# ---------------------------------------------------------------- the scene driver and the command line
def run_f23(fx, root, device, ply=None, **kw):
    views = {}
    res = G.fuse_scene_gipuma(str(root), ply, prob_threshold=float(fx["prob_threshold"]), device=device, return_skipped=True,
                              on_view=lambda r, out: views.__setitem__(r, {k: t.cpu().numpy().copy() for k, t in out.items()}), **kw)
    return res, [views[r] for r in range(len(views))]


def check_f23_fusion(fx, res, views, params=None):
    """fuse_scene_gipuma on F23 against the oracle on the reference's own filtered depth maps."""
    import tempfile
    params = params or GC.PARAMS
    depth, rgb, cams = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for v in range(4):
            p = os.path.join(tmp, "d.pfm")
            open(p, "wb").write(fx["out/depth_est/%08d_prob_filtered.pfm" % v].tobytes())
            depth.append(data_io.read_pfm(p)[0])
            p = os.path.join(tmp, "c.txt")
            open(p, "wb").write(fx["in/cams/%08d_cam.txt" % v].tobytes())
            K, E = data_io.read_camera_parameters(p)
            c = np.zeros((2, 4, 4), np.float32)
            c[0], c[1, :3, :3] = E, K
            cams.append(c)
            p = os.path.join(tmp, "i.png")
            open(p, "wb").write(fx["in/images/%08d.jpg" % v].tobytes())
            rgb.append(data_io.read_img(p))
    sc = {"depth": np.stack(depth).astype(np.float32), "rgb": np.stack(rgb), "cams": np.stack(cams)}
    dev = {"views": views, "skipped": res["skipped"], "xyz": res["xyz"], "rgb": res["rgb"], "counts": res["counts"]}
    nb, ne = GC.check_vs_oracle(sc, dev, params)
    assert res["views"].tolist() == [0, 1, 2, 3] and res["xyz"].shape[0] > 0
    return nb, ne


def test_fuse_scene_f23(emu, tmp_path):
    fx = load_f23()
    materialise_f23(fx, str(tmp_path))
    ply = str(tmp_path / "g.ply")
    st = {}
    res, views = run_f23(fx, tmp_path, emu, ply, stats=st)
    check_f23_fusion(fx, res, views)
    xyz, rgb = data_io.read_ply(ply)
    assert xyz.tobytes() == res["xyz"].tobytes() and np.array_equal(rgb, res["rgb"])
    assert set(st) == {"wall", "decode", "decode_wait", "write", "views", "vertices", "flushes", "gpu"} and st["vertices"] == xyz.shape[0]


def test_cli(emu, tmp_path, capsys):
    fx = load_f23()
    materialise_f23(fx, str(tmp_path))
    ply = str(tmp_path / "cli.ply")
    G.main(["--scan_folder", str(tmp_path), "--plyfilename", ply, "--prob_threshold", str(float(fx["prob_threshold"])), "--device", "cpu",
            "--num_consistent", "3", "--disp_threshold", "0.2"])
    res, _ = run_f23(fx, tmp_path, emu)
    xyz, rgb = data_io.read_ply(ply)
    assert xyz.tobytes() == res["xyz"].tobytes() and np.array_equal(rgb, res["rgb"]) and xyz.shape[0] > 0
    assert "(%d vertices" % xyz.shape[0] in capsys.readouterr().out


def test_sorted_view_order(emu, tmp_path):
    """Views are processed in sorted file-name order, whatever order the file system lists them in."""
    sc = GC.make_scene(5, 15, 21, 23)
    names = ["v3", "v0", "v4", "v1", "v2"]                 # created in this order; sorted: v0 .. v4 = scene views 1, 3, 4, 0, 2
    GC.write_scene_folder(str(tmp_path), sc, names=names)
    res = G.fuse_scene_gipuma(str(tmp_path), device=emu, prob_threshold=0.5)
    assert res["views"].tolist() == sorted(names)
    perm = [names.index(n) for n in sorted(names)]
    want = GC.run_device({k: v[perm] for k, v in sc.items()}, emu, GC.PARAMS)
    assert res["xyz"].tobytes() == want["xyz"].tobytes() and np.array_equal(res["rgb"], want["rgb"])
    other = GC.run_device(sc, emu, GC.PARAMS)
    assert res["xyz"].tobytes() != other["xyz"].tobytes()


def test_driver_errors(emu, tmp_path):
    fx = load_f23()
    materialise_f23(fx, str(tmp_path))
    with pytest.raises(ValueError, match="normal_thresh"):
        G.fuse_scene_gipuma(str(tmp_path), device=emu, normal_thresh=90)
    with pytest.raises(ValueError, match="normal_thresh"):
        G.main(["--scan_folder", str(tmp_path), "--plyfilename", str(tmp_path / "x.ply"), "--device", "cpu", "--normal_thresh", "179"])
    G.fuse_scene_gipuma(str(tmp_path), device=emu, normal_thresh=180)
    # a depth map without an image
    os.rename(tmp_path / "images" / "00000002.jpg", tmp_path / "x.jpg")
    with pytest.raises(ValueError, match="00000002.pfm has no image"):
        G.fuse_scene_gipuma(str(tmp_path), device=emu)
    os.rename(tmp_path / "x.jpg", tmp_path / "images" / "00000002.jpg")
    # an image of another size
    from PIL import Image
    Image.fromarray(np.zeros((10, 12, 3), np.uint8)).save(str(tmp_path / "images" / "00000001.jpg"), format="PNG")
    with pytest.raises(ValueError, match="00000001.jpg"):
        G.fuse_scene_gipuma(str(tmp_path), device=emu)
    # a depth map of another size
    materialise_f23(fx, str(tmp_path))
    data_io.save_pfm(str(tmp_path / "depth_est" / "00000003.pfm"), np.ones((24, 31), np.float32))
    with pytest.raises(ValueError):
        G.fuse_scene_gipuma(str(tmp_path), device=emu)
    # no views at all
    empty = tmp_path / "empty"
    os.makedirs(empty / "images")
    with pytest.raises(ValueError, match="no view"):
        G.fuse_scene_gipuma(str(empty), device=emu)
