"""CPU: the point-cloud step (mvsformerplusplus_amd/pointcloud.py, csrc/pointcloud_kernels.hip on the host emulator) - PLY
format, pair-file and confidence quirks of the reference's drivers, bitwise compaction order, and the whole scene driver against
fixture F22 (tests/golden/make_golden_pointcloud.py, generated from the reference)."""
import os

import numpy as np
import pytest
import torch

from mvsformerplusplus_amd import data_io, pointcloud as PC

from conftest import GOLDEN

PLY_HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def test_ply_header_and_roundtrip(tmp_path):
    xyz = np.array([[1.5, -2.0, 3.25], [0.0, 1e-30, -7.0], [np.inf, -0.0, 5.0]], np.float32)
    rgb = np.array([[0, 128, 255], [1, 2, 3], [250, 251, 252]], np.uint8)
    p = str(tmp_path / "a.ply")
    data_io.write_ply(p, xyz, rgb)
    raw = open(p, "rb").read()
    assert raw.startswith(PLY_HEADER) and len(raw) == len(PLY_HEADER) + 3 * 15
    body = raw[len(PLY_HEADER):]
    assert body[:15] == xyz[0].astype("<f4").tobytes() + rgb[0].tobytes()
    x2, c2 = data_io.read_ply(p)
    assert x2.tobytes() == xyz.tobytes() and np.array_equal(c2, rgb)
    q = str(tmp_path / "b.ply")
    data_io.write_ply_records(q, np.frombuffer(body, np.uint8))
    assert open(q, "rb").read() == raw


def _write_pair(path, rows):
    with open(path, "w") as f:
        f.write("%d\n" % len(rows))
        for ref, srcs in rows:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d 1.0" % s for s in srcs)))


def test_pair_file_quirks(tmp_path):
    p = str(tmp_path / "pair.txt")
    _write_pair(p, [(0, list(range(1, 13))), (1, []), (2, [5, 6])])
    assert data_io.read_pair_file(p, "dtu") == [(0, list(range(1, 13))), (2, [5, 6])]          # empty line dropped
    assert data_io.read_pair_file(p, "tt", 10) == [(0, list(range(1, 10))), (2, [5, 6, 5, 5, 5, 5, 5, 5, 5])]
    assert data_io.read_pair_file(p, "tt", 4) == [(0, [1, 2, 3]), (2, [5, 6, 5])]
    with pytest.raises(ValueError):
        data_io.read_pair_file(p, "eth3d")
    # scene_views: dtu keeps the first 10 sources; tt prefers new_pair.txt; sources without a camera are skipped; a repeated
    # reference keeps its first place and its last entry
    scan = tmp_path / "scan"
    os.makedirs(scan / "cams")
    for v in range(14):
        if v != 3:
            open(scan / "cams" / ("%08d_cam.txt" % v), "w").close()
    _write_pair(str(scan / "pair.txt"), [(0, list(range(1, 14))), (5, [1, 2]), (0, [4, 3, 2])])
    assert PC.scene_views(str(scan), convention="dtu") == [(0, [4, 2]), (5, [1, 2])]
    assert PC.scene_views(str(scan), convention="tt", n_src_views=4) == [(0, [4, 2]), (5, [1, 2, 1])]
    _write_pair(str(scan / "new_pair.txt"), [(7, [8, 3])])
    assert PC.scene_views(str(scan), convention="tt", n_src_views=4) == [(7, [8, 8])]
    assert PC.scene_views(str(scan), convention="dtu")[0] == (0, [4, 2])


def test_conf_gate_per_convention():
    c = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    for t in (0.5, 0.3, 128 / 255, 0.0, 1.0, -1.0, 254.5, 255.0):
        ref = torch.from_numpy(c.numpy() / 255) > t                       # test.py:354-355: uint8 / 255 (float64), then > conf
        raw = c > t                                                        # test.py:389 on the raw uint8 sources
        assert torch.equal(PC.conf_gate(c, t, divide_uint8=True), ref), t
        assert torch.equal(PC.conf_gate(c, t, divide_uint8=False), raw), t
    f = torch.tensor([0.49, 0.5, 0.5000001, 0.9], dtype=torch.float32)
    assert PC.conf_gate(f, 0.5, divide_uint8=True).tolist() == [False, False, True, True]


def _view(h, w, seed, kind="rand"):
    g = torch.Generator().manual_seed(seed)
    if kind == "zeros":
        m = torch.zeros(h, w, dtype=torch.bool)
    elif kind == "ones":
        m = torch.ones(h, w, dtype=torch.bool)
    elif kind == "last":
        m = torch.zeros(h, w, dtype=torch.bool)
        m[-1, -1] = True
    else:
        m = torch.rand(h, w, generator=g) < 0.6
    pts = torch.randn(3, h, w, generator=g) * 100
    special = torch.tensor([float("nan"), float("inf"), -0.0])[:w]
    pts[0, 0, :special.numel()] = special
    rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    return m, pts, rgb


def _numpy_compaction(views):
    recs = []
    for m, pts, rgb in views:
        mm = m.numpy()
        v = np.empty(int(mm.sum()), data_io.PLY_VERTEX_DTYPE)
        for k, c in enumerate("xyz"):
            v[c] = pts[k].numpy()[mm]                                       # points_np[i, k][mask_np[i, 0]], test.py:419
        for k, c in enumerate(("red", "green", "blue")):
            v[c] = rgb.numpy()[..., k][mm]
        recs.append(v.view(np.uint8))
    return np.concatenate(recs)


@pytest.mark.parametrize("views,capacity", [
    ([(48, 64, "zeros"), (48, 64, "ones")], 1 << 20),
    ([(37, 41, "last"), (33, 65, "rand")], 1 << 20),                       # w not a multiple of 64, h*w not of the 1024-pixel tile
    ([(48, 64, "ones"), (31, 77, "rand"), (1, 1, "ones"), (40, 30, "rand")], 1 << 20),
    ([(20, 30, "rand"), (20, 30, "ones"), (5, 7, "rand"), (20, 30, "rand"), (20, 30, "last")], 700),   # several flushes, one growth
])
def test_compaction_exact(emu, views, capacity):
    """Records bitwise equal to numpy's masking, in order, across views (NaN / inf / -0 bit patterns included)."""
    vs = [_view(h, w, 100 + i, kind) for i, (h, w, kind) in enumerate(views)]
    acc = PC.PointCloudAccumulator(emu, capacity=capacity)
    for m, pts, rgb in vs:
        acc.append(m, pts, rgb)
    want = _numpy_compaction(vs)
    got = acc.records()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    fin = acc.finalize()
    assert fin["counts"].tolist() == [int(m.sum()) for m, _, _ in vs]
    if capacity < 1000:
        assert acc.flushes >= 3


def materialise_f22(fx, root):
    """Write fixture F22's scene files under `root` (the layout fuse_scene reads)."""
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for v in range(fx["depth"].shape[0]):
        data_io.save_pfm(os.path.join(root, "depth_est", "%08d.pfm" % v), fx["depth"][v])
        np.save(os.path.join(root, "confidence", "%08d.npy" % v), fx["conf"][v])
        with open(os.path.join(root, "cams", "%08d_cam.txt" % v), "w") as f:
            f.write(str(fx["cam%d" % v]))
        with open(os.path.join(root, "images", "%08d.jpg" % v), "wb") as f:
            f.write(fx["img%d" % v].tobytes())
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write(str(fx["pair_dtu"]))
    with open(os.path.join(root, "new_pair.txt"), "w") as f:
        f.write(str(fx["pair_tt"]))


def load_f22():
    return dict(np.load(os.path.join(GOLDEN, "f22_point_cloud.npz")))


def check_f22_case(fx, method, conv, res, masks):
    """The f10 bars: per-view mask mismatch <= 0.5 %; vertices matched by (view, pixel): positions <= 5e-3, colours exact; the
    common vertices in the same relative order."""
    key = "%s_%s_" % (method, conv)
    views = fx[key + "views"]
    assert res["views"].tolist() == views.tolist()
    ours_vid, ours_pix = [], []
    for i, vid in enumerate(views):
        m = masks[int(vid)]
        assert float((m != fx[key + "masks"][i]).mean()) <= 5e-3, (key, int(vid))
        assert int(res["counts"][i]) == int(m.sum())
        p = np.flatnonzero(m)
        ours_vid.append(np.full(p.size, vid))
        ours_pix.append(p)
    ours = np.concatenate(ours_vid).astype(np.int64) * 10 ** 7 + np.concatenate(ours_pix)
    ref = fx[key + "vid"].astype(np.int64) * 10 ** 7 + fx[key + "pix"]
    assert ours.size == res["xyz"].shape[0]
    common, io_, ir = np.intersect1d(ours, ref, assume_unique=True, return_indices=True)
    assert common.size >= 0.99 * max(ours.size, ref.size)
    # relative order: the views' emission order, then row-major; map keys to (emission rank, pixel)
    rank = {int(v): i for i, v in enumerate(views)}
    seq = lambda idx, keys: np.array([rank[int(k // 10 ** 7)] * 10 ** 7 + k % 10 ** 7 for k in keys[np.sort(idx)]])
    assert (np.diff(seq(io_, ours)) > 0).all() and (np.diff(seq(ir, ref)) > 0).all()
    assert np.array_equal(ours[np.sort(io_)], ref[np.sort(ir)])
    assert np.abs(res["xyz"][io_] - fx[key + "xyz"][ir]).max() <= 5e-3
    assert np.array_equal(res["rgb"][io_], fx[key + "rgb"][ir])


def run_f22(fx, root, method, conv, device, ply=None):
    masks = {}
    res = PC.fuse_scene(str(root), plyfilename=ply, method=method, convention=conv, conf=float(fx["conf_thresh"]),
                        thres_view=int(fx["thres_view"]), thres_disp=float(fx["thres_disp"]), dist_base=float(fx["dist_base"]),
                        rel_diff_base=float(fx["rel_diff_base"]), n_src_views=int(fx["fusion_view"]) if conv == "tt" else 10,
                        device=device, on_view=lambda vid, out: masks.__setitem__(int(vid), out["mask"][0].cpu().numpy()))
    return res, masks


@pytest.mark.parametrize("method", ["pcd", "dpcd"])
@pytest.mark.parametrize("conv", ["dtu", "tt"])
def test_fuse_scene_f22(emu, tmp_path, method, conv):
    fx = load_f22()
    materialise_f22(fx, str(tmp_path))
    ply = str(tmp_path / "scan.ply")
    res, masks = run_f22(fx, tmp_path, method, conv, emu, ply)
    check_f22_case(fx, method, conv, res, masks)
    xyz, rgb = data_io.read_ply(ply)
    assert xyz.tobytes() == res["xyz"].tobytes() and np.array_equal(rgb, res["rgb"])


def test_cli_f22(emu, tmp_path):
    fx = load_f22()
    materialise_f22(fx, str(tmp_path))
    ply = str(tmp_path / "cli.ply")
    PC.main(["--scan_folder", str(tmp_path), "--plyfilename", ply, "--filter_method", "dpcd", "--device", "cpu"])
    res, _ = run_f22(fx, tmp_path, "dpcd", "dtu", emu)
    xyz, rgb = data_io.read_ply(ply)
    assert xyz.tobytes() == res["xyz"].tobytes() and np.array_equal(rgb, res["rgb"]) and xyz.shape[0] > 0


def test_image_size_mismatch(emu, tmp_path):
    fx = load_f22()
    materialise_f22(fx, str(tmp_path))
    from PIL import Image
    bad = os.path.join(str(tmp_path), "images", "%08d.jpg" % 2)
    Image.fromarray(np.zeros((10, 12, 3), np.uint8)).save(bad, format="PNG")
    with pytest.raises(ValueError, match="00000002.jpg"):
        PC.fuse_scene(str(tmp_path), method="dpcd", device=emu)
