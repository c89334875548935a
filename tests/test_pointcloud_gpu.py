"""GPU (MI355X): the point-cloud step end to end on the device - fixture F22 through fuse_scene, a full-size synthetic scene
(1920x1056, 9 sources, 6 reference views, both methods) whose PLY body must equal numpy's compaction of the same run's filter
outputs byte for byte, and run-to-run reproducibility of the written file."""
import os

import numpy as np
import pytest
import torch

from mvsformerplusplus_amd import data_io, pointcloud as PC, synth

from test_pointcloud import check_f22_case, load_f22, materialise_f22, run_f22

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("method", ["pcd", "dpcd"])
@pytest.mark.parametrize("conv", ["dtu", "tt"])
def test_f22_gpu(tmp_path, method, conv):
    fx = load_f22()
    materialise_f22(fx, str(tmp_path))
    ply = str(tmp_path / "scan.ply")
    res, masks = run_f22(fx, tmp_path, method, conv, DEV, ply)
    check_f22_case(fx, method, conv, res, masks)
    xyz, rgb = data_io.read_ply(ply)
    assert xyz.tobytes() == res["xyz"].tobytes() and np.array_equal(rgb, res["rgb"])


def _full_scene_run(method, scene, path, capacity=1 << 24):
    """6 reference views, each with the 9 other views of a 10-view scene as sources; -> (records, per-view (mask, points, rgb))."""
    dev = torch.device(DEV)
    d, c, cams, rgb = (scene[k].to(dev) for k in ("depth", "conf", "cams", "rgb"))
    V = d.shape[0]
    acc = PC.PointCloudAccumulator(dev, capacity=capacity)
    outs = []
    for r in range(6):
        srcs = [s for s in range(V) if s != r]
        gate = PC.conf_gate(c[r], 0.5, divide_uint8=True).float()
        sgate = torch.stack([PC.conf_gate(c[s], 0.5, divide_uint8=False) for s in srcs]).float()
        out = acc.add_view(d[r], gate, d[srcs], sgate if method == "pcd" else None, cams[r], cams[srcs], rgb[r], method, conf=0.5)
        outs.append((out["mask"][0].bool().cpu().numpy(), out["points"][0].cpu().numpy(), scene["rgb"][r].numpy()))
    acc.write_ply(path)
    return acc.records(), outs, acc.finalize()["counts"]


@pytest.mark.parametrize("method", ["pcd", "dpcd"])
def test_full_size_scene_bitwise(tmp_path, method):
    scene = synth.make_fusion_scene(10, 1056, 1920, seed=3)
    # a small capacity forces flushes in the middle of the scene
    rec, outs, counts = _full_scene_run(method, scene, str(tmp_path / "a.ply"), capacity=3 * 1056 * 1920)
    want = []
    for m, pts, rgb in outs:
        v = np.empty(int(m.sum()), data_io.PLY_VERTEX_DTYPE)
        for k, ch in enumerate("xyz"):
            v[ch] = pts[k][m]
        for k, ch in enumerate(("red", "green", "blue")):
            v[ch] = rgb[..., k][m]
        want.append(v.view(np.uint8))
    want = np.concatenate(want)
    assert counts.tolist() == [int(m.sum()) for m, _, _ in outs]
    assert 0.2 < counts.sum() / (6 * 1056 * 1920) < 0.95, counts        # the scene keeps a real, partial share of the pixels
    assert rec.size == want.size and rec.tobytes() == want.tobytes()
    raw = open(str(tmp_path / "a.ply"), "rb").read()
    assert raw == data_io.ply_header(rec.size // 15) + want.tobytes()
    # run to run: the same file, byte for byte
    rec2, _, _ = _full_scene_run(method, scene, str(tmp_path / "b.ply"))
    assert open(str(tmp_path / "b.ply"), "rb").read() == raw


def test_f22_reproducible_files(tmp_path):
    fx = load_f22()
    materialise_f22(fx, str(tmp_path))
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    run_f22(fx, tmp_path, "pcd", "tt", DEV, a)
    run_f22(fx, tmp_path, "pcd", "tt", DEV, b)
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 1000


@pytest.mark.parametrize("method", ["pcd", "dpcd"])
def test_full_size_scene_fp64(method):
    """Sibling of test_full_size_scene_bitwise against an independent reference: one 1152x1600 reference view with 10 rotated
    sources (synth.make_box_scene) through PointCloudAccumulator.  Each record's colour carries its pixel index, so the records
    name their pixels: every decided pixel the fp64 restatement keeps (parity_cases.fusion_vs_fp64) is a record, no decided
    pixel it drops is, and each record's xyz is within the rule's point bound of the fp64 point."""
    import parity_cases as P
    H, W, v = 1152, 1600, 10
    rd, rconf, sd, sconf, rc, sc = P._box_inputs(H, W, v, seed=5, rot_deg=3.0)
    idx = torch.arange(H * W, dtype=torch.int64).reshape(H, W)
    rgb = torch.stack([idx & 255, (idx >> 8) & 255, (idx >> 16) & 255], -1).to(torch.uint8)
    dev = torch.device(DEV)
    acc = PC.PointCloudAccumulator(dev, capacity=1 << 22)
    with torch.no_grad():
        out = acc.add_view(rd.to(dev), rconf.to(dev), sd.to(dev), sconf.to(dev) if method == "pcd" else None, rc.to(dev), sc.to(dev),
                           rgb.to(dev), method, conf=0.5)
    rec = acc.records().view(data_io.PLY_VERTEX_DTYPE)
    got = {"mask": out["mask"][0].cpu(), "points": out["points"][0].cpu(), "depth": out["depth"][0].cpu(), "geo_mask": out["geo_mask"][0].cpu()}
    dyn = method == "dpcd"
    st = P.fusion_vs_fp64(got, rd, rconf, sd, None if dyn else sconf, rc, sc, dynamic=dyn, conf_thresh=0.5,
                          p0=4.0 if dyn else 1.0, p1=1300.0 if dyn else 0.01, vthresh=2)
    pix = torch.from_numpy(rec["red"].astype(np.int64) | (rec["green"].astype(np.int64) << 8) | (rec["blue"].astype(np.int64) << 16))
    assert pix.numel() == int(got["mask"].sum()) and bool((pix[1:] > pix[:-1]).all())     # one record per kept pixel, row-major
    in_ply = torch.zeros(H * W, dtype=torch.bool)
    in_ply[pix] = True
    dec, keep = st["_decided"].reshape(-1), st["_mask64"].reshape(-1)
    assert torch.equal(in_ply[dec], keep[dec])
    assert 0.3 < float(keep.double().mean()) < 0.95
    # the records hold the filter's points bit for bit, and those met fusion_vs_fp64's point bound on every decided pixel above
    xyz = torch.from_numpy(np.stack([rec["x"], rec["y"], rec["z"]]))
    assert torch.equal(xyz, got["points"].reshape(3, -1)[:, pix])
