"""GPU (MI355X): a scene's depth inference on the device - the two kernels of csrc/scene_kernels.hip (the checks of tests/test_scene.py:
bit equality with the integer restatement and the normalisation table, at most 1 level from the fp64 bilinear), the ViT level cache with the
full ViT-B/14 (a view's levels alone = its slice of the batched run; forward(vit_levels=) = forward() on F29 case c's inputs) and the
driver end to end on a 4-view scene against direct calls of the network on inputs assembled by tests/scene_ref.py.  Every bar is bit
equality except the fp64 bilinear one.  One network (F29's arguments and seeded weights) serves the module, shared with
tests/test_network_gpu.py.  Never reads the reference tree."""
import os

import numpy as np
import pytest
import torch

import scene_ref
from test_network import F29_CASES, STAGES, case_inputs, shared_network
from test_scene import PACK_CASES, PREPARE_CASES, check_pack, check_prepare, check_vit_levels, kernel_refusals
from mvsformerplusplus_amd import data_io, pointcloud, scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("src,size", PREPARE_CASES)
def test_image_prepare_on_device(src, size):
    check_prepare(src, size, DEV)


@pytest.mark.parametrize("H,W,combine", PACK_CASES)
def test_depth_outputs_pack_on_device(H, W, combine):
    check_pack(H, W, combine, DEV)


def test_kernel_refusals_on_device():
    kernel_refusals(DEV)


def test_vit_levels_do_not_depend_on_the_batch_on_device():
    check_vit_levels(shared_network(DEV, F29_CASES["a"][3]), DEV)


def test_forward_with_cached_levels_equals_forward():
    """F29 case c's inputs: the levels computed view by view and handed back give every output of the plain forward, bit for bit."""
    H, W, V, rescale = F29_CASES["c"][:4]
    net = shared_network(DEV, rescale)
    imgs, projs, dv = case_inputs("c", DEV)
    with torch.no_grad():
        want = net(imgs, projs, dv)
        per_view = [net.vit_levels(imgs[0, v:v + 1]) for v in range(V)]
        levels = [torch.cat([per_view[v][l] for v in range(V)])[None] for l in range(len(per_view[0]))]
        got = net(imgs, projs, dv, vit_levels=levels)
    assert sorted(got) == sorted(want)
    for k in ("refined_depth", "photometric_confidence"):
        assert torch.equal(got[k], want[k]), k
    for k in STAGES:
        for name in ("depth", "photometric_confidence", "prob_volume"):
            assert torch.equal(got[k][name], want[k][name]), (k, name)


def test_driver_on_device(tmp_path):
    """4 views resized to 64 x 64, num_view 3, 192 depths: the written depth and confidence of every view equal a direct net(imgs, projs,
    dv) call on scene_ref's inputs bit for bit; the ViT cache on and off give byte-identical files; fuse_scene accepts the folder."""
    H = W = 64
    nviews, ndepths, scale = 3, 192, 1.06
    root = str(tmp_path / "in")
    scene_ref.write_scene(root, "scan4", 4, 80, 72, [(0, [1, 2, 3]), (1, [0, 2]), (2, [1, 3, 0]), (3, [2, 1])], seed=21)
    net = shared_network(DEV, F29_CASES["a"][3])
    kw = dict(dataset="dtu", num_view=nviews, numdepth=ndepths, interval_scale=scale, max_h=H, max_w=W, combine_reg_conf=True, device=DEV)
    st_off, st_on = {}, {}
    scene.infer_scene(net, root, ["scan4"], str(tmp_path / "off"), vit_cache=False, stats=st_off, **kw)
    scene.infer_scene(net, root, ["scan4"], str(tmp_path / "on"), vit_cache=True, stats=st_on, **kw)
    assert st_off["decodes"] == st_on["decodes"] == 4 and st_on["vit_views"] == 4 and st_off["vit_views"] == 0 and st_on["samples"] == 4
    want = scene_ref.samples(root, "scan4", nviews, ndepths, scale, H, W, "dtu", with_images=True)
    for w in want:
        name = "%08d" % w["view_ids"][0]
        imgs = torch.from_numpy(w["imgs"])[None].to(DEV)
        projs = {k: torch.from_numpy(w["proj_matrices"][k])[None].to(DEV) for k in STAGES}
        dv = torch.from_numpy(w["depth_values"])[None].to(DEV)
        with torch.no_grad():
            out = net(imgs, projs, dv)
        depth = out["refined_depth"][0].cpu().numpy()
        conf = (out["photometric_confidence"][0].cpu().numpy() * 3 + out["stage4"]["photometric_confidence"][0].cpu().numpy()) / 4
        got, _ = data_io.read_pfm(str(tmp_path / "off" / "scan4" / "depth_est" / (name + ".pfm")))
        assert np.isfinite(depth).all() and np.array_equal(got, depth), name
        assert np.array_equal(np.load(tmp_path / "off" / "scan4" / "confidence" / (name + ".npy")), (conf * 255).astype(np.uint8)), name
    for sub in ("depth_est", "confidence", "cams", "images"):
        names = sorted(os.listdir(tmp_path / "off" / "scan4" / sub))
        assert len(names) == 4 and names == sorted(os.listdir(tmp_path / "on" / "scan4" / sub))
        for name in names:
            assert (tmp_path / "off" / "scan4" / sub / name).read_bytes() == (tmp_path / "on" / "scan4" / sub / name).read_bytes(), (sub, name)
    res = pointcloud.fuse_scene(str(tmp_path / "on" / "scan4"), plyfilename=str(tmp_path / "scan4.ply"), method="dpcd", device=DEV)
    assert list(res["views"]) == [0, 1, 2, 3] and len(res["counts"]) == 4 and os.path.getsize(tmp_path / "scan4.ply") > 0
