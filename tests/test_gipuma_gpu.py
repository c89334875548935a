"""GPU (MI355X): the Gipuma route on the device - the CPU file's small scenes and edge cases, a 16-view 576x800 scene checked
whole against the fp64 oracle, a DTU-shaped 49-view 1152x1600 scene checked per view on a fixed pixel sample through skipped,
run-to-run byte identity of the PLY, and fixture F23 through fuse_scene_gipuma end to end."""
import numpy as np
import pytest

import gipuma_cases as GC
import test_gipuma as T
from mvsformerplusplus_amd import data_io, gipuma as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# borderline shares (pixels with any borderline comparison, over the pixels evaluated).  At these sizes u
# and v carry fp32 errors of 1e-4 px and a pixel is compared against 15 / 48 views, four floors each, so many pixels have one
# near-integer coordinate among their consistent views.  Measured on the MI355X: 7.93 % of the DTU-shaped scene's sampled pixels,
# 5.07 % of the 16-view scene's pixels
DTU_BORDER_CAP = 0.12
S16_BORDER_CAP = 0.08


@pytest.mark.parametrize("V,H,W,nc,seed", T.EXACT_SCENES)
def test_exact_scene_gpu(V, H, W, nc, seed):
    T.test_exact_scene(DEV, V, H, W, nc, seed)


@pytest.mark.parametrize("case", ["num_consistent", "values", "disparity", "clamp", "z", "marked", "partner", "range"])
def test_edge_cases_gpu(case):
    if case == "num_consistent":
        for nc, emits in ((3, True), (2.5, True), (3.5, False), (4, False)):
            T.test_num_consistent_edge(DEV, nc, emits)
    elif case == "values":
        T.test_shift_scene_values(DEV)
    elif case == "disparity":
        T.test_disparity_at_threshold(DEV, 0.25, False)
        T.test_disparity_at_threshold(DEV, float(np.nextafter(np.float32(0.25), np.float32(1))), True)
    elif case == "clamp":
        T.test_clamped_texel(DEV)
    elif case == "z":
        T.test_z_not_positive(DEV)
    elif case == "marked":
        T.test_marked_reference_pixel(DEV)
    elif case == "partner":
        T.test_view_without_partner(DEV)
    else:
        T.test_depth_range(DEV)


def test_borderline_scene_gpu():
    T.test_borderline_scene_per_view(DEV)


def test_scene_16_views_whole():
    sc = GC.make_scene(16, 576, 800, seed=16)
    dev = GC.run_device(sc, DEV, GC.PARAMS, capacity=2 * 576 * 800)          # small buffer: flushes mid-scene
    nb, ne = GC.check_vs_oracle(sc, dev, GC.PARAMS)
    assert dev["xyz"].shape[0] > 0.2 * 576 * 800
    print("16-view scene: %d vertices, borderline %d of %d pixels (%.2f %%)" % (dev["xyz"].shape[0], nb, ne, 100.0 * nb / ne))
    assert nb <= S16_BORDER_CAP * ne, (nb, ne)


def test_dtu_shaped_scene_sampled():
    sc = GC.make_scene(49, 1152, 1600, seed=49)
    dev = GC.run_device(sc, DEV, GC.PARAMS)
    nb, ne = GC.check_vs_oracle(sc, dev, GC.PARAMS, pixels_per_view=4000, seed=1, check_marks=False)
    print("DTU-shaped scene: %d vertices, borderline %d of %d sampled pixels (%.2f %%)" % (dev["xyz"].shape[0], nb, ne, 100.0 * nb / ne))
    assert nb <= DTU_BORDER_CAP * ne, (nb, ne)
    assert dev["xyz"].shape[0] > 0


def test_ply_run_to_run_identical(tmp_path):
    sc = GC.make_scene(16, 576, 800, seed=7)
    GC.write_scene_folder(str(tmp_path / "scan"), sc)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ra = G.fuse_scene_gipuma(str(tmp_path / "scan"), a, device=DEV)
    G.fuse_scene_gipuma(str(tmp_path / "scan"), b, device=DEV)
    assert open(a, "rb").read() == open(b, "rb").read()
    xyz, _ = data_io.read_ply(a)
    assert xyz.shape[0] == int(ra["counts"].sum()) > 0


def test_f23_gpu(tmp_path):
    fx = T.load_f23()
    T.materialise_f23(fx, str(tmp_path))
    ply = str(tmp_path / "g.ply")
    st = {}
    res, views = T.run_f23(fx, tmp_path, DEV, ply, stats=st)
    T.check_f23_fusion(fx, res, views)
    xyz, rgb = data_io.read_ply(ply)
    assert xyz.tobytes() == res["xyz"].tobytes() and np.array_equal(rgb, res["rgb"]) and st["gpu"] > 0
