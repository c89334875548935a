"""CPU: a scene's depth inference (mvsformerplusplus_amd.scene, csrc/scene_kernels.hip, DINOv2MVSNet.vit_levels) - the dataset contract
against tests/scene_ref.py (a numpy restatement of datasets/general_eval.py), the two kernels on the host emulator, the ViT level cache on
a 3-block ViT, and the driver with a stub network.  tests/test_scene_gpu.py runs the kernel and ViT checks of this file on the device.

Bars: everything here is bit equality, except the resize against round(fp64 bilinear at half-pixel centres, edges clamped): at most 1
level (coefficient rounding <= 0.13 level, the two >> 16 truncations < 0.5 together, the final rounding 0.5), asserted for the kernel and
for the integer restatement alone.  No real cv2.resize is compared anywhere: OpenCV is not a dependency of the project."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import scene_ref
from mvsformerplusplus_amd import DINOv2MVSNet, _lib, data_io, ops, pointcloud, scene, synth

STAGES = ("stage1", "stage2", "stage3", "stage4")
# (source h, w, tt pad rows) -> (H, W): identity, the test scene's size, upscaling, the tt pad, odd sizes (vector tails), one pixel, 2 x 3
PREPARE_CASES = [((64, 96, 0), (64, 96)), ((75, 100, 0), (64, 96)), ((30, 40, 0), (64, 96)), ((56, 96, 4), (64, 96)), ((13, 17, 0), (9, 11)),
                 ((1, 1, 0), (8, 8)), ((2, 3, 0), (8, 8))]
PACK_CASES = [(5, 7, False), (5, 7, True), (64, 96, False), (64, 96, True)]
_SHARED = {}


# ---- 1. the dataset contract ----------------------------------------------------------------------------------------------------------
PAIRS = [(0, [1, 2, 3, 4]), (1, [0, 2]), (2, []), (3, [4, 2, 1, 0]), (4, [3])]          # view 2 has no sources, views 1 and 4 fewer than num_view


def contract_scene(root):
    """5 views of 75 x 100; cams with and without the third token on line 11, a cams_1 variant for two views, short-range cameras."""
    key = ("contract", str(root))
    if key not in _SHARED:
        line11 = {0: "425.0 2.5", 1: "425.0 2.5 192.7", 2: "0.5 7.25", 3: "410.25 1.9 256 935.0", 4: "431.0 2.65"}
        scene_ref.write_scene(str(root), "Scan9", 5, 75, 100, PAIRS, seed=3, line11=line11, cams_1=(0, 3), short_range=True)
        # eth3d reads the second token as depth_max: a scene of its own, one view with a third token as well
        scene_ref.write_scene(str(root), "Pipes", 5, 75, 100, PAIRS, seed=4, line11={0: "0.5 7.25", 1: "1.25 30.5 64", 2: "0.5 9.0", 3: "0.75 12.5", 4: "2.0 41.0"})
        _SHARED[key] = str(root)
    return _SHARED[key]


@pytest.mark.parametrize("dataset,short", [("dtu", False), ("tt", False), ("tt", True), ("eth3d", False)])
def test_contract_matches_the_restatement(tmp_path_factory, dataset, short):
    root = contract_scene(tmp_path_factory.getbasetemp() / "scene_contract")
    nviews, ndepths, scale, H, W = 4, 192, 1.06, 64, 96
    scan = "Pipes" if dataset == "eth3d" else "Scan9"
    want = scene_ref.samples(root, scan, nviews, ndepths, scale, H, W, dataset, use_short_range=short)
    got = scene.scene_samples(os.path.join(root, scan), nviews, ndepths, scale, H, W, dataset, use_short_range=short, fix_res=True)
    assert [g["view_ids"] for g in got] == [w["view_ids"] for w in want] == [[0, 1, 2, 3], [1, 0, 2, 0], [3, 4, 2, 1], [4, 3, 3, 3]]
    for g, w in zip(got, want):
        assert g["ref"] == g["view_ids"][0] and g["filename"].format("depth_est", ".pfm") == "%s/depth_est/%08d.pfm" % (scan, g["ref"])
        assert sorted(g["proj_matrices"]) == sorted(STAGES)
        for k in STAGES:
            a, b = g["proj_matrices"][k], w["proj_matrices"][k]
            assert a.dtype == np.float32 and a.shape == (nviews, 2, 4, 4) and a.tobytes() == b.tobytes(), (dataset, k)
        assert g["depth_values"].dtype == np.float32 and g["depth_values"].tobytes() == w["depth_values"].tobytes()
        assert len(g["depth_values"]) == ndepths
    if dataset == "dtu":                # view 0 reads cams_1 (interval 2.5 whatever the file says), view 1 cams/ with a third token
        assert got[0]["depth_interval"] == 2.5 * scale and got[0]["depth_min"] == 430.5
        assert got[1]["depth_interval"] == (425.0 + 192 * 2.5 - 425.0) / ndepths * scale
    if dataset == "tt":
        assert got[0]["depth_min"] == (0.4 if short else 425.0)
    if dataset == "eth3d":              # the second token is depth_max
        assert got[1]["depth_min"] == 1.25 and got[1]["depth_interval"] == (30.5 - 1.25) / ndepths * scale


def test_contract_refusals(tmp_path_factory):
    root = contract_scene(tmp_path_factory.getbasetemp() / "scene_contract")
    folder = os.path.join(root, "Scan9")
    with pytest.raises(NotImplementedError, match="stage3"):
        scene.scene_samples(folder, 4, 192, 1.06, 64, 96, "dtu", stage3=True)
    with pytest.raises(ValueError, match="dataset"):
        scene.scene_samples(folder, 4, 192, 1.06, 64, 96, "blended")
    with pytest.raises(ValueError, match="num_view"):
        scene.scene_samples(folder, 1, 192, 1.06, 64, 96, "dtu")


# ---- 2. the kernels -------------------------------------------------------------------------------------------------------------------
def source_image(h, w):
    rng = np.random.default_rng(1000 * h + w)
    return scene_ref.smooth_image(rng, h, w) if h * w > 6 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def check_restatement(src, size):
    """The integer restatement alone against the fp64 bilinear: at most 1 level.  -> (resized uint8, worst difference)."""
    (h, w, pad), (H, W) = src, size
    img = source_image(h, w)
    padded = scene_ref.pad_tt(img, pad) if pad else img
    want = scene_ref.resize_u8(padded, H, W)
    worst = int(np.abs(want.astype(np.int64) - np.rint(scene_ref.bilinear_f64(padded, H, W)).astype(np.int64)).max())
    print("resize %s -> %s: the integer restatement is within %d level(s) of round(fp64 bilinear)" % (src, size, worst))
    assert worst <= 1, (src, size, worst)
    if (h + 2 * pad, w) == (H, W):
        assert np.array_equal(want, padded)                               # equal sizes: the identity
    return img, want


def check_prepare(src, size, device):
    (h, w, pad), (H, W) = src, size
    img, want = check_restatement(src, size)
    table = scene_ref.table()
    assert torch.equal(ops.normalise_table(), table)
    planar, resized = ops.image_prepare(torch.from_numpy(img).to(device), H, W, table.to(device), pad)
    assert planar.dtype == torch.float32 and tuple(planar.shape) == (3, H, W) and resized.dtype == torch.uint8 and tuple(resized.shape) == (H, W, 3)
    got = resized.cpu().numpy()
    assert np.array_equal(got, want), (src, size, int(np.abs(got.astype(int) - want.astype(int)).max()))
    assert planar.cpu().numpy().tobytes() == scene_ref.normalise(want).tobytes()          # ToTensor + Normalize, bit for bit
    padded = scene_ref.pad_tt(img, pad) if pad else img
    assert int(np.abs(got.astype(np.int64) - np.rint(scene_ref.bilinear_f64(padded, H, W)).astype(np.int64)).max()) <= 1
    # into a slot of a larger buffer (the view cache's use), at an offset that keeps 16-byte alignment and at one that does not
    for shift in (4, 1):
        buf_f = torch.full((3 * H * W + 8,), -7.0, device=device)
        buf_u = torch.full((3 * H * W + 8,), 9, dtype=torch.uint8, device=device)
        ops.image_prepare(torch.from_numpy(img).to(device), H, W, table.to(device), pad, planar=buf_f[shift:shift + 3 * H * W].view(3, H, W),
                          resized=buf_u[shift:shift + 3 * H * W].view(H, W, 3))
        assert torch.equal(buf_f[shift:shift + 3 * H * W].view(3, H, W), planar) and torch.equal(buf_u[shift:shift + 3 * H * W].view(H, W, 3), resized)
        assert bool((buf_f[:shift] == -7).all()) and bool((buf_f[shift + 3 * H * W:] == -7).all())
        assert bool((buf_u[:shift] == 9).all()) and bool((buf_u[shift + 3 * H * W:] == 9).all())


def check_pack(H, W, combine, device):
    g = torch.Generator().manual_seed(H * 100 + W + int(combine))
    depth = 400.0 + 500.0 * torch.rand(H, W, generator=g)
    conf, reg = torch.rand(H, W, generator=g), torch.rand(H, W, generator=g)
    conf.view(-1)[:4] = torch.tensor([0.0, 1.0, 0.99999994, 1.0 / 255.0])
    reg.view(-1)[:4] = torch.tensor([0.0, 1.0, 1.0, 0.0])
    out = ops.depth_outputs_pack(depth.to(device), conf.to(device), reg.to(device) if combine else None).cpu().numpy()
    assert out.dtype == np.uint8 and out.shape == (5 * H * W,)
    c = conf.numpy()
    if combine:
        c = (c * 3 + reg.numpy()) / 4                                     # test.py:282 on float32 arrays
    assert c.dtype == np.float32
    assert out[:4 * H * W].tobytes() == np.flipud(depth.numpy()).tobytes()
    assert out[4 * H * W:].tobytes() == (c * 255).astype(np.uint8).tobytes()


@pytest.mark.parametrize("src,size", PREPARE_CASES)
def test_image_prepare(emu, src, size):
    check_prepare(src, size, emu)


@pytest.mark.parametrize("H,W,combine", PACK_CASES)
def test_depth_outputs_pack(emu, H, W, combine):
    check_pack(H, W, combine, emu)


def test_pack_clamps(emu):
    """Out-of-range confidences are clamped to 0..255 and NaN gives 0 (numpy's cast is undefined there)."""
    conf = torch.tensor([[-0.5, 1.5, float("nan"), 2.0 / 255.0, float("inf")]])
    out = ops.depth_outputs_pack(torch.ones(1, 5), conf).numpy()
    assert out[20:].tolist() == [0, 255, 0, 2, 255]


def kernel_refusals(device):
    table = ops.normalise_table().to(device)
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device=device)
    for bad in (img.float(), img[..., :2], img[0], torch.zeros(0, 8, 3, dtype=torch.uint8, device=device)):
        with pytest.raises(ValueError, match=r"uint8 tensor \[h, w, 3\]"):
            ops.image_prepare(bad, 8, 8, table)
    with pytest.raises(ValueError, match="at least 1 x 1"):
        ops.image_prepare(img, 0, 8, table)
    for bad in (table.double(), table[:2], table[:, :255]):
        with pytest.raises(ValueError, match="table"):
            ops.image_prepare(img, 8, 8, bad)
    with pytest.raises(ValueError, match="planar"):
        ops.image_prepare(img, 8, 8, table, planar=torch.zeros(3, 8, 4, device=device))
    with pytest.raises(_lib.MvsHipError, match="pad_rows"):
        ops.image_prepare(img, 8, 8, table, pad_rows=65)
    d = torch.ones(4, 4, device=device)
    for bad in ((d.double(), d), (d, d.half()), (d, d[:2]), (d[:0], d[:0]), (d[0], d[0])):
        with pytest.raises(ValueError, match="fp32 tensor"):
            ops.depth_outputs_pack(*bad)
    with pytest.raises(ValueError, match="reg_conf"):
        ops.depth_outputs_pack(d, d, d.double())
    with pytest.raises(ValueError, match="5 H W"):
        ops.depth_outputs_pack(d, d, out=torch.zeros(79, dtype=torch.uint8, device=device))


def test_kernel_refusals(emu):
    kernel_refusals(emu)


def test_kernels_need_a_device():
    """Without the emulator the binding refuses host tensors: no PyTorch fall-back behind the wrappers."""
    with pytest.raises(_lib.MvsHipError):
        ops.image_prepare(torch.zeros(8, 8, 3, dtype=torch.uint8), 8, 8, ops.normalise_table())
    with pytest.raises(_lib.MvsHipError):
        ops.depth_outputs_pack(torch.ones(4, 4), torch.ones(4, 4))


# ---- 3. the ViT level cache -------------------------------------------------------------------------------------------------------------
def check_vit_levels(net, device, seed=5):
    """Three views whose ViT input is 28 x 28: each view's levels computed alone equal its slice of the batched run, bit for bit."""
    assert net.vit_size(64, 64) == (28, 28)
    views = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(device)
    with torch.no_grad():
        batched = net.vit_levels(views)
        assert len(batched) >= 2 and all(t.shape == (3, 4, 768) and t.is_contiguous() and t.dtype == torch.float32 for t in batched)
        for v in range(3):
            alone = net.vit_levels(views[v:v + 1])
            for a, b in zip(alone, batched):
                assert a.shape == (1, 4, 768) and torch.equal(a[0], b[v]), v
        pair = net.vit_levels(views[1:])
        for a, b in zip(pair, batched):
            assert torch.equal(a, b[1:])
    return batched


def test_vit_levels_do_not_depend_on_the_batch(emu):
    from test_network import f29_args
    args = f29_args()
    args["dino_cfg"] = dict(args["dino_cfg"], depth=3)
    net = DINOv2MVSNet(args)
    net.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(net.state_dict()), 3), strict=True)
    net.eval()
    check_vit_levels(net, emu)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
            net.vit_levels(torch.zeros(1, 3, 3, 64, 64))
        imgs = torch.zeros(1, 2, 3, 64, 64)
        with pytest.raises(ValueError, match="interval levels"):
            net.feature_maps(imgs, vit_levels=[torch.zeros(1, 3, 4, 768)] * 3)


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------------
class StubNet:
    """A callable with the forward's signature: deterministic maps from the inputs (so a wrong image, camera or depth range shows)."""

    def __init__(self):
        self.calls = []

    def __call__(self, imgs, proj_matrices, depth_values, tmp=(5.0, 5.0, 5.0, 1.0)):
        assert imgs.dim() == 5 and imgs.shape[0] == 1 and sorted(proj_matrices) == sorted(STAGES) and depth_values.dim() == 2
        self.calls.append((imgs.clone(), {k: v.clone() for k, v in proj_matrices.items()}, depth_values, list(tmp)))
        ref = imgs[0, 0]
        depth = depth_values[0, 0] + (ref[0] - ref[0].min()) * 7.0 + imgs[0, 1:].mean(dim=(0, 1)) + proj_matrices["stage4"][0, 0, 1, 0, 2] * 1e-3
        conf = torch.sigmoid(ref[1] + imgs[0, -1, 2])
        reg = torch.sigmoid(ref[2] * 2.0)
        return {"refined_depth": depth[None], "photometric_confidence": conf[None], "stage4": {"photometric_confidence": reg[None]}}


def driver_scene(root):
    key = ("driver", str(root))
    if key not in _SHARED:
        scene_ref.write_scene(str(root), "scan1", 5, 75, 100, PAIRS, seed=11, line11={3: "300.0 3.0"})
        scene_ref.write_scene(str(root), "scan2", 5, 75, 100, [(0, [1, 2]), (3, [4, 2]), (1, [0, 4])], seed=12)     # views 0 and 1 come back late
        _SHARED[key] = str(root)
    return _SHARED[key]


def counting_decoder():
    seen = []

    def decode(path):
        seen.append(os.path.basename(path))
        return scene.decode_image(path)

    return decode, seen


@pytest.mark.parametrize("combine", [False, True])
def test_driver_writes_what_the_network_returned(emu, tmp_path_factory, tmp_path, combine):
    root = driver_scene(tmp_path_factory.getbasetemp() / "scene_driver")
    H, W, nviews = 64, 96, 3
    net, (decode, seen), st = StubNet(), counting_decoder(), {}
    done = scene.infer_scene(net, root, ["scan1"], str(tmp_path), dataset="dtu", num_view=nviews, numdepth=48, interval_scale=1.06, max_h=H,
                             max_w=W, tmps=(4.0, 3.0, 2.0, 1.0), combine_reg_conf=combine, device=emu, decoder=decode, stats=st)
    want = scene_ref.samples(root, "scan1", nviews, 48, 1.06, H, W, "dtu", with_images=True)
    refs = [w["view_ids"][0] for w in want]
    assert done == {"scan1": refs} and refs == [0, 1, 3, 4]
    assert sorted(seen) == ["%08d.jpg" % v for v in range(5)] and st["decodes"] == 5 and st["samples"] == 4       # each image once per scene
    assert st["evictions"] == 0 and st["misses"] == 5 and st["hits"] == 4 * nviews - 5
    out = tmp_path / "scan1"
    assert sorted(os.listdir(out)) == ["cams", "confidence", "depth_est", "images", "pair.txt"]
    assert (out / "pair.txt").read_text() == open(os.path.join(root, "scan1", "pair.txt")).read()
    for sub, ext in (("depth_est", ".pfm"), ("confidence", ".npy"), ("cams", "_cam.txt"), ("images", ".jpg")):
        assert sorted(os.listdir(out / sub)) == ["%08d%s" % (r, ext) for r in refs]
    assert len(net.calls) == 4
    ranges = {}
    for w, (imgs, projs, dv, tmp) in zip(want, net.calls):
        ref = w["view_ids"][0]
        assert tmp == [4.0, 3.0, 2.0, 1.0] and imgs.shape == (1, nviews, 3, H, W)
        assert imgs[0].numpy().tobytes() == w["imgs"].tobytes()                   # the dataset's imgs, bit for bit
        for k in STAGES:
            assert projs[k].shape == (1, nviews, 2, 4, 4) and projs[k][0].numpy().tobytes() == w["proj_matrices"][k].tobytes()
        assert dv.shape == (1, 48) and dv[0].numpy().tobytes() == w["depth_values"].tobytes()
        ranges.setdefault(dv[0].numpy().tobytes(), set()).add(id(dv))
        res = StubNet()(imgs, projs, dv)
        depth, conf = res["refined_depth"][0].numpy(), res["photometric_confidence"][0].numpy()
        if combine:
            conf = (conf * 3 + res["stage4"]["photometric_confidence"][0].numpy()) / 4
        name = "%08d" % ref
        got, scale = data_io.read_pfm(str(out / "depth_est" / (name + ".pfm")))
        assert scale == 1.0 and got.dtype == np.float32 and np.array_equal(got, depth)
        data_io.save_pfm(str(tmp_path / "want.pfm"), depth)
        assert (out / "depth_est" / (name + ".pfm")).read_bytes() == (tmp_path / "want.pfm").read_bytes()      # the reference writer's bytes
        c = np.load(out / "confidence" / (name + ".npy"))
        assert c.dtype == np.uint8 and np.array_equal(c, (conf * 255).astype(np.uint8))
        K, E = data_io.read_camera_parameters(str(out / "cams" / (name + "_cam.txt")))
        assert np.array_equal(E, w["proj_matrices"]["stage4"][0, 0]) and np.array_equal(K, w["proj_matrices"]["stage4"][0, 1, :3, :3])
        data_io.write_cam(str(tmp_path / "want_cam.txt"), w["proj_matrices"]["stage4"][0])
        assert (out / "cams" / (name + "_cam.txt")).read_text() == (tmp_path / "want_cam.txt").read_text()
        resized = scene_ref.resize_u8(scene_ref.read_img(os.path.join(root, "scan1", "images", name + ".jpg"), "dtu"), H, W)
        Image.fromarray(resized).save(str(tmp_path / "want.jpg"), quality=95)          # PIL's encoding of the resized uint8 image itself
        assert (out / "images" / (name + ".jpg")).read_bytes() == (tmp_path / "want.jpg").read_bytes()
        assert data_io.read_img(str(out / "images" / (name + ".jpg"))).shape == (H, W, 3)
    assert len(ranges) == 2 and all(len(ids) == 1 for ids in ranges.values())      # ONE depth_values tensor per distinct (depth_min, interval)
    views = pointcloud.scene_views(str(out))
    assert [r for r, _ in views] == refs and views[0][1] == [1, 3, 4] and views[2][1] == [4, 1, 0]


def test_driver_lru_eviction(emu, tmp_path_factory, tmp_path):
    """A budget of two views (each 3 H W floats + 3 H W bytes): the running sample's views are held, everything else goes, the evicted
    views are decoded again and the files do not change."""
    root = driver_scene(tmp_path_factory.getbasetemp() / "scene_driver")
    H, W = 64, 96
    kw = dict(dataset="dtu", num_view=3, numdepth=48, interval_scale=1.06, max_h=H, max_w=W, device=emu)
    full, tiny = {}, {}
    (dec_a, seen_a), (dec_b, seen_b) = counting_decoder(), counting_decoder()
    scene.infer_scene(StubNet(), root, ["scan2"], str(tmp_path / "full"), decoder=dec_a, stats=full, **kw)
    scene.infer_scene(StubNet(), root, ["scan2"], str(tmp_path / "tiny"), decoder=dec_b, stats=tiny, cache_bytes=2 * 15 * H * W, **kw)
    assert full["evictions"] == 0 and len(seen_a) == 5
    assert tiny["evictions"] > 0 and len(seen_b) > 5 and tiny["decodes"] == len(seen_b)
    for sub in ("depth_est", "confidence", "cams", "images"):
        for name in sorted(os.listdir(tmp_path / "full" / "scan2" / sub)):
            assert (tmp_path / "full" / "scan2" / sub / name).read_bytes() == (tmp_path / "tiny" / "scan2" / sub / name).read_bytes(), (sub, name)
    cache = scene.ViewCache(budget=100)
    mk = lambda n: {"planar": torch.zeros(n), "rgb": torch.zeros(0, dtype=torch.uint8), "levels": None}       # noqa: E731
    cache.put(1, mk(10))
    cache.put(2, mk(10))
    assert cache.get(1) is not None                     # 1 is now the most recently used
    cache.put(3, mk(10))                                # 120 bytes > 100: the least recently used entry, 2, goes
    assert list(cache.entries) == [1, 3] and cache.evictions == 1 and cache.bytes == 80 and cache.get(2) is None
    cache.put(4, mk(10), held=(1,))                     # 1 is held by the running sample: 3 goes instead
    assert list(cache.entries) == [1, 4] and cache.evictions == 2


def test_driver_refusals(emu, tmp_path_factory, tmp_path):
    root = driver_scene(tmp_path_factory.getbasetemp() / "scene_driver")
    kw = dict(num_view=3, numdepth=48, interval_scale=1.06, max_h=64, max_w=96, device=emu)
    with pytest.raises(ValueError, match="vit_levels"):
        scene.infer_scene(StubNet(), root, ["scan1"], str(tmp_path), vit_cache=True, **kw)
    with pytest.raises(NotImplementedError, match="stage3"):
        scene.infer_scene(StubNet(), root, ["scan1"], str(tmp_path), stage3=True, **kw)
    with pytest.raises(ValueError, match="uint8 RGB"):
        scene.infer_scene(StubNet(), root, ["scan1"], str(tmp_path), decoder=lambda p: np.zeros((4, 4), np.float32), **kw)
    with pytest.raises(ValueError, match="refined_depth"):
        scene.infer_scene(lambda *a: {"refined_depth": torch.zeros(1, 8, 8), "photometric_confidence": torch.zeros(1, 8, 8)}, root, ["scan1"],
                          str(tmp_path), **kw)
    with pytest.raises(NotImplementedError, match="batch_size"):
        scene.main(["--config", "none.json", "--outdir", str(tmp_path), "--interval_scale", "1.06", "--batch_size", "2", "--testpath", root])
