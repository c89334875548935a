"""Synthetic multi-view scenes for tests, golden fixtures and ``bench.py``.

No DTU / Tanks&Temples data or checkpoints exist in the build or GPU containers, so
every workload is synthetic.  The layout mirrors what the reference
dataset emits (``datasets/general_eval.py:211-242``):

* ``proj_matrices["stageK"]``: ``[B, V, 2, 4, 4]`` fp32, ``[:, :, 0]`` = extrinsic 4x4,
  ``[:, :, 1, :3, :3]`` = intrinsic 3x3; per-stage intrinsics scaled by 0.5 / 1 / 2 / 4
  relative to the quarter-resolution intrinsics.
* ``depth_values``: ``[B, numdepth]`` (only first/last element are used by the cascade).
* ``features["stageK"]``: ``[B, V, C, H/8.., W/8..]`` with C = 64/32/16/8.

Features are an analytic multi-channel texture painted on a smooth depth surface and
observed from every camera, so the group-wise correlation really peaks at the true
depth (a flat-noise volume would make depth regression degenerate).

Everything here is plain torch on the CPU; callers move tensors to the GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

STAGE_CH = (64, 32, 16, 8)          # config/mvsformer++.json feat_chs reversed per stage
STAGE_DOWN = (8, 4, 2, 1)           # stage s runs at 1/8, 1/4, 1/2, 1/1 resolution


def make_cameras(V: int, H: int, W: int, *, baseline: float = 25.0, rot_deg: float = 0.0,
                 seed: int = 0, batch: int = 1) -> torch.Tensor:
    """Full-resolution DTU-like pinhole cameras -> ``[B, V, 2, 4, 4]``.

    fx = fy = 2892.33 * (W / 1600) (DTU focal length scaled to the image width),
    principal point at the image centre, view v translated by ``baseline * v`` mm along x
    (alternating sign) and a little along y, optionally rotated by up to ``rot_deg`` degrees.
    """
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(batch, V, 2, 4, 4, dtype=torch.float32)
    f = 2892.33 * (W / 1600.0)
    for b in range(batch):
        for v in range(V):
            K = torch.eye(4, dtype=torch.float64)
            K[0, 0] = f
            K[1, 1] = f
            K[0, 2] = W / 2.0
            K[1, 2] = H / 2.0
            E = torch.eye(4, dtype=torch.float64)
            if v > 0:
                sign = 1.0 if (v % 2) else -1.0
                E[0, 3] = sign * baseline * ((v + 1) // 2)
                E[1, 3] = 0.15 * baseline * (((v * 7) % 5) - 2) / 2.0
                if rot_deg > 0:
                    ang = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 2 * math.radians(rot_deg)
                    cx, cy, cz = torch.cos(ang)
                    sx, sy, sz = torch.sin(ang)
                    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
                    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
                    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
                    E[:3, :3] = Rz @ Ry @ Rx
            out[b, v, 0] = E.float()
            out[b, v, 1, :3, :3] = K[:3, :3].float()
    return out


def stage_proj_matrices(full_res_proj: torch.Tensor, n_stages: int = 4) -> Dict[str, torch.Tensor]:
    """Scale the intrinsics per stage the way ``general_eval.py:229-242`` does.

    ``full_res_proj`` holds FULL-resolution intrinsics; stage s (1-based) runs at
    1/2**(n_stages - s) of full resolution, so rows 0-1 of K are divided accordingly.
    """
    out = {}
    for s in range(n_stages):
        scale = 1.0 / (2 ** (n_stages - 1 - s))
        p = full_res_proj.clone()
        p[:, :, 1, :2, :] = p[:, :, 1, :2, :] * scale
        out["stage%d" % (s + 1)] = p
    return out


def _surface_depth(xn: torch.Tensor, yn: torch.Tensor, dmin: float, dmax: float) -> torch.Tensor:
    """Smooth reference-frame depth map in [dmin, dmax] as a function of normalised pixel coords."""
    mid = 0.5 * (dmin + dmax)
    amp = 0.30 * (dmax - dmin)
    return mid + amp * (0.6 * torch.sin(2.1 * xn + 0.3) * torch.cos(1.7 * yn - 0.2) + 0.4 * torch.sin(3.3 * yn + 1.1))


def _texture(X: torch.Tensor, Y: torch.Tensor, C: int, wavelength: float, seed: int) -> torch.Tensor:
    """Analytic C-channel texture f_c(X, Y) on the world plane (mm units)."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = 2 * math.pi / wavelength
    a = (torch.rand(C, 3, generator=g, dtype=torch.float64) * 2 - 1) * k
    b = (torch.rand(C, 3, generator=g, dtype=torch.float64) * 2 - 1) * k
    ph = torch.rand(C, 3, generator=g, dtype=torch.float64) * 2 * math.pi
    amp = (1.0, 0.6, 0.35)
    a, b, ph = a.to(X.device), b.to(X.device), ph.to(X.device)
    out = torch.zeros((C,) + tuple(X.shape), dtype=torch.float64, device=X.device)
    for j in range(3):
        mult = float(2 ** j)
        out += amp[j] * torch.sin(mult * (a[:, j, None, None] * X + b[:, j, None, None] * Y) + ph[:, j, None, None])
    return out


def make_features(proj_stage: torch.Tensor, C: int, H: int, W: int, *, dmin: float, dmax: float,
                  noise: float = 0.05, seed: int = 0, dtype=torch.float32, device=None) -> torch.Tensor:
    """Geometrically consistent features ``[B, V, C, H, W]`` for one stage.

    The scene is the depth surface ``_surface_depth`` seen from the reference camera.  For a
    source view the surface point behind each source pixel is found by two fixed-point
    iterations (exact for pure translations with equal z), which is accurate enough for a
    benchmark texture; a little white noise decorrelates the views.
    """
    B, V = proj_stage.shape[:2]
    device = torch.device("cpu") if device is None else torch.device(device)
    on_cpu = device.type == "cpu"
    g = torch.Generator(device=device).manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device), torch.arange(W, dtype=torch.float64, device=device), indexing="ij")
    feats = torch.zeros(B, V, C, H, W, dtype=torch.float32, device=device)
    proj_stage = proj_stage.to(device)
    for b in range(B):
        K0 = proj_stage[b, 0, 1, :3, :3].double()
        E0 = proj_stage[b, 0, 0].double()
        # texture wavelength ~ 6 pixels of this stage at mid depth
        wl = 6.0 * (0.5 * (dmin + dmax)) / float(K0[0, 0])
        for v in range(V):
            K = proj_stage[b, v, 1, :3, :3].double()
            E = proj_stage[b, v, 0].double()
            # relative pose view v -> ref
            T = (E0.cpu() @ torch.inverse(E.cpu())).to(device)          # X_ref = T @ X_v
            rx = (xs - K[0, 2]) / K[0, 0]
            ry = (ys - K[1, 2]) / K[1, 1]
            z = torch.full_like(xs, 0.5 * (dmin + dmax))
            for _ in range(3):
                Xv = torch.stack([rx * z, ry * z, z, torch.ones_like(z)], 0).reshape(4, -1)
                Xr = (T @ Xv).reshape(4, H, W)
                ur = (Xr[0] / Xr[2]) * K0[0, 0] + K0[0, 2]
                vr = (Xr[1] / Xr[2]) * K0[1, 1] + K0[1, 2]
                zr = _surface_depth(ur / W * 2 - 1, vr / H * 2 - 1, dmin, dmax)
                # move the guess so that the ref-frame depth matches the surface
                z = z + (zr - Xr[2])
            Xv = torch.stack([rx * z, ry * z, z, torch.ones_like(z)], 0).reshape(4, -1)
            Xr = (T @ Xv).reshape(4, H, W)
            Xw = (torch.inverse(E0.cpu()).to(device) @ Xr.reshape(4, -1)).reshape(4, H, W)
            tex = _texture(Xw[0], Xw[1], C, wl, seed)
            tex = tex + noise * torch.randn(tex.shape, generator=g, dtype=torch.float64, device=device)
            feats[b, v] = tex.float()
    return feats.to(dtype)


def true_depth(proj_stage: torch.Tensor, H: int, W: int, dmin: float, dmax: float) -> torch.Tensor:
    """Ground-truth reference-view depth ``[H, W]`` of the synthetic surface."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return _surface_depth(xs / W * 2 - 1, ys / H * 2 - 1, dmin, dmax).float()


def make_cascade_inputs(H: int, W: int, V: int, *, numdepth: int = 192, depth_min: float = 425.0,
                        depth_interval: float = 2.65, baseline: float = 25.0, rot_deg: float = 0.0,
                        seed: int = 0, batch: int = 1, feat_dtype=torch.float32,
                        stage_ch: Tuple[int, ...] = STAGE_CH, device=None,
                        cams: Optional[torch.Tensor] = None) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor], torch.Tensor]:
    """(features, proj_matrices, depth_values) for a 4-stage cascade at full resolution HxW.

    ``cams``: full-resolution cameras ``[batch, V, 2, 4, 4]`` to use instead of ``make_cameras`` (the default).

    ``depth_values`` mirrors ``general_eval.py:223``: arange(dmin, interval*(nd-0.5)+dmin, interval).
    H and W must be divisible by 64 (SURVEY.md §7 "odd sizes").
    """
    assert H % 64 == 0 and W % 64 == 0, "image size must be divisible by 64"
    dv = torch.arange(depth_min, depth_interval * (numdepth - 0.5) + depth_min, depth_interval, dtype=torch.float32)
    depth_values = dv[None].repeat(batch, 1)
    dmax = float(dv[-1])
    if cams is None:
        cams = make_cameras(V, H, W, baseline=baseline, rot_deg=rot_deg, seed=seed, batch=batch)
    assert tuple(cams.shape) == (batch, V, 2, 4, 4), "cams must be [batch, V, 2, 4, 4]"
    projs = stage_proj_matrices(cams.float().cpu(), len(stage_ch))
    feats = {}
    # keep the surface away from the ends of the hypothesis range
    lo = depth_min + 0.15 * (dmax - depth_min)
    hi = dmax - 0.15 * (dmax - depth_min)
    for s, C in enumerate(stage_ch):
        down = 2 ** (len(stage_ch) - 1 - s)
        feats["stage%d" % (s + 1)] = make_features(projs["stage%d" % (s + 1)], C, H // down, W // down,
                                                   dmin=lo, dmax=hi, seed=seed + s, dtype=feat_dtype, device=device)
    if device is not None:
        projs = {k: v.to(device) for k, v in projs.items()}
        depth_values = depth_values.to(device)
    return feats, projs, depth_values


def randomize_bn_(module: torch.nn.Module, seed: int = 0) -> None:
    """Randomise BatchNorm affine + running stats so BN folding is exercised."""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)


def seeded_state_dict(shapes: Dict[str, Tuple[int, ...]], seed: int) -> Dict[str, torch.Tensor]:
    """Deterministic weights for a state-dict manifest ``{key: shape}``.

    Uses numpy's frozen legacy ``RandomState`` stream with a per-key sub-seed (crc32 of the key), so
    the same key/shape/seed gives bit-identical fp32 values on every machine and numpy version and
    independent of key order.  Golden fixtures therefore store only the manifest + seed, not ~1.2 MB
    of incompressible weights per StageNet.  Conv weights ~ N(0, 2/fan_in); BN weight ~ U(.5,1.5),
    running_var ~ U(.5,1.5), running_mean / biases ~ N(0,.2).
    """
    import zlib

    import numpy as np
    out: Dict[str, torch.Tensor] = {}
    for k, shp in shapes.items():
        shp = tuple(int(s) for s in shp)
        rs = np.random.RandomState((zlib.crc32(k.encode()) + 7919 * int(seed)) % (2 ** 32))
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros(shp, dtype=torch.int64)
            continue
        if k.endswith("running_var") or (len(shp) == 1 and k.endswith("weight")) or k.endswith(("gamma1", "gamma2")):
            a = rs.uniform(0.5, 1.5, size=shp)
        elif k.endswith("running_mean") or k.endswith("bias"):
            a = rs.standard_normal(size=shp) * 0.2
        else:
            fan_in = 1
            for s in shp[1:]:
                fan_in *= s
            a = rs.standard_normal(size=shp) * math.sqrt(2.0 / max(fan_in, 1))
        out[k] = torch.from_numpy(np.asarray(a, dtype=np.float32))           # (a 0-d shape gives a numpy scalar)
    return out


def state_dict_manifest(sd) -> Dict[str, Tuple[int, ...]]:
    return {k: tuple(v.shape) for k, v in sd.items()}


def make_fusion_scene(V: int, H: int, W: int, *, seed: int = 0, baseline: float = 30.0) -> Dict[str, torch.Tensor]:
    """The outputs of an inference run over V views, for the depth-map filtering and point-cloud step: depth maps of one tilted
    plane seen from V translated cameras (closed form) with ~0.5 mm noise, 5 % outliers and a hole strip; uint8 confidences as
    test.py saves them (a low-confidence band included); smooth RGB images with a sparse checker.
    -> depth [V,H,W] fp32, conf [V,H,W] uint8, cams [V,2,4,4], rgb [V,H,W,3] uint8 (CPU)."""
    g = torch.Generator().manual_seed(seed)
    cams = make_cameras(V, H, W, baseline=baseline, rot_deg=0.0, seed=seed)[0]
    a, b, z0 = 0.15, -0.1, 600.0
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5, torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
    depths = []
    for v in range(V):
        K, E = cams[v, 1, :3, :3], cams[v, 0]
        C = -E[:3, 3]
        rx, ry = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
        depths.append((z0 + a * C[0] + b * C[1] - C[2]) / (1 - a * rx - b * ry))
    d = torch.stack(depths)
    d = d * (1 + 0.0008 * torch.randn(d.shape, generator=g))
    d = torch.where(torch.rand(d.shape, generator=g) < 0.05, d * (1 + 0.05 * torch.randn(d.shape, generator=g)), d)
    d[:, :, :max(1, W // 20)] = 0.0
    conf = torch.rand(d.shape, generator=g) * 0.5 + 0.5
    conf[:, H // 5:H // 3, :] *= 0.6
    conf = (conf * 255).to(torch.uint8)
    xr = (torch.arange(W)[None, :] * 4) % 256
    yr = (torch.arange(H)[:, None] * 5) % 256
    rgb = torch.stack([torch.stack([(xr + 20 * v).expand(H, W) % 256, (yr + 30 * v).expand(H, W) % 256,
                                    torch.full((H, W), (40 * v) % 256)], -1) for v in range(V)]).to(torch.uint8)
    rgb[:, ::7, ::5] = 255 - rgb[:, ::7, ::5]
    return {"depth": d.contiguous(), "conf": conf.contiguous(), "cams": cams.contiguous(), "rgb": rgb.contiguous()}


def make_box_scene(V: int, H: int, W: int, *, seed: int = 0, metres: bool = False, rot_deg: float = 3.0,
                   conf_thresh: float = 0.5) -> Dict[str, torch.Tensor]:
    """A harder scene for the depth-map filters than make_fusion_scene: a box in front of a slanted plane (occlusion edges,
    so bilinear taps straddle depth discontinuities) seen by V rotated cameras (make_cameras with ``rot_deg``).  DTU scale
    (mm, depths ~400..870, 30 mm baseline) or, with ``metres``, a Tanks-and-Temples-like one (m, depths ~2.5..9, 0.4 m
    baseline).  Depths are ray-cast in fp64, then get ~0.08 % noise and 2 % outliers; zero-depth holes (a strip and 0.1 %
    scattered pixels).  Float confidences in [0.55, 1) with a low-confidence band below 0.5, and 0.2 % exactly ``conf_thresh``.
    -> depth [V,H,W] fp32, conf [V,H,W] fp32, cams [V,2,4,4] (CPU)."""
    g = torch.Generator().manual_seed(seed)
    s = 0.01 if metres else 1.0
    cams = make_cameras(V, H, W, baseline=40.0 * s if metres else 30.0, rot_deg=rot_deg, seed=seed)[0]
    z0, a, b = (700.0 if metres else 650.0) * s, 0.2, -0.12                        # plane z = z0 + a x + b y (world = camera 0)
    lo = torch.tensor([-90.0, -60.0, 440.0 if not metres else 270.0], dtype=torch.float64) * s   # the box
    hi = torch.tensor([60.0, 80.0, 520.0 if not metres else 350.0], dtype=torch.float64) * s
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)                           # [H,W,3]
    depths = []
    for v in range(V):
        E, K = cams[v, 0].double(), cams[v, 1, :3, :3].double()
        R, t = E[:3, :3], E[:3, 3]
        C = -R.t() @ t
        d = pix @ torch.linalg.inv(K).t() @ R                                      # world ray per pixel, camera depth = ray parameter
        sp = (-z0 - a * C[0] - b * C[1] + C[2]) / (a * d[..., 0] + b * d[..., 1] - d[..., 2])
        t1, t2 = (lo - C) / d, (hi - C) / d
        tmin, tmax = torch.minimum(t1, t2).amax(-1), torch.maximum(t1, t2).amin(-1)
        hit = (tmax >= tmin) & (tmin > 0)
        depths.append(torch.where(hit & (tmin < sp), tmin, sp))
    d = torch.stack(depths).float()
    d = d * (1 + 0.0008 * torch.randn(d.shape, generator=g))
    d = torch.where(torch.rand(d.shape, generator=g) < 0.02, d * (1 + 0.05 * torch.randn(d.shape, generator=g)), d)
    d[:, :, W - max(1, W // 50):] = 0.0
    d[torch.rand(d.shape, generator=g) < 0.001] = 0.0
    conf = torch.rand(d.shape, generator=g) * 0.45 + 0.55
    conf[:, H // 4:H // 4 + max(1, H // 40), :] *= 0.5
    conf[torch.rand(d.shape, generator=g) < 0.002] = conf_thresh
    return {"depth": d.contiguous(), "conf": conf.contiguous(), "cams": cams.contiguous()}


def _rotmat2qvec(R):
    """Unit quaternion (w, x, y, z) of rotation matrices [..., 3, 3] (w >= 0)."""
    import numpy as np
    R = np.asarray(R, np.float64)
    w = np.sqrt(np.maximum(0.0, 1 + R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2])) / 2
    x = np.copysign(np.sqrt(np.maximum(0.0, 1 + R[..., 0, 0] - R[..., 1, 1] - R[..., 2, 2])) / 2, R[..., 2, 1] - R[..., 1, 2])
    y = np.copysign(np.sqrt(np.maximum(0.0, 1 - R[..., 0, 0] + R[..., 1, 1] - R[..., 2, 2])) / 2, R[..., 0, 2] - R[..., 2, 0])
    z = np.copysign(np.sqrt(np.maximum(0.0, 1 - R[..., 0, 0] - R[..., 1, 1] + R[..., 2, 2])) / 2, R[..., 1, 0] - R[..., 0, 1])
    q = np.stack([w, x, y, z], -1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_colmap_model(n_images: int, n_points: int, *, seed: int = 0, layout: str = "ring", window: Optional[int] = None,
                      min_track: int = 2, max_track: int = 60, tail: float = 1.3, duplicates: float = 0.0, invalid: float = 0.0,
                      camera_models: Tuple[str, ...] = ("PINHOLE",), width: int = 640, height: int = 480, shared_camera: bool = False):
    """A seeded synthetic COLMAP model (mvsformerplusplus_amd.colmap.Model) for tests and measurements.

    Cameras sit on a ring (`layout="ring"`, looking at the origin) or a 2-D grid (`"grid"`, looking down); points lie on a wavy
    surface around the origin.  Track lengths are heavy-tailed: min_track + floor(Lomax(tail) * 2), clipped to
    [min_track, min(max_track, n_images)].  A track is a run of consecutive images along the camera order starting at a random
    image (`window=None`: any start; else the start lies within `window` images of the point's nearest camera; runs wrap
    around), so far-apart images share nothing; point k < n_images starts at image k.  `duplicates` / `invalid`: fractions of extra observations that repeat one of the image's
    points / carry point id -1.  Image and point ids are unique but not consecutive; names are not in id order."""
    import numpy as np
    from . import colmap
    g = np.random.default_rng(seed)
    n, p = int(n_images), int(n_points)
    # cameras
    if layout == "ring":
        a = 2 * np.pi * np.arange(n) / n + g.uniform(-0.2, 0.2, n) * (2 * np.pi / max(n, 1))
        C = np.stack([6 * np.cos(a), g.uniform(-0.5, 0.5, n), 6 * np.sin(a)], 1)
        up = np.array([0.0, 1.0, 0.0])
    elif layout == "grid":
        side = int(np.ceil(np.sqrt(n)))
        gx, gy = np.arange(n) % side, np.arange(n) // side
        C = np.stack([(gx - side / 2) * 0.8, (gy - side / 2) * 0.8, np.full(n, -6.0)], 1) + g.uniform(-0.1, 0.1, (n, 3))
        up = np.array([0.0, 1.0, 0.0])
    else:
        raise ValueError("layout must be 'ring' or 'grid'")
    target = g.uniform(-0.3, 0.3, (n, 3))
    if layout == "grid":
        target[:, :2] += C[:, :2]
        target[:, 2] = 0.0
    zax = target - C
    zax /= np.linalg.norm(zax, axis=1, keepdims=True)
    xax = np.cross(np.broadcast_to(up, zax.shape), zax)
    xax /= np.linalg.norm(xax, axis=1, keepdims=True)
    yax = np.cross(zax, xax)
    q = _rotmat2qvec(np.stack([xax, yax, zax], 1))
    R = colmap.qvec2rotmat(q)
    t = -np.einsum("nij,nj->ni", R, C)
    # points on a wavy surface
    u, v = g.uniform(-1, 1, p), g.uniform(-1, 1, p)
    if layout == "ring":
        xyz = np.stack([2 * u, 1.5 * v, 0.3 * np.sin(3 * u) * np.cos(2 * v)], 1)
    else:
        side = int(np.ceil(np.sqrt(n)))
        xyz = np.stack([u * side * 0.45, v * side * 0.45, 0.5 * np.sin(2 * u) * np.cos(3 * v)], 1)
    # tracks: runs of consecutive images
    L = min_track + np.floor(g.pareto(tail, p) * 2).astype(np.int64)
    L = np.clip(L, min_track, min(max_track, n))
    if window is None:
        start = g.integers(0, n, p)
    else:
        near = np.argmin(((xyz[:, None, :] - C[None, :, :]) ** 2).sum(-1), 1) if p * n <= 5e7 else g.integers(0, n, p)
        start = near + g.integers(-window, window + 1, p)
    start[:min(n, p)] = np.arange(min(n, p))                       # every image starts one track
    tptr = np.zeros(p + 1, np.int64)
    np.cumsum(L, out=tptr[1:])
    t_pt = np.repeat(np.arange(p), L)
    t_img = (np.repeat(start, L) + np.arange(tptr[-1]) - np.repeat(tptr[:-1], L)) % n
    # observations per image: the track entries, plus duplicates and -1 entries, shuffled within each image
    extra_d = int(round(duplicates * len(t_pt)))
    if extra_d:
        k = g.integers(0, len(t_pt), extra_d)
        t_pt, t_img = np.concatenate([t_pt, t_pt[k]]), np.concatenate([t_img, t_img[k]])
    pid_dense = t_pt.astype(np.int64)
    o_img = t_img.astype(np.int64)
    extra_i = int(round(invalid * len(o_img)))
    if extra_i:
        pid_dense = np.concatenate([pid_dense, np.full(extra_i, -1)])
        o_img = np.concatenate([o_img, g.integers(0, n, extra_i)])
    order = np.lexsort((g.random(len(o_img)), o_img))
    o_img, pid_dense = o_img[order], pid_dense[order]
    counts = np.bincount(o_img, minlength=n)
    optr = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=optr[1:])
    p2d = np.arange(len(o_img)) - optr[o_img]                    # POINT2D_IDX within its image
    img_ids = g.permutation(np.arange(1, 3 * n + 1))[:n].astype(np.int64)
    pt_ids = g.permutation(np.arange(1, 3 * p + 1))[:p].astype(np.int64)
    names = ["view_%05d.jpg" % k for k in g.permutation(n)]
    cams, cam_ids = {}, np.zeros(n, np.int64)
    for k in range(1 if shared_camera else n):
        mname = camera_models[k % len(camera_models)]
        spec = colmap.PARAM_TYPE[mname]
        f = 500.0 + g.uniform(-20, 20)
        vals = {"f": f, "fx": f, "fy": f * (1 + g.uniform(-0.02, 0.02)), "cx": width / 2 + g.uniform(-5, 5),
                "cy": height / 2 + g.uniform(-5, 5)}
        params = np.array([vals.get(s, g.uniform(-0.05, 0.05)) for s in spec], np.float64)
        cams[k + 1] = colmap.Camera(k + 1, mname, width, height, params)
    cam_ids[:] = 1 if shared_camera else np.arange(1, n + 1)
    xys = np.stack([g.uniform(0, width, len(o_img)), g.uniform(0, height, len(o_img))], 1)
    images = colmap.Images(img_ids, q, t, cam_ids, names, optr, xys, np.where(pid_dense >= 0, pt_ids[np.maximum(pid_dense, 0)], -1))
    # points3D tracks: every observation of the point (duplicates included), grouped by point
    valid = np.nonzero(pid_dense >= 0)[0]
    by_pt = valid[np.argsort(pid_dense[valid], kind="stable")]
    tl = np.bincount(pid_dense[valid], minlength=p)
    pptr = np.zeros(p + 1, np.int64)
    np.cumsum(tl, out=pptr[1:])
    points = colmap.Points3D(pt_ids, xyz, g.integers(0, 256, (p, 3)).astype(np.uint8), g.uniform(0, 2, p), pptr,
                             img_ids[o_img[by_pt]].astype(np.int32), p2d[by_pt].astype(np.int32))
    return colmap.Model(cams, images, points)
