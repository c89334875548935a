"""Camera rigs beyond synth.make_cameras for the warp / gather parity cases (parity_cases.case_*_rigs), and the fp64 reference
(tests/warp_ref.py) of each, computed once per (rig, shape) and shared.

Conventions: cams[v] = [E (world -> camera), K] like make_cameras; feature size H x W; f = 2892.33 * W / 1600, c = (W/2, H/2); the
reference view is the identity at the origin; `s` is the scene scale; hypotheses are linspace(930, 430, D) * s * (1 + 0.03 * rand)
per pixel.  orbit(yaw, pitch, roll): R = Rz(roll) Rx(pitch) Ry(yaw), centre C = T - R^T (0, 0, 650 s) with T = (0, 0, 650 s) - the
camera keeps looking at the point 650 s in front of the reference.

Every condition a rig has to meet (in-image share, behind-the-camera share, excluded share, LDS windows on both sides of their
capacity) is asserted HERE from the fp64 restatement alone, before any kernel runs."""
import functools
import math

import torch

import warp_ref as R64
from oracle import ref_path as O

SHAPES = ((16, 8, 24, 40), (8, 4, 20, 70), (32, 16, 9, 24), (64, 32, 8, 16))      # (C, D, H, W): every chunk geometry and octet count
G = 8


def _rx(deg):
    a = math.radians(deg)
    return torch.tensor([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]], dtype=torch.float64)


def _ry(deg):
    a = math.radians(deg)
    return torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float64)


def _rz(deg):
    a = math.radians(deg)
    return torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]], dtype=torch.float64)


def _orbit(yaw, pitch, roll, s):
    Rm = _rz(roll) @ _rx(pitch) @ _ry(yaw)
    T = torch.tensor([0.0, 0.0, 650.0 * s], dtype=torch.float64)
    return Rm, T - Rm.t() @ T


def _vec(x, y, z, s):
    return torch.tensor([x, y, z], dtype=torch.float64) * s


def sources(name, s=1.0, zoom=2.0, forward_z=600.0):
    """-> list of (R, centre, focal factor, principal-point offset) of the source views of rig `name`."""
    if name == "roll90":
        return [_orbit(5, 0, 90, s) + (1.0, (0.0, 0.0)), _orbit(-4, 3, -90, s) + (1.0, (0.0, 0.0))]
    if name == "convergent":
        return [_orbit(35, 0, 0, s) + (1.0, (0.0, 0.0)), _orbit(-25, 15, 10, s) + (1.0, (0.0, 0.0))]
    if name == "forward":      # source 1 sits INSIDE the hypothesis range: planes nearer than 600 s are behind it
        return [(torch.eye(3, dtype=torch.float64), _vec(10, -5, forward_z, s), 1.0, (0.0, 0.0)),
                (_ry(3), _vec(-20, 0, -400, s), 1.0, (0.0, 0.0))]
    if name == "zoom":
        return [(_ry(2), _vec(60, 0, 0, s), zoom, (5.0, -3.0)), (_rx(-2), _vec(-60, 10, 0, s), 0.5, (-4.0, 2.0))]
    raise KeyError(name)


def make_rig(names, H, W, s=1.0, zoom=2.0, far=False, n_views=None, forward_z=600.0):
    """-> cams [V, 2, 4, 4] fp32: the reference view, then the sources of every rig in `names` (a name or a tuple of names)."""
    names = (names,) if isinstance(names, str) else names
    f, cx, cy = 2892.33 * W / 1600.0, W / 2.0, H / 2.0
    views = [(torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 1.0, (0.0, 0.0))]
    for n in names:
        views += sources(n, s, zoom, forward_z)
    views = views[:n_views] if n_views else views
    Tw = torch.eye(4, dtype=torch.float64)     # the world frame of the "far" rigs: rotated, its origin ~60 units from the cameras
    if far:
        Tw[:3, :3] = _ry(40) @ _rx(25)
        Tw[:3, 3] = torch.tensor([30.0, -20.0, 50.0], dtype=torch.float64)
    out = torch.zeros(len(views), 2, 4, 4, dtype=torch.float64)
    for v, (Rm, C, ff, (dx, dy)) in enumerate(views):
        E = torch.eye(4, dtype=torch.float64)
        E[:3, :3] = Rm
        E[:3, 3] = -Rm @ C
        out[v, 0] = E @ torch.linalg.inv(Tw)
        out[v, 1, :3, :3] = torch.tensor([[f * ff, 0, cx + dx], [0, f * ff, cy + dy], [0, 0, 1]], dtype=torch.float64)
    return out.float()


def make_hyp(D, H, W, s, g, B=1):
    return (torch.linspace(930, 430, D)[None, :, None, None] * s * (1 + 0.03 * torch.rand(B, D, H, W, generator=g))).contiguous()


# name -> the rig(s) of each batch element (`elems`), keyword arguments of make_rig (s, zoom, far, n_views) and what the rig is held to
RIGS = {
    "roll90": dict(elems=["roll90"], zero_excluded=True),
    "convergent": dict(elems=["convergent"], zero_excluded=True),
    "forward": dict(elems=["forward"]),
    "zoom": dict(elems=["zoom"], zero_excluded=True),
    "zoom1.9": dict(elems=["zoom"], zoom=1.9, zero_excluded=True),
    "zoom2.1": dict(elems=["zoom"], zoom=2.1, zero_excluded=True),
    "far-convergent": dict(elems=["convergent"], s=0.01, far=True, zero_excluded=True),
    "far-forward": dict(elems=["forward"], s=0.01, far=True),
    "singular": dict(elems=["forward"], singular=True),
    "mixed": dict(elems=["forward", "roll90"]),
    "roll90-v2": dict(elems=["roll90"], n_views=2, zero_excluded=True),
    "roll90+convergent-v5": dict(elems=[("roll90", "convergent")], zero_excluded=True),
}

# each rig takes two of SHAPES and every shape is used.  "forward" (and what contains it) stays off D = 4: there one whole plane of
# four lies within depth/32 of source 1's camera plane, more than the 10 % the excluded set may hold.  W % 8 != 0 takes the
# direct-gather kernels (make_pair_taps), everything else the LDS-staged ones (make_gtap).  Extra shapes:
#  * zoom1.9 / zoom2.1 at (8, 4, 12, 160) and (16, 8, 16, 192): a tile of the LDS-staged kernels is 64 x 4 pixels at D = 4 and 32 x 4 at
#    D = 8 (lds_window_sizes), and at these sizes one tile's fp32 window of source 1 lies under GL_CAP positions at factor 1.9 and over
#    it at 2.1 - the staged gather on one side, the gather from global memory of gl_unit on the other (rig_conditions asserts it).  At the
#    SHAPES above a x 2 window never comes near the capacity (a 24 x 40 image holds 960 positions): zoom1.9 / zoom2.1 at (16, 8, 24, 40)
#    and (8, 4, 24, 64) are two more focal factors at C = 16 and C = 8, nothing else.
#  * (16, 8, 12, 36): behind-the-camera, singular, far-world, rolled and batched rigs on the direct-gather kernels, D > 4
#  * forward at (32, 8, 12, 32): a second LDS shape on which source 1's entropy is value-checked (from D = 16 on every pixel has an
#    excluded plane)
CAP_EDGE_SHAPES = ((8, 4, 12, 160), (16, 8, 16, 192))
GATHER_CASES = [
    ("roll90", (16, 8, 24, 40)), ("roll90", (64, 32, 8, 16)),
    ("convergent", (8, 4, 20, 70)), ("convergent", (32, 16, 9, 24)),
    ("forward", (16, 8, 24, 40)), ("forward", (32, 16, 9, 24)), ("forward", (32, 8, 12, 32)),
    ("zoom", (16, 8, 24, 40)), ("zoom", (8, 4, 20, 70)),
    ("zoom1.9", (16, 8, 24, 40)), ("zoom1.9", (8, 4, 24, 64)), ("zoom2.1", (16, 8, 24, 40)), ("zoom2.1", (8, 4, 24, 64)),
    ("zoom1.9", (8, 4, 12, 160)), ("zoom1.9", (16, 8, 16, 192)), ("zoom2.1", (8, 4, 12, 160)), ("zoom2.1", (16, 8, 16, 192)),
    ("far-convergent", (32, 16, 9, 24)), ("far-convergent", (16, 8, 24, 40)),
    ("far-forward", (64, 32, 8, 16)), ("far-forward", (16, 8, 24, 40)), ("far-forward", (16, 8, 12, 36)),
    ("singular", (16, 8, 24, 40)), ("singular", (32, 16, 9, 24)), ("singular", (16, 8, 12, 36)),
    ("mixed", (32, 16, 9, 24)), ("mixed", (64, 32, 8, 16)), ("mixed", (16, 8, 12, 36)),
    ("roll90-v2", (32, 16, 9, 24)), ("roll90+convergent-v5", (16, 8, 24, 40)),
]
assert set(SHAPES) <= {s for _, s in GATHER_CASES}
GATHER_IDS = ["%s-%dx%dx%dx%d" % ((n,) + s) for n, s in GATHER_CASES]
BACKWARD_CASES = [(n, s) for n in ("roll90", "convergent", "zoom", "forward") for s in ((8, 4, 12, 20), (32, 6, 10, 16))]
BACKWARD_IDS = ["%s-%dx%dx%dx%d" % ((n,) + s) for n, s in BACKWARD_CASES]


def make_inputs(name, shape, seed=None):
    """-> dict(cams [B,V,2,4,4], hyp [B,D,H,W], feats [B,V,C,H,W], vis [B,V-1,H,W]) fp32 (CPU), random N(0,1) features."""
    C, D, H, W = shape
    spec = RIGS[name]
    s = spec.get("s", 1.0)
    g = torch.Generator().manual_seed(1000 + sum(shape) + len(name) if seed is None else seed)
    cams = torch.stack([make_rig(e, H, W, s=s, zoom=spec.get("zoom", 2.0), far=spec.get("far", False), n_views=spec.get("n_views"))
                        for e in spec["elems"]])
    B, V = cams.shape[:2]
    hyp = make_hyp(D, H, W, s, g, B)
    if spec.get("singular"):       # planes ON source 1's camera plane (pz = 0: the reference divides by 1e-6) and a hair behind it
        hyp[:, 3] = 600.0 * s
        below = torch.nextafter(torch.tensor(600.0 * s), torch.tensor(0.0))
        hyp[:, 4] = torch.where(torch.arange(W) % 2 == 0, torch.tensor(600.0 * s - 1e-6), below)[None, None, :].expand(B, H, W)
    feats = torch.randn(B, V, C, H, W, generator=g)
    vis = torch.rand(B, V - 1, H, W, generator=g) * 0.9 + 0.05
    return {"cams": cams.contiguous(), "hyp": hyp.contiguous(), "feats": feats, "vis": vis}


GL_CAP = 1024        # csrc/gather_lds.h: the capacity of an fp32 LDS window in source positions; a larger one gathers from global memory


def lds_window_sizes(ix, iy):
    """The LDS windows of the LDS-staged gather (csrc/gather_lds.h, gl_unit) from the fp64 pixel coordinates ix, iy [D,H,W] of one
    source view -> n [rounds, tiles y, tiles x] source positions (0: no tap of the tile is inside the image).  A block is a tile of
    TW x 4 pixels, TW = 64 / NS with NS = min(8, largest power of two <= ceil(D / 4)) plane chunks side by side, so one window holds
    the 2 x 2 tap blocks (make_gtap: top-left corner clamped to [0, W-2] x [0, H-2]) of 4 NS planes of the tile; its x origin and
    width are multiples of 8."""
    D, H, W = ix.shape
    nch = (D + 3) // 4
    NS = 8 if nch >= 8 else 4 if nch >= 4 else 2 if nch >= 2 else 1
    TW, TH, DP = 64 // NS, 4, 4 * NS
    sane = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    xb, yb = ix.floor().clamp(0, W - 2).long(), iy.floor().clamp(0, H - 2).long()
    out = torch.zeros((D + DP - 1) // DP, (H + TH - 1) // TH, (W + TW - 1) // TW, dtype=torch.long)
    for it in range(out.shape[0]):
        for ty in range(out.shape[1]):
            for tx in range(out.shape[2]):
                box = (slice(it * DP, (it + 1) * DP), slice(ty * TH, (ty + 1) * TH), slice(tx * TW, (tx + 1) * TW))
                ok = sane[box]
                if not bool(ok.any()):
                    continue
                x, y = xb[box][ok], yb[box][ok]
                wx0 = int(x.min()) & ~7
                ww = (int(x.max()) + 2 - wx0 + 7) & ~7
                out[it, ty, tx] = ww * (int(y.max()) + 2 - int(y.min()))
    return out


def rig_conditions(name, geo, D, planted=(), windows=None):
    """What a rig has to offer, from the fp64 geometry `geo` = {(batch element, source view): (inside the source image, behind the camera,
    excluded from value comparisons) [1,D,H,W]}: at least 5 % of the voxels sample inside the source image; source 1 of "forward" has at
    least 25 % of the voxels behind it and 0.5 % behind it AND inside its image; at most 10 % are excluded (none on the rigs marked
    zero_excluded) - counted without the `planted` planes of the singular rig, which lie on the camera plane on purpose.  zoom1.9 / zoom2.1
    at CAP_EDGE_SHAPES come with `windows` = (lds_window_sizes of source 1 at focal factor 1.9, the same at 2.1): at 1.9 every window fits
    the LDS (the largest within a quarter of GL_CAP), at 2.1 a tile that fitted at 1.9 is over GL_CAP by at most a quarter."""
    spec = RIGS[name]
    if windows is not None:
        under, over = windows
        assert int(under.max()) <= GL_CAP, (name, "a window at factor 1.9 is over the capacity", int(under.max()))
        edge = (under > 0) & (over > GL_CAP)
        assert bool(edge.any()), (name, "no tile crosses the capacity between 1.9 and 2.1", int(under.max()), int(over.max()))
        assert int(under[edge].max()) >= 3 * GL_CAP // 4 and int(over[edge].min()) <= 5 * GL_CAP // 4, (name, under[edge], over[edge])
    for (b, v), (inside, behind, excl) in geo.items():
        rig = spec["elems"][b]
        assert float(inside.double().mean()) >= 0.05, (name, b, v, "share of voxels sampling inside the source image", float(inside.double().mean()))
        if rig == "forward" and v == 1 and not spec.get("singular"):
            assert float(behind.double().mean()) >= 0.25, (name, "share behind source 1", float(behind.double().mean()))
            assert float((behind & inside).double().mean()) >= 0.005, (name, "behind AND inside", float((behind & inside).double().mean()))
        keep = [d for d in range(D) if d not in planted]
        share = float(excl[:, keep].double().mean())
        assert share <= 0.10, (name, b, v, "excluded share", share)
        if spec.get("zero_excluded"):
            assert share == 0.0, (name, b, v, "no voxel of this rig may be excluded", share)


def oracle32(feats, cams, hyp, vis, source=None):
    """The fp32 oracle's aggregation -> (volume [B,G,D,H,W], correlations [B,V-1,G,D,H,W], entropies [B,V-1,H,W], [(warped, mask)] per view);
    `source` as in warp_ref.aggregate64."""
    V = feats.shape[1]
    src = feats if source is None else source
    ref_p = O.compose_proj(cams[:, 0])
    acc, vsum, corr, ent, wps = 0.0, 0.0, [], [], []
    for v in range(1, V):
        w32, m32 = O.homo_warping_3D_with_mask(src[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
        ip = O.group_correlation(feats[:, 0], w32, G)
        corr.append(ip)
        ent.append(O.entropy_of_similarity(ip)[:, 0])
        acc = acc + ip * vis[:, v - 1][:, None, None]
        vsum = vsum + vis[:, v - 1]
        wps.append((w32, m32))
    return acc / (vsum[:, None, None] + 1e-6), torch.stack(corr, 1), torch.stack(ent, 1), wps


@functools.lru_cache(maxsize=None)
def reference(name, shape):
    """The inputs of (rig, shape) and everything the cases compare against, computed once: per source view the fp64 warp (warped, mask,
    ix, iy, pz), correlations, entropies and the aggregated volume - from the fp32 features and from their fp16 rounding (the fp16
    windows of the keeping pass) - and the SAME quantities from the fp32 oracle, whose distance from fp64 sets the comparison bar.
    `inc[b, v-1]` [D,H,W]: voxels that take part in value comparisons (depth / |pz| <= 32 in fp64).  Treat as read-only."""
    inp = make_inputs(name, shape)
    cams, hyp, feats, vis = inp["cams"], inp["hyp"], inp["feats"], inp["vis"]
    B, V, C, H, W = feats.shape
    D = hyp.shape[1]
    spec = RIGS[name]
    hom = R64.homography64(cams)
    f16src = feats.half().float()
    out = dict(inp, hom64=hom, f16src=f16src)
    geo, warps = {}, []
    for v in range(1, V):
        w, m, ix, iy, pz = R64.warp64_hom(feats[:, v], hom[:, v - 1], hyp)
        warps.append(dict(warped=w, mask=m, ix=ix, iy=iy, pz=pz))
        inside = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
        for b in range(B):
            geo[(b, v)] = (inside[b:b + 1], pz[b:b + 1] <= 0, (hyp[b:b + 1].double() > 32 * pz[b:b + 1].abs()))
    windows = None
    if name in ("zoom1.9", "zoom2.1") and shape in CAP_EDGE_SHAPES:           # source 1 at both focal factors, the same hypotheses
        windows = []
        for z in (1.9, 2.1):
            xn, yn, _ = R64.project64(R64.homography64(make_rig(spec["elems"][0], H, W, zoom=z)[None])[:, 0], hyp, H, W)
            windows.append(lds_window_sizes((xn[0] + 1) / 2 * (W - 1), (yn[0] + 1) / 2 * (H - 1)))
    rig_conditions(name, geo, D, planted=(3, 4) if spec.get("singular") else (), windows=windows)
    out["warp"] = warps
    out["inc"] = torch.stack([~(hyp.double() > 32 * w["pz"].abs()) for w in warps], 1)           # [B,V-1,D,H,W]
    out["far_px"] = torch.stack([(w["ix"].abs() > 1e4) | (w["iy"].abs() > 1e4) for w in warps], 1)
    out["vol64"], out["corr64"], out["ent64"] = R64.aggregate64(feats, cams, hyp, vis, G)
    out["vol64_16"], out["corr64_16"], out["ent64_16"] = R64.aggregate64(feats, cams, hyp, vis, G, source=f16src)
    # the fp32 oracle on the same inputs
    out["vol32"], out["corr32"], out["ent32"], out["warp32"] = oracle32(feats, cams, hyp, vis)
    out["vol32_16"], out["corr32_16"], out["ent32_16"], _ = oracle32(feats, cams, hyp, vis, source=f16src)
    return out
