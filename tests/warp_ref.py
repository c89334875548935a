"""TEST ORACLE: an fp64 restatement of the reference's homography warp, group-wise correlation, visibility entropy and weighted
aggregation (models/warping.py:69-109, models/cost_volume.py:68-101), from scratch in plain torch.  The fp32 restatement
(oracle/ref_path.py) inverts the reference projection in fp32 like the reference; the kernels invert it in fp64 (warp_kernels.hip,
invert4), so on rigs where the fp32 inverse is poor only an fp64 comparator can tell a better kernel from a wrong one.  Inputs are
the fp32 camera values widened to fp64 and the fp32 hypotheses; everything is differentiable, so fp64 autograd gives the backward
reference.  Pinned to the fp32 oracle (and through it to fixture F1) by tests/test_warp_ref.py."""
import torch
import torch.nn.functional as F


def compose_proj64(cams):
    """cams [..., 2, 4, 4] (0 = extrinsic, 1 = intrinsic) -> P [..., 4, 4] fp64 with P[:3, :4] = K[:3, :3] @ E[:3, :4], P[3] = E[3]
    (cost_volume.py:68-71)."""
    c = cams.double()
    P = c[..., 0, :, :].clone()
    P[..., :3, :4] = c[..., 1, :3, :3] @ c[..., 0, :3, :4]
    return P


def homography64(cams):
    """cams [B, V, 2, 4, 4] -> P_v @ inv(P_0) for every source view, [B, V-1, 4, 4] fp64 (warping.py:80)."""
    P = compose_proj64(cams)
    return P[:, 1:] @ torch.linalg.inv(P[:, :1])


def homography64_from_proj(src_proj, ref_proj):
    """Composed projections [B, 4, 4] -> src @ inv(ref), fp64."""
    return src_proj.double() @ torch.linalg.inv(ref_proj.double())


def project64(hom, hyp, H, W):
    """hom [B, 4, 4] fp64, hyp [B, D] or [B, D, H, W] -> (xn, yn, pz) [B, D, H, W] fp64: the normalised sampling grid and the
    projected depth, statement for statement warping.py:83-95."""
    B, D = hyp.shape[:2]
    hyp = hyp.double()
    rot, trans = hom[:, :3, :3], hom[:, :3, 3:4]
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(H * W, dtype=torch.float64)))[None].repeat(B, 1, 1)     # :88
    rot_xyz = rot @ xyz                                                                                                  # :90
    dv = hyp.reshape(B, 1, D, -1) if hyp.dim() == 4 else hyp.reshape(B, 1, D, 1)
    proj_xyz = rot_xyz.unsqueeze(2) * dv + trans.reshape(B, 3, 1, 1)                                                     # :91-92
    proj_xy = proj_xyz[:, :2] / (proj_xyz[:, 2:3] + 1e-6)                                                                # :93
    xn = proj_xy[:, 0] / ((W - 1) / 2) - 1                                                                               # :94
    yn = proj_xy[:, 1] / ((H - 1) / 2) - 1                                                                               # :95
    return xn.reshape(B, D, H, W), yn.reshape(B, D, H, W), proj_xyz[:, 2].reshape(B, D, H, W)


def warp64_hom(src, hom, hyp):
    """src [B, C, H, W]; hom [B, 4, 4] fp64; hyp [B, D] / [B, D, H, W] -> (warped [B, C, D, H, W] fp64, mask [B, D, H, W] bool,
    ix, iy [B, D, H, W] = the pixel coordinates grid_sample un-normalises to, pz).  warping.py:80-106."""
    B, C, H, W = src.shape
    D = hyp.shape[1]
    xn, yn, pz = project64(hom, hyp, H, W)
    mask = (xn > 1) | (xn < -1) | (yn > 1) | (yn < -1) | (pz <= 0)                                                       # :99-103
    grid = torch.stack((xn, yn), dim=-1).reshape(B, D * H, W, 2)
    warped = F.grid_sample(src.double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)                # :105
    ix = (xn + 1) / 2 * (W - 1)                                                                                          # grid_sampler_unnormalize
    iy = (yn + 1) / 2 * (H - 1)
    return warped.reshape(B, C, D, H, W), mask, ix, iy, pz


def warp64(src, cams, v, hyp):
    """Source view v of the rig `cams` [B, V, 2, 4, 4]: warp64_hom with homography64(cams)[:, v - 1]."""
    return warp64_hom(src, homography64(cams)[:, v - 1], hyp)


def group_correlation64(ref_feat, warped, G):
    """ref_feat [B, C, H, W], warped [B, C, D, H, W] -> [B, G, D, H, W] fp64 (cost_volume.py:74-87)."""
    B, C, D, H, W = warped.shape
    assert G <= C and C % G == 0
    return (ref_feat.double().reshape(B, G, C // G, 1, H, W) * warped.double().reshape(B, G, C // G, D, H, W)).mean(dim=2)


def entropy64(in_prod):
    """[B, G, D, H, W] -> [B, H, W] fp64 (cost_volume.py:90-92)."""
    p = F.softmax(in_prod.double().sum(dim=1), dim=1)
    return (-p * torch.log(p + 1e-7)).sum(dim=1)


def aggregate64(feats, cams, hyp, vis, G, source=None):
    """feats [B, V, C, H, W]; vis [B, V-1, H, W] -> (volume [B, G, D, H, W], per-view correlations [B, V-1, G, D, H, W], entropies
    [B, V-1, H, W]), all fp64 (cost_volume.py:60-101, the `+ 1e-6` denominator).  `source`: the features the SOURCE views are sampled
    from when they differ from `feats` (fp16-rounded windows)."""
    V = feats.shape[1]
    hom = homography64(cams)
    src = feats if source is None else source
    acc, vsum, corr, ent = 0.0, 0.0, [], []
    for v in range(1, V):
        warped = warp64_hom(src[:, v], hom[:, v - 1], hyp)[0]
        ip = group_correlation64(feats[:, 0], warped, G)
        w = vis[:, v - 1].double()
        acc = acc + ip * w[:, None, None]
        vsum = vsum + w
        corr.append(ip)
        ent.append(entropy64(ip))
    return acc / (vsum[:, None, None] + 1e-6), torch.stack(corr, 1), torch.stack(ent, 1)
