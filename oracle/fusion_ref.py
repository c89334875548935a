"""CPU restatement (torch, fp32) of the reference's depth-map filtering step - TEST INFRASTRUCTURE,
never imported by the product path.  Follows misc/fusion.py (Vis-MVSNet's filters as vendored by the reference) and the
two drivers in test.py op for op; every function cites the lines it restates.  Device-agnostic (the reference hard-codes
``.cuda()`` in get_pixel_grids, fusion.py:8-13)."""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn.functional as F


def get_pixel_grids(height: int, width: int, dtype=torch.float32) -> torch.Tensor:  # fusion.py:8-13   -> [h,w,3,1], pixel centres
    x = (torch.arange(width, dtype=dtype) + 0.5).repeat(height, 1)
    y = (torch.arange(height, dtype=dtype) + 0.5).repeat(width, 1).t()
    return torch.stack([x, y, torch.ones_like(x)], dim=-1).unsqueeze(-1)


def bin_op_reduce(lst: List, func):                                                 # fusion.py:16-20
    r = lst[0]
    for t in lst[1:]:
        r = func(r, t)
    return r


def idx_img2cam(idx_img_homo, depth, cam):                                           # fusion.py:23-28
    idx_cam = cam[:, 1:2, :3, :3].unsqueeze(1).inverse() @ idx_img_homo
    idx_cam = idx_cam / (idx_cam[..., -1:, :] + 1e-9) * depth.permute(0, 2, 3, 1).unsqueeze(4)
    return torch.cat([idx_cam, torch.ones_like(idx_cam[..., -1:, :])], dim=-2)


def idx_cam2world(idx_cam_homo, cam):                                                # fusion.py:31-34
    w = cam[:, 0:1, ...].unsqueeze(1).inverse() @ idx_cam_homo
    return w / (w[..., -1:, :] + 1e-9)


def idx_world2cam(idx_world_homo, cam):                                              # fusion.py:37-40
    c = cam[:, 0:1, ...].unsqueeze(1) @ idx_world_homo
    return c / (c[..., -1:, :] + 1e-9)


def idx_cam2img(idx_cam_homo, cam):                                                  # fusion.py:43-47
    idx_cam = idx_cam_homo[..., :3, :] / (idx_cam_homo[..., 3:4, :] + 1e-9)
    img = cam[:, 1:2, :3, :3].unsqueeze(1) @ idx_cam
    return img / (img[..., -1:, :] + 1e-9)


def project_warp(dst_depth, src_cam, dst_cam, height, width):                       # fusion.py:52-58  -> [N,h,w,2] clamped grid
    dst_idx_img = get_pixel_grids(height, width, dst_depth.dtype).unsqueeze(0)
    dst2src = idx_cam2img(idx_world2cam(idx_cam2world(idx_img2cam(dst_idx_img, dst_depth, dst_cam), dst_cam), src_cam), src_cam)
    warp = dst2src[..., :2, 0].clone()
    warp[..., 0] /= width
    warp[..., 1] /= height
    return (warp * 2 - 1).clamp(-1.1, 1.1)


def project_img(src_img, dst_depth, src_cam, dst_cam):                               # fusion.py:50-66
    height, width = src_img.shape[-2:]
    warp = project_warp(dst_depth, src_cam, dst_cam, height, width)
    in_range = bin_op_reduce([-1 <= warp[..., 0], warp[..., 0] <= 1, -1 <= warp[..., 1], warp[..., 1] <= 1], torch.min).to(src_img.dtype).unsqueeze(1)
    return F.grid_sample(src_img, warp, mode="bilinear", padding_mode="zeros", align_corners=True), in_range


def source_xyd(sd, sc, rc):                                                          # fusion.py:87-91  [N,1,h,w] -> [N,3,h,w]
    idx_img = get_pixel_grids(*sd.shape[-2:], dtype=sd.dtype).unsqueeze(0)
    s2r_cam = idx_world2cam(idx_cam2world(idx_img2cam(idx_img, sd, sc), sc), rc)
    s2r_img = idx_cam2img(s2r_cam, rc)
    return torch.cat([s2r_img[..., :2, 0], s2r_cam[..., 2:3, 0]], dim=-1).permute(0, 3, 1, 2)


def get_reproj(ref_depth, srcs_depth, ref_cam, srcs_cam):                            # fusion.py:80-97   n1hw, nv1hw -> nv3hw, nv1hw
    n, v, _, h, w = srcs_depth.shape
    sd = srcs_depth.reshape(n * v, 1, h, w)
    sc = srcs_cam.reshape(n * v, 2, 4, 4)
    rd = ref_depth.unsqueeze(1).repeat(1, v, 1, 1, 1).reshape(n * v, 1, h, w)
    rc = ref_cam.unsqueeze(1).repeat(1, v, 1, 1, 1).reshape(n * v, 2, 4, 4)
    s2r_xyd = source_xyd(sd, sc, rc)
    xyd, in_range = project_img(s2r_xyd, rd, sc, rc)
    return xyd.reshape(n, v, 3, h, w), in_range.reshape(n, v, 1, h, w)


def vis_filter(ref_depth, reproj_xyd, in_range, img_dist_thresh, depth_thresh, vthresh):      # fusion.py:100-109
    n, v, _, h, w = reproj_xyd.shape
    xy = get_pixel_grids(h, w, reproj_xyd.dtype).permute(3, 2, 0, 1).unsqueeze(1)[:, :, :2]
    dist_masks = (reproj_xyd[:, :, :2] - xy).norm(dim=2, keepdim=True) < img_dist_thresh
    depth_masks = (ref_depth.unsqueeze(1) - reproj_xyd[:, :, 2:]).abs() < (torch.max(ref_depth.unsqueeze(1), reproj_xyd[:, :, 2:]) * depth_thresh)
    masks = bin_op_reduce([in_range, dist_masks.to(ref_depth.dtype), depth_masks.to(ref_depth.dtype)], torch.min)
    mask = masks.sum(dim=1) >= (vthresh - 1.1)
    return masks, mask


def ave_fusion(ref_depth, reproj_xyd, masks):                                         # fusion.py:112-114
    return ((reproj_xyd[:, :, 2:] * masks).sum(dim=1) + ref_depth) / (masks.sum(dim=1) + 1)


def get_reproj_dynamic(ref_depth, srcs_depth, ref_cam, srcs_cam):                     # fusion.py:116-153
    n, v, _, h, w = srcs_depth.shape
    sd = srcs_depth.reshape(n * v, 1, h, w)
    sc = srcs_cam.reshape(n * v, 2, 4, 4)
    rc = ref_cam.unsqueeze(1).repeat(1, v, 1, 1, 1).reshape(n * v, 2, 4, 4)
    rd = ref_depth.unsqueeze(1).repeat(1, v, 1, 1, 1).reshape(n * v, 1, h, w)
    idx_img = get_pixel_grids(h, w, srcs_depth.dtype).unsqueeze(0)
    r2s_img = idx_cam2img(idx_world2cam(idx_cam2world(idx_img2cam(idx_img, rd, rc), rc), sc), sc)
    warp = r2s_img[..., :2, 0]
    grid = torch.stack((warp[..., 0] / ((w - 1) / 2) - 1, warp[..., 1] / ((h - 1) / 2) - 1), dim=-1)
    warped = F.grid_sample(sd, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    homo = torch.cat([warp, torch.ones_like(warp[..., -1:])], dim=-1).unsqueeze(-1)
    s2r_cam = idx_world2cam(idx_cam2world(idx_img2cam(homo, warped, sc), sc), rc)
    reproj_depth = s2r_cam[:, :, :, 2, 0].clone()
    s2r_img = idx_cam2img(s2r_cam, rc)
    xyd = torch.cat([s2r_img[..., :2, 0], reproj_depth.unsqueeze(-1)], dim=-1).permute(0, 3, 1, 2)
    return xyd.reshape(n, v, 3, h, w)


def ladder(v, base, dtype=torch.float32):                                             # fusion.py:161-162  -> i / base, i = 2 .. v
    return torch.arange(2, v + 1, dtype=dtype) / base


def vis_filter_dynamic(ref_depth, reproj_xyd, dist_base=4, rel_diff_base=1300):       # fusion.py:156-168
    n, v, _, h, w = reproj_xyd.shape
    xy = get_pixel_grids(h, w, reproj_xyd.dtype).permute(3, 2, 0, 1).unsqueeze(1)[:, :, :2]
    corrd_diff = (reproj_xyd[:, :, :2] - xy).norm(dim=2, keepdim=True)
    depth_diff = (ref_depth.unsqueeze(1) - reproj_xyd[:, :, 2:]).abs() / ref_depth.unsqueeze(1)
    dist_thred = ladder(v, dist_base, reproj_xyd.dtype).reshape(1, 1, -1, 1, 1).repeat(n, v, 1, 1, 1)
    rel_thred = ladder(v, rel_diff_base, reproj_xyd.dtype).reshape(1, 1, -1, 1, 1).repeat(n, v, 1, 1, 1)
    masks = torch.min(corrd_diff < dist_thred, depth_diff < rel_thred)
    return masks, masks[:, :, -1:]


def backproject(depth, cam):                                                          # test.py:407-409 / 481-483 -> [n,3,h,w] world points
    idx_img = get_pixel_grids(*depth.shape[-2:], dtype=depth.dtype).unsqueeze(0)
    return idx_cam2world(idx_img2cam(idx_img, depth, cam), cam)[..., :3, 0].permute(0, 3, 1, 2)


def filter_depth(ref_depth, ref_conf, srcs_depth, srcs_conf, ref_cam, srcs_cam, *, conf_thresh, thres_disp, thres_view,
                 depth_thresh=0.01) -> Dict[str, torch.Tensor]:
    """Static filter of one reference view, test.py:388-409 ("pcd")."""
    srcs_depth = srcs_depth.clone()
    for i in range(srcs_depth.shape[1]):
        srcs_depth[:, i] *= (srcs_conf[:, i] > conf_thresh).float().unsqueeze(1)
    prob_mask = ref_conf > conf_thresh
    xyd, in_range = get_reproj(ref_depth, srcs_depth, ref_cam, srcs_cam)
    vis_masks, vis_mask = vis_filter(ref_depth, xyd, in_range, thres_disp, depth_thresh, thres_view)
    ave = ave_fusion(ref_depth, xyd, vis_masks)
    mask = bin_op_reduce([prob_mask.reshape(vis_mask.shape), vis_mask], torch.min)
    return {"reproj_xyd": xyd, "in_range": in_range, "vis_masks": vis_masks, "geo_mask": vis_mask, "depth": ave, "mask": mask,
            "points": backproject(ave, ref_cam)}


def dynamic_fuse(ref_depth, xyd, vis_masks, vis_mask):                                # test.py:466-474 -> averaged depth, geo mask
    dy_range = xyd.shape[1] + 1
    reproj_depth = xyd[:, :, -1].clone()
    reproj_depth[~vis_mask.squeeze(2)] = 0
    geo_mask_sums = vis_masks.sum(dim=1)
    geo_mask_sum = vis_mask.sum(dim=1)
    ave = (torch.sum(reproj_depth, dim=1, keepdim=True) + ref_depth) / (geo_mask_sum + 1)
    geo_mask = geo_mask_sum >= dy_range
    for i in range(2, dy_range):
        geo_mask = torch.logical_or(geo_mask, geo_mask_sums[:, i - 2] >= i)
    return ave, geo_mask


def dynamic_filter_depth(ref_depth, ref_conf, srcs_depth, ref_cam, srcs_cam, *, conf_thresh, dist_base=4, rel_diff_base=1300) -> Dict[str, torch.Tensor]:
    """Dynamic-consistency filter of one reference view, test.py:455-483 ("dpcd")."""
    prob_mask = ref_conf > conf_thresh
    xyd = get_reproj_dynamic(ref_depth, srcs_depth, ref_cam, srcs_cam)
    vis_masks, vis_mask = vis_filter_dynamic(ref_depth, xyd, dist_base, rel_diff_base)
    ave, geo_mask = dynamic_fuse(ref_depth, xyd, vis_masks, vis_mask)
    mask = bin_op_reduce([prob_mask.reshape(geo_mask.shape), geo_mask], torch.min)
    return {"reproj_xyd": xyd, "vis_masks": vis_masks, "geo_mask": geo_mask, "depth": ave, "mask": mask, "points": backproject(ave, ref_cam)}


def tap_sensitivity(img, ix, iy, ulps: float = 4.0):
    """How much a bilinear sample of img [C,h,w] (zero padding) at pixel coordinates (ix, iy) [h',w'] moves when the sample
    position moves by `ulps` fp32 ulps (of the coordinate and of the normalised grid it is computed from).  -> [C,h',w'].
    The slope bound is the largest tap difference of the cell the sample lies in, and of a neighbouring cell when the sample
    lies that close to its edge.  Large next to a zero-depth tap (its value is far from its neighbours) when the weight of
    that tap is about as small as the coordinate's rounding."""
    C, h, w = img.shape
    p = F.pad(img, (2, 2, 2, 2))                                                  # node (x, y) at p[:, y + 2, x + 2]
    ex = (p[:, :, 1:] - p[:, :, :-1]).abs()                                       # edge (x, x+1) on row y at [y+2, x+2]
    ey = (p[:, 1:, :] - p[:, :-1, :]).abs()
    sx = torch.maximum(ex[:, :-1, :], ex[:, 1:, :])                               # cell (x..x+1, y..y+1) at [y+2, x+2]
    sy = torch.maximum(ey[:, :, :-1], ey[:, :, 1:])
    f32 = lambda t: t.to(torch.float32)
    ulp = lambda t: (torch.nextafter(f32(t), torch.tensor(float("inf"))) - f32(t)).to(t.dtype).abs()
    ok = torch.isfinite(ix) & torch.isfinite(iy)
    ixc = ix.where(ok, torch.zeros_like(ix)).clamp(-1.5, w + 0.5)
    iyc = iy.where(ok, torch.zeros_like(iy)).clamp(-1.5, h + 0.5)
    dx = ulps * (ulp(ixc) + (w - 1) / 2 * ulp(ixc / ((w - 1) / 2) - 1))
    dy = ulps * (ulp(iyc) + (h - 1) / 2 * ulp(iyc / ((h - 1) / 2) - 1))
    x0, y0 = ixc.floor(), iyc.floor()
    fx, fy = ixc - x0, iyc - y0
    x0, y0 = x0.long(), y0.long()
    out = torch.zeros((C,) + ix.shape, dtype=img.dtype)
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            use = torch.ones_like(ok)
            if ox == -1: use = use & (fx < dx)
            if ox == 1: use = use & (1 - fx < dx)
            if oy == -1: use = use & (fy < dy)
            if oy == 1: use = use & (1 - fy < dy)
            cx = (x0 + ox + 2).clamp(0, sx.shape[2] - 1)
            cy = (y0 + oy + 2).clamp(0, sx.shape[1] - 1)
            cxy = (x0 + ox + 2).clamp(0, sy.shape[2] - 1)
            cyy = (y0 + oy + 2).clamp(0, sy.shape[1] - 1)
            v = sx[:, cy, cx] * dx + sy[:, cyy, cxy] * dy
            out = torch.maximum(out, torch.where(use, v, torch.zeros_like(v)))
    return torch.where(ok, out, torch.full_like(out, float("inf")))


def near_zero(img, ix, iy, edge: float = 1e-3):
    """Is a zero of img [h,w] (a hole, or the zero padding of a cell across the image border) among the taps of the bilinear
    sample at pixel coordinates (ix, iy), or of a neighbouring cell when the sample lies within `edge` px of that cell?
    -> bool [h',w'] (True where the coordinate is not finite)."""
    h, w = img.shape
    z = F.pad((img == 0).to(img.dtype)[None, None], (2, 2, 2, 2), value=0.0)
    cell = F.max_pool2d(z, 2, 1)[0, 0]                                           # cell (x..x+1, y..y+1) at [y + 2, x + 2]
    cell[1, :] = cell[h + 1, :] = 1.0                                            # cells across the image border: half zero padding
    cell[:, 1] = cell[:, w + 1] = 1.0                                            # (cells wholly outside sample a constant 0)
    ok = torch.isfinite(ix) & torch.isfinite(iy)
    ixc = ix.where(ok, torch.zeros_like(ix)).clamp(-1.5, w + 0.5)
    iyc = iy.where(ok, torch.zeros_like(iy)).clamp(-1.5, h + 0.5)
    x0, y0 = ixc.floor(), iyc.floor()
    fx, fy = ixc - x0, iyc - y0
    x0, y0 = x0.long(), y0.long()
    out = torch.zeros_like(ok)
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            use = ok.clone()
            if ox == -1: use &= fx < edge
            if ox == 1: use &= 1 - fx < edge
            if oy == -1: use &= fy < edge
            if oy == 1: use &= 1 - fy < edge
            out |= use & (cell[(y0 + oy + 2).clamp(0, cell.shape[0] - 1), (x0 + ox + 2).clamp(0, cell.shape[1] - 1)] > 0)
    return out | ~ok


def view_quantities(ref_depth, src_depth, ref_cam, src_cam, *, dynamic: bool, depth_thresh: float = 0.01) -> Dict[str, torch.Tensor]:
    """What the filters compare with their thresholds, for ONE source view of ONE reference view, in the inputs' dtype (run it
    in float64 for a high-precision reference; one view at a time keeps the peak memory of a 1152x1600 image at a few hundred MB).
    ref_depth [1,1,h,w]; src_depth [1,1,1,h,w] (static: already gated by its confidence, test.py:389-392); cameras [1,2,4,4] /
    [1,1,2,4,4].  -> [h,w] maps: x, y, z (the reprojection, get_reproj* restated above) and dist (|xy - pixel centre|);
    static: gx, gy (the clamped grid whose [-1, 1] box is in_range, fusion.py:57-59) and dmargin = |ref - z| - max(ref, z) *
    depth_thresh (the depth test passes below 0, fusion.py:105); dynamic: ddiff = |ref - z| / ref (fusion.py:159).
    sx, sy, sz: tap_sensitivity of x, y, z (dynamic: of the sampled source depth, carried through the back-projection);
    hole: near_zero of the sampled source depth."""
    h, w = ref_depth.shape[-2:]
    if dynamic:
        xyd = get_reproj_dynamic(ref_depth, src_depth, ref_cam, src_cam)
    else:
        xyd, _ = get_reproj(ref_depth, src_depth, ref_cam, src_cam)
    x, y, z = xyd[0, 0, 0], xyd[0, 0, 1], xyd[0, 0, 2]
    xy = get_pixel_grids(h, w, xyd.dtype)[..., :2, 0]
    out = {"x": x, "y": y, "z": z, "dist": (xyd[0, 0, :2] - xy.permute(2, 0, 1)).norm(dim=0)}
    rd = ref_depth[0, 0]
    if dynamic:
        out["ddiff"] = (rd - z).abs() / rd
        r2s = idx_cam2img(idx_world2cam(idx_cam2world(idx_img2cam(get_pixel_grids(h, w, rd.dtype).unsqueeze(0), ref_depth, ref_cam),
                                                      ref_cam), src_cam[:, 0]), src_cam[:, 0])[0, ..., :2, 0]
        sd = src_depth[0, 0]
        s_wd = tap_sensitivity(sd, r2s[..., 0], r2s[..., 1])[0]
        out["hole"] = near_zero(sd[0], r2s[..., 0], r2s[..., 1])
        # d(x, y, z) / d(sampled depth) by one absolute step added to the whole source map (x, y, z are affine in the sampled
        # depth along the source ray, holes included: a zero sample lifts to the camera centre); the sample moves by the step
        # times the in-image weight (1 inside the image)
        step = 1e-6 * float(sd.abs().max().clamp_min(1e-30))
        xyd2 = get_reproj_dynamic(ref_depth, src_depth + step, ref_cam, src_cam)[0, 0]
        for k, c in zip(("sx", "sy", "sz"), range(3)):
            out[k] = (xyd2[c] - xyd[0, 0, c]).abs() / step * s_wd
    else:
        warp = project_warp(ref_depth, src_cam[:, 0], ref_cam, h, w)[0]
        out["gx"], out["gy"] = warp[..., 0], warp[..., 1]
        out["dmargin"] = (rd - z).abs() - torch.max(rd, z) * depth_thresh
        ix, iy = (warp[..., 0] + 1) / 2 * (w - 1), (warp[..., 1] + 1) / 2 * (h - 1)
        s = tap_sensitivity(source_xyd(src_depth[:, 0], src_cam[:, 0], ref_cam)[0], ix, iy)
        out["hole"] = near_zero(src_depth[0, 0, 0], ix, iy)
        out["sx"], out["sy"], out["sz"] = s[0], s[1], s[2]
    return out
