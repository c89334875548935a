"""CPU: the fp64 restatement of the warp / correlation / aggregation (tests/warp_ref.py) pinned to the fp32 oracle - itself pinned to
fixture F1, generated from the reference (tests/test_oracle_golden.py) - at fp32-rounding distance, and to F1 directly."""
import pytest
import torch

import warp_ref as R64
from conftest import load_golden
from mvsformerplusplus_amd import synth
from oracle import ref_path as O


def test_warp_ref_vs_oracle():
    """A make_cameras rig (where the fp32 inverse of the oracle is good): every quantity agrees to fp32 rounding, masks away from the
    frame border are equal, and fp64 autograd agrees with fp32 autograd through the oracle."""
    g = torch.Generator().manual_seed(3)
    B, V, C, D, H, W, G = 2, 3, 16, 6, 12, 20, 8
    cams = synth.make_cameras(V, H * 8, W * 8, baseline=60.0, rot_deg=3.0, seed=1, batch=B)
    cams[:, :, 1, :2, :] /= 8
    feats = torch.randn(B, V, C, H, W, generator=g)
    hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.03 * torch.rand(B, D, H, W, generator=g))).contiguous()
    vis = torch.rand(B, V - 1, H, W, generator=g) * 0.9 + 0.05
    ref_p = O.compose_proj(cams[:, 0])
    P = O.compose_proj(cams.reshape(-1, 2, 4, 4)).reshape(B, V, 4, 4)
    assert (R64.homography64(cams) - torch.matmul(P[:, 1:], torch.inverse(P[:, :1]))).abs().max() <= 1e-3      # entries up to ~4e4
    f64, v64 = feats.double().requires_grad_(True), vis.double().requires_grad_(True)
    f32, v32 = feats.clone().requires_grad_(True), vis.clone().requires_grad_(True)
    vol64, corr64, ent64 = R64.aggregate64(f64, cams, hyp, v64, G)
    acc, vsum = 0.0, 0.0
    for v in range(1, V):
        w32, m32 = O.homo_warping_3D_with_mask(f32[:, v], O.compose_proj(cams[:, v]), ref_p, hyp)
        w64, m64, ix, iy, pz = R64.warp64(feats[:, v], cams, v, hyp)
        assert (w64 - w32.detach()).abs().max() <= 1e-4
        border = ((ix.abs() < 1e-3) | ((ix - (W - 1)).abs() < 1e-3) | (iy.abs() < 1e-3) | ((iy - (H - 1)).abs() < 1e-3))
        assert torch.equal(m64 | border, m32 | border) and 0.02 < float(m64.double().mean()) < 0.98
        assert bool((pz > 0).all())
        ip = O.group_correlation(f32[:, 0], w32, G)
        assert (corr64[:, v - 1] - ip.detach()).abs().max() <= 5e-5
        assert (ent64[:, v - 1] - O.entropy_of_similarity(ip)[:, 0].detach()).abs().max() <= 2e-5
        assert (R64.entropy64(ip.detach()) - O.entropy_of_similarity(ip.detach().double())[:, 0]).abs().max() <= 1e-12
        acc = acc + ip * v32[:, v - 1][:, None, None]
        vsum = vsum + v32[:, v - 1]
    vol32 = acc / (vsum[:, None, None] + 1e-6)
    assert (vol64.detach() - vol32.detach()).abs().max() <= 5e-5
    gv = torch.randn(vol32.shape, generator=g)
    (vol64 * gv.double()).sum().backward()
    (vol32 * gv).sum().backward()
    assert (f64.grad - f32.grad).abs().max() <= 1e-4 * float(f64.grad.abs().max())
    assert (v64.grad - v32.grad).abs().max() <= 1e-4 * float(v64.grad.abs().max())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_warp_ref_f1(tag):
    """Fixture F1 (the reference's own homo_warping_3D_with_mask), [B, D] and [B, D, H, W] hypotheses."""
    fx = load_golden("f1_warp_%s.npz" % tag)
    hom = R64.homography64_from_proj(fx["src_proj"], fx["ref_proj"])
    for dv, wk, mk in (("dv2", "warped2", "mask2"), ("dv4", "warped4", "mask4")):
        w, m, ix, iy, pz = R64.warp64_hom(fx["src_fea"], hom, fx[dv])
        assert (m != fx[mk]).float().mean() <= 2e-3
        assert (w - fx[wk]).abs().max() <= 2e-4 and (w - fx[wk]).abs().mean() <= 2e-6
