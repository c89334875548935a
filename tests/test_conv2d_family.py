"""CPU: the three users of the 2-D split-bf16 convolution template (csrc/conv2d_split.h) - ops.fpn_conv, ops.fmt_smooth and the
feature emitter ops.conv2d3x3_tiles - are one arithmetic: wherever two entry points compute the same function they return the same
bits.  Plus the case the fixtures cannot reach: stride 2 across a tile seam (F25's maps are at most 96 wide; a tile is 64 columns)."""
import pytest
import torch
import torch.nn.functional as F

from mvsformerplusplus_amd import ops, packing

LAYER_BAR = 3e-5          # per layer: x max(1, max|ref|) (tests/test_fpn.py)
# N = 2; one pixel that is all halo, a partial tile in both directions, three column tiles with interior tile seams
SHAPES = [(1, 1), (5, 67), (9, 130)]


def unpack(t):
    """octet tiles [N, C/8, H, W, 8] -> planar [N, C, H, W]"""
    N, O, H, W, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(N, O * 8, H, W)


def narrow(t, dtype):
    """The emitter's narrowing rule on the host: bf16 rounds to nearest even; fp16 clamps to +-65504, then converts."""
    return t.to(torch.bfloat16) if dtype == torch.bfloat16 else t.clamp(-65504.0, 65504.0).to(torch.float16)


def check_family(H, W, device):
    g = torch.Generator().manual_seed(1000 * H + W)
    for C in (8, 16, 32):
        x = torch.randn(2, C, H, W, generator=g).to(device)
        wp = packing.pack_fpn_conv_weights(torch.randn(C, C, 3, 3, generator=g) * 0.2, 1).to(device)
        smooth = ops.fmt_smooth(x, wp)
        tiles = ops.conv2d3x3_tiles(x, wp, None, C, False, dtype=torch.float32)
        assert torch.equal(smooth, unpack(tiles)), ("fmt_smooth != conv2d3x3_tiles", C, H, W)
        if C > 8:                                                     # fpn_conv has no (8, 8, 3, 1) instance
            assert torch.equal(smooth, ops.fpn_conv(x, wp, None, C, 3, 1, ops.FPN_ACT_NONE)), ("fmt_smooth != fpn_conv", C, H, W)
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(ops.conv2d3x3_tiles(x, wp, None, C, False, dtype=dt), narrow(tiles, dt)), ("emitter narrowing", dt, C, H, W)
    for co in (8, 16, 32):
        # x 3e4: outputs beyond the fp16 range, so that the clamp is on the path (Swish keeps large positive values as they are)
        x = (torch.randn(2, 64, H, W, generator=g) * 3e4).to(device)
        wp = packing.pack_fpn_conv_weights(torch.randn(co, 64, 3, 3, generator=g) * 0.1, 1).to(device)
        bias = torch.randn(co, generator=g).to(device)
        planar = ops.fpn_conv(x, wp, bias, co, 3, 1, ops.FPN_ACT_SWISH)
        tiles = ops.conv2d3x3_tiles(x, wp, bias, co, True, dtype=torch.float32)
        assert torch.equal(planar, unpack(tiles)), ("fpn_conv != conv2d3x3_tiles", co, H, W)
        assert H * W == 1 or float(tiles.max()) > 65504.0
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(ops.conv2d3x3_tiles(x, wp, bias, co, True, dtype=dt), narrow(tiles, dt)), ("emitter narrowing", dt, co, H, W)


@pytest.mark.parametrize("H,W", SHAPES)
def test_entry_points_share_one_arithmetic(emu, H, W):
    check_family(H, W, emu)


@pytest.mark.parametrize("cin,cout,k", [(8, 16, 5), (32, 64, 3)])
def test_stride_2_across_a_tile_seam(emu, cin, cout, k):
    """7 x 131 -> 4 x 66 output pixels: the second column tile starts at output column 64 = input column 128."""
    g = torch.Generator().manual_seed(cin + k)
    x = torch.randn(2, cin, 7, 131, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=g)
    got = ops.fpn_conv(x, packing.pack_fpn_conv_weights(w, 2), bias, cout, k, 2, ops.FPN_ACT_LEAKY)
    want = F.leaky_relu(F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=k // 2), 0.1)
    assert got.shape == want.shape == (2, cout, 4, 66)
    err, lim = float((got.double() - want).abs().max()), LAYER_BAR * max(1.0, float(want.abs().max()))
    print("fpn_conv (%d, %d, %d, 2) at 7 x 131: max |error| %.3g (bar %.3g)" % (cin, cout, k, err, lim))
    assert err <= lim, (err, lim)
