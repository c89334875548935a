"""CPU (emulator): the split-bf16 format has ONE definition (csrc/split_format.h) and the cost volume ONE store (csrc/volume_format.h).

* Both device roundings - the hardware convert (split_bf16: the packed-split row store of ops.vitdec_rows) and the integer form
  (split_bf16_bits: the split volume of ops.volume_normalise_) - against their host mirrors (packing.pack_tokens_split, ops.to_split)
  and against each other, bit for bit, on 393 216 fp32 patterns: all 65 536 upper halves x the lower halves 0x0000, 0x0001, 0x7fff,
  0x8000, 0x8001, 0xffff (every exponent's ties and near-ties, subnormals, +-0, +-inf, the round-up into inf).
  NaN patterns are kept out of the equalities: a NaN input must give a NaN hi; the lo of +-inf is bf16(inf - inf), a NaN whose sign
  is the host's or the device's, and must be a NaN.
* volume_store8 through its four kernels (warp_corr_aggregate, corr_aggregate, volume_to_f16, volume_normalise_) in the three volume
  formats: fp16 = the clamped fp16 of the fp32 result, split = to_split of the fp32 result, and the fp16 saturation counter moves only
  when a value left the fp16 range."""
import pytest
import torch

from mvsformerplusplus_amd import ops, packing, synth

LOWER = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)


def patterns():
    """393 216 fp32 values: lower half l of LOWER (outer) x upper half 0 .. 65535 (inner)."""
    hi = torch.arange(65536, dtype=torch.int64) << 16
    bits = torch.cat([hi | l for l in LOWER])
    return (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)


def same_bits(a, b):
    """element-wise: the same bf16 bits, or a NaN on both sides"""
    return (a.view(torch.int16) == b.view(torch.int16)) | (a.isnan() & b.isnan())


def rows_hi_lo(packed, m, c):
    """packed-split [rb][step][hi|lo][g][li][e] (packing.pack_tokens_split) -> (hi, lo) bf16 [m, c]"""
    p = packed.view(torch.bfloat16).reshape(m // 16, c // 32, 2, 4, 16, 8).permute(2, 0, 4, 1, 3, 5).reshape(2, m, c)
    return p[0], p[1]


def octets_hi_lo(split_cl):
    """split activation format [..., 8] fp32 = [hi x8 | lo x8] bf16 per voxel (ops.to_split) -> (hi, lo) bf16 [..., 8]"""
    p = split_cl.contiguous().view(torch.bfloat16).reshape(*split_cl.shape[:-1], 2, 8)
    return p[..., 0, :], p[..., 1, :]


def check_roundings(device):
    x = patterns()
    finite_or_inf = ~x.isnan()
    # ---- the convert form: 512 rows of 768 through the ViT decoder's row pass ----
    got = ops.vitdec_rows(x.reshape(1, 1, 512, 768).to(device), 0, 1, want_x=False, want_packed=True)[1].cpu()
    ch, cl = rows_hi_lo(got, 512, 768)
    wh, wl = rows_hi_lo(packing.pack_tokens_split(x.reshape(512, 768)), 512, 768)
    nan_lo = wl.isnan()
    assert ch.isnan()[~finite_or_inf.reshape(512, 768)].all(), "convert form: the hi of a NaN must be a NaN"
    keep = finite_or_inf.reshape(512, 768)
    assert torch.equal(ch.view(torch.int16)[keep], wh.view(torch.int16)[keep]), "convert form: hi != packing.pack_tokens_split"
    assert torch.equal(cl.view(torch.int16)[keep & ~nan_lo], wl.view(torch.int16)[keep & ~nan_lo]), "convert form: lo != packing.pack_tokens_split"
    assert cl.isnan()[keep & nan_lo].all()
    # ---- the integer form: the same values as a volume [1, 6, 64, 128, 8], normalised by a visibility sum that makes the divisor 1.0 ----
    vsum = torch.full((1, 64, 128), 1.0) - torch.tensor(1e-6)
    assert bool((vsum + torch.tensor(1e-6) == 1.0).all())
    vol = x.reshape(1, 6, 64, 128, 8)
    v32 = ops.volume_normalise_(vol.clone().to(device), vsum.to(device)).cpu()
    vs = ops.volume_normalise_(vol.clone().to(device), vsum.to(device), split=True).cpu()
    keepv = finite_or_inf.reshape(vol.shape)
    assert torch.equal(v32.view(torch.int32)[keepv], vol.view(torch.int32)[keepv]), "x / 1.0 must reach the split unchanged"
    ih, il = octets_hi_lo(vs)
    th, tl = octets_hi_lo(ops.to_split(v32))
    assert ih.isnan()[~keepv].all(), "integer form: the hi of a NaN must be a NaN"
    assert torch.equal(ih.view(torch.int16)[keepv], th.view(torch.int16)[keepv]), "integer form: hi != ops.to_split"
    assert same_bits(il, tl)[keepv].all(), "integer form: lo != ops.to_split"
    assert (il.isnan() == tl.isnan())[keepv].all()
    # ---- both device forms against each other ----
    assert torch.equal(ch.reshape(-1).view(torch.int16)[keep.reshape(-1)], ih.reshape(-1).view(torch.int16)[keep.reshape(-1)]), "convert hi != integer hi"
    assert same_bits(cl.reshape(-1), il.reshape(-1))[keep.reshape(-1)].all(), "convert lo != integer lo"


def clamp_f16(v32):
    return v32.clamp(-65504.0, 65504.0).half()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def check_volume_store(H, W, scale, device):
    """B = 1, V = 3, C = 16, D = 6: the last chunk of four planes is partial.  scale = 1: every value inside the fp16 range; scale > 1: the
    correlations leave it (clamp + saturation counter)."""
    B, V, C, D = 1, 3, 16, 6
    g = torch.Generator().manual_seed(100 * H + W)
    cams = synth.make_cameras(V, H * 8, W * 8, baseline=60.0, rot_deg=2.0, seed=3, batch=B)
    cams[:, :, 1, :2, :] /= 8
    # The fp16 volume's gather is another instantiation than the fp32 volume's: source windows staged as fp16 (MVS_GATHER_F16) and sampled
    # by explicit fmas, where the fp32 form leaves contraction to the compiler.  Features and visibilities that are signed powers of two
    # make the two one arithmetic: nothing is lost in the fp16 window, every product (tap x bilinear weight, reference x sample,
    # correlation x visibility) is exact, and a sum of exact products rounds the same fused or not - so "the clamped fp16 of the fp32
    # result" holds bit for bit for that kernel too, with every pixel, channel and plane still different from its neighbours.
    def pow2(shape, lo, hi):
        return torch.ldexp(torch.ones(shape), torch.randint(lo, hi + 1, shape, generator=g))
    feats = pow2((B, V, C, H, W), -2, 3) * (torch.randint(0, 2, (B, V, C, H, W), generator=g) * 2 - 1) * scale
    hyp = (torch.linspace(900, 450, D)[None, :, None, None] * (1 + 0.03 * torch.rand(B, D, H, W, generator=g))).contiguous().to(device)
    vis = pow2((B, V - 1, H, W), -3, 0).to(device)
    f, code = ops._feat(feats.to(device))
    hom = ops.compose_homography(cams.to(device))
    saturates = scale > 1.0
    counts = {}
    ops.f16_saturation_count(reset=True)

    # ---- gl_aggregate_kernel (LDS-staged shapes) or the direct kernels + the conversions ----
    v32 = ops.warp_corr_aggregate(f, code, hom, hyp, vis, 8)[0].cpu()
    assert bool(float(v32.abs().max()) > 65504.0) == saturates, float(v32.abs().max())
    assert ops.f16_saturation_count(reset=True) == 0, "the fp32 volume counts nothing"
    vsp = ops.warp_corr_aggregate(f, code, hom, hyp, vis, 8, split=True)[0].cpu()
    assert torch.equal(vsp.view(torch.int32), ops.to_split(v32).view(torch.int32)), "warp_corr_aggregate: split volume"
    assert ops.f16_saturation_count(reset=True) == 0, "the split volume counts nothing"
    part, vsum = ops.warp_corr_aggregate(f, code, hom, hyp, vis, 8, normalise=False)
    if ops.gather_is_lds_staged(f, 8, hyp):
        v16 = ops.warp_corr_aggregate(f, code, hom, hyp, vis, 8, f16=True)[0].cpu()
        diff = (v16.float() - clamp_f16(v32).float()).abs().max()
        print("warp_corr_aggregate %dx%d x%g: max |fp16 volume - clamped fp16 of the fp32 volume| = %g" % (H, W, scale, float(diff)))
        assert bits_equal(v16, clamp_f16(v32)), "warp_corr_aggregate: fp16 volume"
        counts["warp_corr_aggregate"] = ops.f16_saturation_count(reset=True)
    else:
        assert W % 8 != 0                                   # the conversion route: fp32 partial volume -> normalised fp16

    # ---- volume_to_f16_kernel / volume_to_split_kernel, with and without the division ----
    n32 = ops.volume_normalise_(part.clone(), vsum).cpu()
    assert bits_equal(ops.volume_to_f16(part, vsum).cpu(), clamp_f16(n32)), "volume_to_f16 (normalising)"
    counts["volume_to_f16 (normalising)"] = ops.f16_saturation_count(reset=True)
    assert bits_equal(ops.volume_to_f16(v32.to(device)).cpu(), clamp_f16(v32)), "volume_to_f16"
    counts["volume_to_f16"] = ops.f16_saturation_count(reset=True)
    nsp = ops.volume_normalise_(part.clone(), vsum, split=True).cpu()
    assert torch.equal(nsp.view(torch.int32), ops.to_split(n32).view(torch.int32)), "volume_normalise_: split volume"
    assert ops.f16_saturation_count(reset=True) == 0

    # ---- corr_aggregate_kernel: kept correlations in fp16 (always inside the range) and in fp32 ----
    corr32 = torch.randn(B, V - 1, D, H, W, 8, generator=g) * (1e5 if saturates else 1.0)
    for corr, name in ((corr32.to(device), "corr_aggregate (fp32 correlations)"), (corr32.clamp(-6e4, 6e4).half().to(device), "corr_aggregate (fp16 correlations)")):
        c32 = ops.corr_aggregate(corr, vis, f16=False).cpu()
        assert c32.dtype == torch.float32
        assert torch.equal(ops.corr_aggregate(corr, vis, split=True).cpu().view(torch.int32), ops.to_split(c32).view(torch.int32)), name + ": split volume"
        assert ops.f16_saturation_count(reset=True) == 0
        assert bits_equal(ops.corr_aggregate(corr, vis).cpu(), clamp_f16(c32)), name + ": fp16 volume"
        n = ops.f16_saturation_count(reset=True)
        if corr.dtype == torch.float32:
            assert bool(float(c32.abs().max()) > 65504.0) == saturates
            counts[name] = n
        else:
            assert n == 0, "a weighted mean of fp16 values stays inside the fp16 range"
    for name, n in counts.items():
        assert (n > 0) == saturates, (name, n, "f16_saturation_count must move only when a value left the fp16 range")


# 12 x 24: LDS-staged gather (gl_aggregate_kernel writes the three formats itself); 12 x 20 (W % 8 != 0): the direct kernels + conversions
VOLUME_CASES = [(12, 24, 1.0), (12, 24, 512.0), (12, 20, 1.0), (12, 20, 512.0)]


def test_both_roundings_match_their_host_mirrors_and_each_other(emu):
    check_roundings(emu)


@pytest.mark.parametrize("H,W,scale", VOLUME_CASES)
def test_volume_store8_in_its_four_kernels(emu, H, W, scale):
    check_volume_store(H, W, scale, emu)
