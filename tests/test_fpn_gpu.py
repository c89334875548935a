"""GPU (MI355X): the native FPN encoder / decoder on the device - F25, both full image sizes against the restatement (tests/fpn_ref.py,
fp32 on the host for the whole image), run-to-run bit identity, a non-default stream, and the peak-memory proof that the decoder's
last level never forms its 64-channel full-resolution map."""
import pytest
import torch

import fpn_ref as R
from test_fpn import MODULE_BAR, check_layers, check_modules, f25, f25_weights, modules, within_range

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_f25_on_device():
    fx = f25()
    check_layers(fx, DEV)
    worst = check_modules(fx, DEV)
    print("FPN modules vs F25 on the device: worst |error| = %.3g of an output's range" % worst)


@pytest.mark.parametrize("H,W", [(1152, 1536), (1088, 1920)])
def test_full_size_against_restatement(H, W):
    """N = 5 in one call against the restatement (fp32, host), and N = 1 per view: bit-equal to the batched call."""
    fx = f25()
    enc, dec = modules(fx, DEV)
    sde, sdd = f25_weights(fx, "enc."), f25_weights(fx, "dec.")
    x = torch.randn(5, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    with torch.no_grad():
        e5 = enc(x.to(DEV))
        d5 = dec(*e5)
        got = [t.cpu() for t in e5 + d5]
        torch.set_num_threads(16)
        eref = R.encoder(x, sde, dtype=torch.float32)
        dref = R.decoder(*eref, sdd, dtype=torch.float32)
        worst = 0.0
        for g, r, n in zip(got, eref + dref, ["conv01", "conv11", "conv21", "conv31", "out0", "out1", "out2", "out3"]):
            worst = max(worst, within_range(g, r, MODULE_BAR, (H, W, n)))
        for v in (0, 4):
            one = enc(x[v:v + 1].to(DEV))
            one = one + dec(*one)
            for a, b in zip(one, got):
                assert torch.equal(a[0].cpu(), b[v]), "per-view call != batched call"
    print("%dx%d N=5: worst |error| = %.3g of an output's range" % (H, W, worst))


def test_bit_identity_and_non_default_stream():
    fx = f25()
    enc, dec = modules(fx, DEV)
    x = torch.randn(2, 3, 256, 320, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        a = enc(x)
        a = a + dec(*a)
        b = enc(x)
        b = b + dec(*b)
        for s, t in zip(a, b):
            assert torch.equal(s, t)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = enc(x)
            c = c + dec(*c)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        for s, t in zip(a, c):
            assert torch.equal(s, t)


def test_decoder_peak_memory_proves_the_fusion():
    """During FPNDecoder.forward at 1152 x 1536 the allocator's peak rises by less than one 64-channel fp32 full-resolution map
    (64 H W 4 = 453 MB); the decoder's own outputs and intra1 / intra2 total about 250 MB."""
    H, W = 1152, 1536
    fx = f25()
    _, dec = modules(fx, DEV)
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(1, c, H // s, W // s, generator=g).to(DEV) for c, s in ((8, 1), (16, 2), (32, 4), (64, 8))]
    with torch.no_grad():
        out = dec(*feats)                                   # warm-up: packed weights cached
        del out
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = dec(*feats)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print("FPNDecoder at %dx%d: peak rise %.1f MB (one 64-channel map: %.1f MB)" % (H, W, rise / 1e6, 64 * H * W * 4 / 1e6))
    assert rise < 64 * H * W * 4, rise
