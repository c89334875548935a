"""GPU (MI355X): the native CrossVITDecoder on the device - F27 (entry points and module), both product sizes at V = 5 against the fp64
restatement (tests/vit_decoder_ref.py on the host, 16 threads), run-to-run bit identity, a non-default stream and one graph capture.

No allocator-peak test: the [M, 3072] hidden activation IS written (packed-split, 4 bytes per element), so
there is no never-written claim to prove.

Bars: the project's LAYER_BAR / MODULE_BAR (tests/test_vit_decoder.py).  Next to each measured error the test prints the error of the
FORMAT (the fp64 restatement with every GEMM operand rounded to hi + lo bf16) and the fp32 restatement's own distance from fp64.
Measured on an MI355X: entry points 8.38e-6 x max(1, max|ref|) (emulator 9.73e-6); module against F27 1.11e-5 (a) / 1.20e-5 (b) of the
output's range (emulator 1.08e-5 / 1.29e-5); V = 5 against fp64: 1.03e-5 at 36 x 48 tokens and 1.03e-5 at 34 x 60, where the format's own
error is 8.1e-6 / 8.4e-6 and PyTorch-ROCm fp32 sits 1.6e-6 / 2.4e-6 from fp64."""
import pytest
import torch

import vit_decoder_ref as R
from test_vit_decoder import MODULE_BAR, check_entry_points, check_module, f27, f27_weights, module, within_range

pytestmark = pytest.mark.gpu
DEV = "cuda"


def seeded_inputs(B, V, n, seed, scales=(1.0, 30.0, 30.0)):
    """Three [B, V, n, 768] levels; the middle and last level x30 as in F27 case b (the reference notes that those ViT levels are large)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, V, n, 768, generator=g) * s for s in scales]


def test_f27_on_device():
    fx = f27()
    layer = check_entry_points(fx, DEV)
    fr = check_module(fx, DEV)
    print("vitdec vs F27 on the device: entry points %.3g x max(1, max|ref|); whole module %.3g (a) / %.3g (b) of the output's range"
          % (layer, fr["a"], fr["b"]))


@pytest.mark.parametrize("h,w", [(36, 48), (34, 60)])
def test_full_size_against_restatement(h, w):
    """V = 5 at 1152 x 1536 (36 x 48 tokens) and 1088 x 1920 (34 x 60 tokens: int(H 0.4375 // 14 * 14) / 14) against fp64 on the host."""
    fx = f27()
    m = module(fx, DEV)
    sd = f27_weights(fx)
    V, shape = 5, [1, 5, h, w, 768]
    x = seeded_inputs(1, V, h * w, h + w)
    with torch.no_grad():
        got = m([t.to(DEV) for t in x], vit_shape=shape).cpu()
        sd_dev = {k: v.to(DEV) for k, v in sd.items()}
        ref32 = R.vit_decoder([t.to(DEV) for t in x], sd_dev, shape, dtype=torch.float32).cpu()
        torch.set_num_threads(16)
        ref = R.vit_decoder(x, sd, shape)
        model = R.vit_decoder(x, sd, shape, split_operands=True)
    rng = float(ref.max() - ref.min())
    fmt_err = float((model - ref).abs().max()) / rng
    f32_err = float((ref32.double() - ref).abs().max()) / rng
    frac = float((got.double() - ref).abs().max()) / rng
    print("%d x %d tokens V=5: |error| = %.3g of the output's range (bar %g); two-term operand model %.3g; PyTorch-ROCm fp32 vs fp64 %.3g"
          % (h, w, frac, MODULE_BAR, fmt_err, f32_err))
    within_range(got, ref, MODULE_BAR, (h, w))


def test_bit_identity_stream_and_graph():
    fx = f27()
    m = module(fx, DEV)
    B, V, h, w = 2, 3, 9, 13                                      # n = 117: ragged tiles everywhere
    shape = [B, V, h, w, 768]
    x = [t.to(DEV) for t in seeded_inputs(B, V, h * w, 1)]
    with torch.no_grad():
        a = m(x, vit_shape=shape)
        b = m(x, vit_shape=shape)
        assert torch.equal(a, b)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = m(x, vit_shape=shape)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert torch.equal(a, c)
        # the ViT's output minus its class token: a strided view, read in place
        g = torch.Generator().manual_seed(3)
        with_cls = [(torch.randn(B * V, h * w + 1, 768, generator=g) * s).to(DEV) for s in (1.0, 30.0, 30.0)]
        strided = [t[:, 1:].unflatten(0, (B, V)) for t in with_cls]
        assert torch.equal(m(strided, vit_shape=shape), m([t.contiguous() for t in strided], vit_shape=shape))
        # one capture (packed weights are cached by the calls above) and one replay on fresh input values
        static = [t.clone() for t in x]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(static, vit_shape=shape)
        other = [t.to(DEV) for t in seeded_inputs(B, V, h * w, 2)]
        for s, o in zip(static, other):
            s.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m(other, vit_shape=shape))
