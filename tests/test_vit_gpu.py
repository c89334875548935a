"""GPU (MI355X): the native DINOv2 ViT-B/14 on the device - F28 (entry points and module), ragged sizes and one view at the product's
36 x 48 patches against the fp64 restatement (tests/vit_ref.py on the host, 16 threads), the forced-rescale attention case, run-to-run
bit identity, a non-default stream, one graph capture, and the chain into CrossVITDecoder through the strided outputs.

Bars: the project's LAYER_BAR / MODULE_BAR (tests/test_vit.py, where the format's own error is measured and the choice is written down).
One view at 36 x 48 is the smallest case with the product's token count (1729) and grid size; V = 5 adds nothing that the batched small
cases do not cover.  The tests print their figures (pytest -s)."""
import pytest
import torch

import vit_ref as R
from test_vit import MODULE_BAR, check_entry_points, check_forced_rescale, check_module, f28, f28_weights, module, within_range

pytestmark = pytest.mark.gpu
DEV = "cuda"


def images(NV, gh, gw, seed):
    return torch.randn(NV, 3, 14 * gh, 14 * gw, generator=torch.Generator().manual_seed(seed))


def test_f28_on_device():
    fx = f28()
    layer = check_entry_points(fx, DEV)
    fr = check_module(fx, DEV)
    print("vit vs F28 on the device: entry points %.3g x max(1, max|ref|); whole module %s (a) / %s (b) of each level's range"
          % (layer, ["%.3g" % f for f in fr["a"]], ["%.3g" % f for f in fr["b"]]))


@pytest.mark.parametrize("NV,gh,gw", [(3, 9, 13), (2, 17, 23), (1, 36, 48)])
def test_against_restatement(NV, gh, gw):
    """3 views of 9 x 13 patches (118 tokens: ragged everywhere), 2 views of 17 x 23 (392 tokens: several key steps) and one view at the
    product's 36 x 48 (1729 tokens) against fp64 on the host."""
    fx = f28()
    m = module(fx, DEV)
    sd = f28_weights(fx)
    x = images(NV, gh, gw, gh + gw)
    got = [t.cpu() for t in m.forward_interval_features(x.to(DEV))]
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = R.vit(x, sd)
        model = R.vit(x, sd, split_operands=True) if gh < 36 else None
    for i in range(3):
        frac = within_range(got[i], ref[i], MODULE_BAR, (NV, gh, gw, i))
        rng = float(ref[i].max() - ref[i].min())
        fmt = float((model[i] - ref[i]).abs().max()) / rng if model is not None else float("nan")
        print("%d x (%d x %d) level %d: |error| = %.3g of the level's range (bar %g); two-term operand model %.3g" % (NV, gh, gw, i, frac, MODULE_BAR, fmt))


def test_attention_forced_rescale_on_device():
    got, fmt = check_forced_rescale(DEV)
    print("forced rescale on the device: %.3g x max(1, max|ref|); the format alone %.3g" % (got, fmt))


def test_bit_identity_stream_and_graph():
    fx = f28()
    m = module(fx, DEV)
    x = images(3, 9, 13, 1).to(DEV)
    same = lambda a, b: len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))
    a = m.forward_interval_features(x)
    assert same(a, m.forward_interval_features(x))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = m.forward_interval_features(x)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert same(a, c)
    # one capture (packed weights and the position table are cached by the calls above) and one replay on fresh input values
    static = x.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.forward_interval_features(static)
    other = images(3, 9, 13, 2).to(DEV)
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, m.forward_interval_features(other))


def test_chained_with_the_decoder():
    """CrossVITDecoder fed the ViT's three strided outputs (views of the padded buffers, read in place) equals CrossVITDecoder fed their
    contiguous copies, bit for bit."""
    import test_vit_decoder as TD
    m = module(f28(), DEV)
    dec = TD.module(TD.f27(), DEV)
    B, V, gh, gw = 1, 3, 5, 7
    feats = [t.reshape(B, V, -1, 768) for t in m.forward_interval_features(images(B * V, gh, gw, 4).to(DEV))]
    assert all(not t.is_contiguous() and t.stride(2) == 768 for t in feats)
    shape = [B, V, gh, gw, 768]
    with torch.no_grad():
        assert torch.equal(dec(feats, vit_shape=shape), dec([t.contiguous() for t in feats], vit_shape=shape))
