"""GPU (MI355X): the native FMT_with_pathway on the device - F26, both full sizes at V = 5 against the fp64 restatement
(tests/fmt_ref.py on the host), run-to-run bit identity, a non-default stream, one graph capture, and the two allocator-peak proofs
that neither the full-resolution merged map nor the 256-wide hidden activation is ever written."""
import pytest
import torch

import fmt_ref as R
from test_fmt import MODULE_BAR, STAGES, check_entry_points, check_module, f26, f26_config, f26_weights, module, within_range

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHS = (64, 32, 16, 8)


def seeded_inputs(H, W, V, seed, B=1):
    g = torch.Generator().manual_seed(seed)
    return {"stage%d" % (k + 1): torch.randn(B, V, c, H // s, W // s, generator=g) for k, (c, s) in enumerate(zip(CHS, (8, 4, 2, 1)))}


def test_f26_on_device():
    fx = f26()
    layer = check_entry_points(fx, DEV)
    worst = check_module(fx, DEV)
    print("FMT vs F26 on the device: entry points %.3g x max(1, max|ref|); whole module %.3g of an output's range" % (layer, worst))


@pytest.mark.parametrize("H,W", [(1152, 1536), (1088, 1920)])
def test_full_size_against_restatement(H, W):
    """V = 5 (stage1 144 x 192 / 136 x 240) against the restatement in fp64 on the host."""
    fx = f26()
    m = module(fx, DEV)
    sd = f26_weights(fx)
    feats = seeded_inputs(H, W, 5, H + W)
    with torch.no_grad():
        got = {s: t.cpu() for s, t in m({s: t.to(DEV) for s, t in feats.items()}).items()}
        torch.set_num_threads(16)
        ref = R.fmt(feats, sd, f26_config(fx)["layer_names"])
    worst = 0.0
    for s in STAGES:
        frac = within_range(got[s], ref[s], MODULE_BAR, (H, W, s))
        print("%dx%d V=5 %s: |error| = %.3g of the output's range" % (H, W, s, frac))
        worst = max(worst, frac)
    print("%dx%d V=5: worst |error| = %.3g of an output's range (bar %g)" % (H, W, worst, MODULE_BAR))


def test_bit_identity_stream_and_graph():
    fx = f26()
    m = module(fx, DEV)
    feats = {s: t.to(DEV) for s, t in seeded_inputs(256, 320, 3, 1, B=2).items()}
    with torch.no_grad():
        a = m(feats)
        b = m(feats)
        for s in STAGES:
            assert torch.equal(a[s], b[s]), s
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = m(feats)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        for s in STAGES:
            assert torch.equal(a[s], c[s]), s
        # one capture (weights and the position table are cached by the calls above) and one replay on fresh input values
        static = {s: t.clone() for s, t in feats.items()}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(static)
        other = {s: t.to(DEV) for s, t in seeded_inputs(256, 320, 3, 2, B=2).items()}
        for s in STAGES:
            static[s].copy_(other[s])
        graph.replay()
        torch.cuda.synchronize()
        eager = m(other)
        for s in STAGES:
            assert torch.equal(out[s], eager[s]), s


def _peak_rise(fn):
    fn()                                                    # warm-up: packed weights, position table and allocator blocks
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def test_full_resolution_level_never_writes_the_merged_map():
    """During the full-resolution pathway level (16 -> 8, its ops wrapper) at 1152 x 1536, V = 5, the allocator's peak rises by less than
    the output's bytes + one view's 8-channel full-resolution fp32 map: a merged map materialised for even one view fails this."""
    from mvsformerplusplus_amd import ops
    H, W, V = 1152, 1536, 5
    m = module(f26(), DEV)
    w_red, w_sm = m._params(torch.device(DEV))["level3"]
    g = torch.Generator().manual_seed(4)
    prev = torch.randn(V, 16, H // 2, W // 2, generator=g).to(DEV)
    lat = torch.randn(V, 8, H, W, generator=g).to(DEV)
    one_view = 8 * H * W * 4
    rise = _peak_rise(lambda: ops.fmt_path(prev, lat, w_red, w_sm))
    print("pathway level 3 at %dx%d V=%d: peak rise %.1f MB (output %.1f MB, one view's map %.1f MB)" % (H, W, V, rise / 1e6, V * one_view / 1e6, one_view / 1e6))
    assert rise < V * one_view + one_view, rise
    unfused = _peak_rise(lambda: ops.fmt_smooth(ops.fmt_merge(prev, lat, w_red), w_sm))
    assert unfused >= 2 * V * one_view, unfused             # the check can see a materialised map: the unfused form shows all five


def test_block_never_writes_the_hidden_activation():
    """During one block over the four source views at 1152 x 1536 the peak rises by less than the output tokens' bytes + one view's
    256-wide hidden activation (n x 256 x 4 bytes)."""
    from mvsformerplusplus_amd import ops
    h, w, N = 144, 192, 4
    n = h * w
    m = module(f26(), DEV)
    wp, vec = m._params(torch.device(DEV))["block1"]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, 64, h, w, generator=g).to(DEV)
    kv = ops.fmt_kv(torch.randn(1, 64, h, w, generator=g).to(DEV), wp, vec)
    rise = _peak_rise(lambda: ops.fmt_block(x, kv, wp, vec, kv_div=N))
    print("block over %d views of %d tokens: peak rise %.1f MB (output %.1f MB, one hidden activation %.1f MB)"
          % (N, n, rise / 1e6, N * n * 64 * 4 / 1e6, n * 256 * 4 / 1e6))
    assert rise < N * n * 64 * 4 + n * 256 * 4, rise
