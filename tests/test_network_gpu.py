"""GPU (MI355X): the native DINOv2MVSNet on the device - the two glue kernels against fp64 F.interpolate, fixture F29 (cases a, b, c)
through the whole module, run-to-run bit identity, a non-default stream, one graph capture of the whole forward, and the batched forward
against the same native sub-modules chained view by view.  Never reads the reference tree.

Bars: the project's, as tests/test_network.py states and asserts them (check_bicubic, check_bilinear_add, check_case are shared).  One
network (126 M parameters) is built once and serves every test.  The tests print their figures (pytest -s)."""
import pytest
import torch

from test_network import (BICUBIC_CASES, BILINEAR_CASES, F29_CASES, STAGES, case_inputs, check_bicubic, check_bicubic_view,
                          check_bilinear_add, check_case, run_captured, shared_network)
from mvsformerplusplus_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_resize_ops_on_device():
    bic = [check_bicubic(shape, size, DEV) for shape, size in BICUBIC_CASES] + [check_bicubic_view(DEV)]
    bil = [check_bilinear_add(shape, size, DEV) for shape, size in BILINEAR_CASES]
    print("on the device, x max(1, max|ref|) against fp64: resize_bicubic %s (last = strided views); resize_bilinear_add %s"
          % (["%.3g" % e for e in bic], ["%.3g" % e for e in bil]))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_f29_on_device(name):
    check_case(name, DEV)


def outputs_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in ("refined_depth", "photometric_confidence"):
        assert torch.equal(a[k], b[k]), k
    for k in STAGES:
        for name in ("depth", "photometric_confidence", "prob_volume"):
            assert torch.equal(a[k][name], b[k][name]), (k, name)


def test_bit_identity_stream_and_graph():
    H, W, V, rescale = F29_CASES["c"][:4]
    net = shared_network(DEV, rescale)
    imgs, projs, dv = case_inputs("c", DEV)
    with torch.no_grad():
        a = net(imgs, projs, dv)
        outputs_equal(a, net(imgs, projs, dv))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = net(imgs, projs, dv)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        outputs_equal(a, c)
        # one capture of the whole forward (the calls above warmed every cache and the cascade's policy for `dv`), one replay on fresh images
        static = imgs.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(static, projs, dv)
        other = torch.rand(imgs.shape, generator=torch.Generator().manual_seed(17)).to(DEV)
        static.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        eager = net(other, projs, dv)
        outputs_equal(out, eager)
        assert not torch.equal(eager["refined_depth"], a["refined_depth"])


def test_batched_forward_equals_the_modules_chained_by_hand():
    """Case a's features equal, bit for bit, the reference's eval route over the same native modules: the FPN once per view, `conv31 +
    vit_feat[vi]` by PyTorch, torch.stack, the FMT.  Batching the views and the fused add changed nothing."""
    H, W, V, rescale = F29_CASES["a"][:4]
    net = shared_network(DEV, rescale)
    imgs, projs, dv = case_inputs("a", DEV)
    _, cap = run_captured(net, imgs, projs, dv)
    with torch.no_grad():
        vit_h, vit_w = net.vit_size(H, W)
        vit_imgs = ops.resize_bicubic(imgs.reshape(V, 3, H, W), vit_h, vit_w)
        assert torch.equal(vit_imgs, cap["vit_imgs"])
        levels = [t.reshape(1, V, -1, 768) for t in net.vit.forward_interval_features(vit_imgs)]
        vit_feat = net.decoder_vit(levels, Fmats=None, vit_shape=[1, V, vit_h // 14, vit_w // 14, 768])
        assert tuple(vit_feat.shape[-2:]) == (H // 8, W // 8)
        feats = [[], [], [], []]
        for vi in range(V):
            conv01, conv11, conv21, conv31 = net.encoder(imgs[:, vi])
            conv31 = conv31 + vit_feat[vi].unsqueeze(0)
            assert torch.equal(conv31[0], cap["conv31"][vi])
            for k, f in enumerate(net.decoder(conv01, conv11, conv21, conv31)):
                feats[k].append(f)
        want = net.FMT_module({"stage%d" % (k + 1): torch.stack(f, 1) for k, f in enumerate(feats)})
    for k in STAGES:
        assert torch.equal(cap["feat"][k], want[k]), k
