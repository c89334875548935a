"""GPU (MI355X): training of the FPN decoder on the device - the three shapes of tests/test_fpn_train.py, its single
nodes and the decoder -> FMT_with_pathway chain against the same host fp64 oracle at the same bars; bit identity of all 26 gradients and
the running statistics over two runs and on a non-default stream (nothing uses atomics: asserted); and the allocator-peak proof that the
fused last level never materialises its 64-channel full-resolution map, forward or backward.

Measured on an MI355X, worst tensor x max|g64|: cases a / b / c 1.5e-5 / 1.7e-5 / 1.8e-5, heads 9.2e-6, merges 5.4e-6, fused level 3 1.4e-5,
the chain 3.4e-5; the fused level's peak lay 13.25 MB = 2.53 views' worth of the map over the step's end (bar 3; a whole map is 6)."""
import pytest
import torch

import test_fpn_train as C
from mvsformerplusplus_amd import training

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_module_backward_on_device(case):
    worst, frac, run = C.check_module_case(case, DEV)
    print("fpn_decoder_forward_train on the device vs fp64, case %s: worst gradient |error| = %.3g x max|g64| over 22 tensors (bar %g); outputs "
          "%.3g of their range; running statistics %.3g" % (case, worst, C.BAR, frac, run))


def test_single_nodes_on_device():
    heads, merges, level3 = C.check_heads(DEV), C.check_merges(DEV), C.check_level3(DEV)
    print("FPN decoder nodes on the device vs fp64: heads %.3g, merges %.3g, fused level 3 %.3g x max|g64| (bar %g)" % (heads, merges, level3, C.BAR))


def test_chain_into_fmt_on_device():
    print("FPNDecoder -> FMT_with_pathway chain on the device vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (C.check_chain(DEV), C.BAR))


def _step(case):
    m = C.trainable(DEV)
    xs = [x.clone().to(DEV).requires_grad_(True) for x in C.inputs(case)]
    _, grads = C.native_step(m, xs)
    out = {k: v.clone() for k, v in grads.items()}
    out.update({("buffer", k): v.clone() for k, v in m.named_buffers()})
    return out


def test_bit_identity():
    """All 26 gradients and the 12 buffers: equal over two runs and on a non-default stream."""
    for case in ("b", "c"):
        a, b = _step(case), _step(case)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = _step(case)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert len(a) == 38
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (case, k)


def test_level3_never_materialises_its_map():
    """Fused level 3 forward + backward at N = 6, 128 x 160: the allocator's peak, minus what is allocated when the step ends (output and
    gradients), stays below three views' worth of the 64-channel map.  A whole intra3 or d intra3 costs six; what the node holds at its
    peak is the pre-activation z and dz (0.75 of a view's map each at N = 6) and a one-view slab of d intra3."""
    N, H, W = 6, 128, 160
    ts, cot = C.level3_case(N, H // 8, W // 8, 7)
    cot = cot.to(DEV)
    bn = C._bn(8, DEV)
    leaves = C._leaves(ts, DEV)

    def step():
        for t in leaves:
            t.grad = None
        y = training.FpnLevel3Train.apply(leaves[0], leaves[1], bn, *leaves[2:])
        y.backward(cot)
        return y

    step()                                                  # warm-up: allocator blocks
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    y = step()
    torch.cuda.synchronize()
    over = torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()
    view_map = 64 * H * W * 4
    print("fused level 3 forward + backward at %dx%d N=%d: peak over the step's end %.2f MB = %.2f views' worth of the 64-channel map (bar 3, a whole "
          "map 6)" % (H, W, N, over / 1e6, over / view_map))
    assert y.shape == (N, 8, H, W) and all(t.grad is not None for t in leaves)
    assert over < 3 * view_map, (over, view_map)
