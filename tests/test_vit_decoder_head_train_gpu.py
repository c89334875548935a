"""GPU (MI355X): the native train-mode head of the CrossVITDecoder on the device - the checks of
tests/test_vit_decoder_head_train.py through its check_* helpers against the same host fp64 oracles at the same bars, and bit identity
of the head alone (output, token gradient, 9 parameter gradients, 6 running tensors) over two runs and on a non-default stream, at F27's
case a and at (NV, h, w) = (4, 16, 20), where every weight-gradient launch has several slabs and every BatchNorm reduction several
partials per channel (no oracle at that size).  Whole-step bit identity is measured by scripts/bench_vit_decoder_train.py and reported
in DESIGN.md, not asserted: part of a block's backward runs on PyTorch einsums.

Measured on an MI355X: see the figures each test prints (pytest -s) and DESIGN.md section 4.21."""
import pytest
import torch

import test_vit_decoder_head_train as H

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_window_gemms_on_device():
    z, dx, dw = H.check_convs(DEV)
    print("head convolutions on the device vs fp64 on %s: pre-activation %.3g, data gradient %.3g, weight gradient %.3g x max(1, max|ref|) "
          "(bar %g)" % (H.shapes(), z, dx, dw, H.LAYER_BAR))


def test_token_batchnorm_on_device():
    fwd, bwd = H.check_bn(DEV)
    print("token-major BatchNorm + SiLU on the device vs fp64: forward %.3g x max(1, max|ref|) (bar %g), backward %.3g x max|g64| (bar %g)"
          % (fwd, H.LAYER_BAR, bwd, H.BAR))


def test_head_nodes_on_device():
    print("head-layer nodes on the device vs fp64 autograd: worst gradient |error| = %.3g x max|g64| (bar %g); conv bias gradients exactly zero"
          % (H.check_nodes(DEV), H.BAR))


def test_module_with_native_head_on_device():
    for case, (worst, frac, run) in H.check_module(DEV).items():
        print("vitdec_forward_train with the native head on the device, case %s vs fp64: worst gradient |error| = %.3g x max|g64| over 93 "
              "tensors (bar %g); output %.3g of its range; running statistics %.3g" % (case, worst, H.BAR, frac, run))


@pytest.mark.parametrize("shape", [(3, 4, 6), (4, 16, 20)])
def test_head_is_bit_identical(shape):
    """Two runs on the current stream and one on a non-default stream: 19 tensors, torch.equal."""
    from mvsformerplusplus_amd import ops
    if shape == (4, 16, 20):
        assert all(ops.vitdec_head_wgrad_slabs(layer, 4, 16 * s, 20 * s) > 1 for layer, s in ((0, 1), (1, 1), (2, 2)))
        assert ops.lib().mvs_vitdec_head_bn_workspace_bytes(4 * 16 * 20, 256) > (2 + 2) * 256 * 8            # several partials per channel
    a = H.check_head_bit_identity(DEV, *shape)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = H.head_alone(DEV, *shape)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(a, c)):
        assert torch.equal(p, q), ("the head on a non-default stream differs", i, shape)
