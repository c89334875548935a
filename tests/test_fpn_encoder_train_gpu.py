"""GPU (MI355X): training of the FPN encoder on the device - the checks of tests/test_fpn_encoder_train.py through its
check_* helpers against the same host fp64 oracle at the same bars and under the same condition on the oracle's pre-activations, and bit
identity of all 33 gradients and 33 buffers over two runs and on a non-default stream (nothing uses atomics).

Measured on an MI355X, worst tensor x max|g64|: weight gradients 3.6e-7, data gradients 7.1e-6, BatchNorm + LeakyReLU 1.1e-7, block nodes 8.2e-6,
the whole module 8.4e-5 (outputs 3.7e-5 of their range, running statistics 3.1e-6), the chain 1.0e-4; max |u_native - u64| = 1.32e-4 against
1.39e-4 on the emulator (DELTA 5.55e-4)."""
import pytest
import torch

import test_fpn_encoder_train as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_weight_gradients_on_device():
    print("fpn_enc_wgrad on the device vs fp64: worst |error| = %.3g x max|g64| (bar %g)" % (C.check_wgrads(DEV), C.BAR))


def test_data_gradients_on_device():
    worst = C.check_dgrads(DEV)
    C.check_dgrad_adjoint(DEV)
    print("fpn_enc_dgrad on the device vs fp64: worst |error| = %.3g x max|g64| (bar %g); stride-2 adjoint identity holds" % (worst, C.BAR))


def test_bn_leaky_and_block_nodes_on_device():
    bn, blocks = C.check_bn_leaky(DEV), C.check_blocks(DEV)
    print("encoder nodes on the device vs fp64: BatchNorm + LeakyReLU %.3g, block nodes %.3g x max|g64| (bar %g)" % (bn, blocks, C.BAR))


def test_module_backward_on_device():
    e = C.measure_u_error(DEV)
    print("max |u_native - u64| over the 11 blocks on the device: %.3g (emulator %.3g, DELTA %.3g)" % (e, C.E_MEASURED, C.DELTA))
    assert e <= C.DELTA / 2, (e, C.DELTA)
    worst, frac, run = C.check_module(DEV)
    print("fpn_encoder_forward_train on the device vs fp64: worst gradient |error| = %.3g x max|g64| over 33 tensors (bar %g); outputs %.3g of "
          "their range; running statistics %.3g" % (worst, C.BAR, frac, run))


def test_chain_on_device():
    print("image -> FPNEncoder -> FPNDecoder -> FMT_with_pathway on the device vs fp64: worst |error| = %.3g x max|g64| (bar %g)"
          % (C.check_chain(DEV), C.BAR))


def _step(x):
    m = C.trainable(DEV)
    _, grads = C.native_step(m, x)
    out = {k: v.clone() for k, v in grads.items()}
    out.update({("buffer", k): v.clone() for k, v in m.named_buffers()})
    return out


def test_bit_identity():
    """All 33 gradients and the 33 buffers: equal over two runs and on a non-default stream, at a size with several partials per launch."""
    x = torch.randn(3, 3, 24, 136, generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = _step(x), _step(x)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = _step(x)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert len(a) == 66
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
