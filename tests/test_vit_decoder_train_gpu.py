"""GPU (MI355X): training of the CrossVITDecoder on the device - the checks of tests/test_vit_decoder_train.py
through its check_* helpers against the same host fp64 oracle at the same bars, and bit identity of the mvs_vitdec_wgrad and
mvs_vitdec_ln_bwd outputs over two runs and on a non-default stream at the multi-slab M (nothing uses atomics).  Whole-step bit identity
is measured by scripts/bench_vit_decoder_train.py and reported in DESIGN.md, not asserted: part of a block's backward and the head run on
PyTorch ops.

Measured on an MI355X: see the figures each test prints (pytest -s) and DESIGN.md section 4.20."""
import pytest
import torch

import test_vit_decoder_train as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_wgrad_on_device():
    print("vitdec_wgrad on the device vs fp64 (M = %s): worst |error| = %.3g x max(1, max|ref|) (bar %g)"
          % (C.token_counts(), C.check_wgrad(DEV), C.LAYER_BAR))


def test_ln_bwd_on_device():
    print("vitdec_ln_bwd on the device vs fp64 autograd: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (C.check_ln_bwd(DEV), C.LAYER_BAR))


def test_data_gradient_gemms_on_device():
    print("data-gradient GEMMs on the device vs fp64: worst |error| = %.3g x max(1, max|ref|) (bar %g)" % (C.check_dgrad(DEV), C.LAYER_BAR))


def test_nodes_on_device():
    blocks, mix = C.check_blocks(DEV), C.check_mix(DEV)
    print("decoder nodes on the device vs fp64: block nodes %.3g, mix node %.3g x max|g64| (bar %g); block forward = the inference bits"
          % (blocks, mix, C.BAR))


def test_module_backward_on_device():
    for case, (worst, frac, run) in C.check_module(DEV).items():
        print("vitdec_forward_train on the device, case %s vs fp64: worst gradient |error| = %.3g x max|g64| over 93 tensors (bar %g); output "
              "%.3g of its range; running statistics %.3g" % (case, worst, C.BAR, frac, run))


def test_kernels_are_bit_identical():
    """mvs_vitdec_wgrad (with its bias) and mvs_vitdec_ln_bwd at the multi-slab M and at a size with many slabs and partials: equal over two
    runs and on a non-default stream."""
    from mvsformerplusplus_amd import ops
    g = torch.Generator().manual_seed(9)
    for M in (C.multi_slab_m(), 1300):
        dy, x, w = torch.randn(M, 768, generator=g).to(DEV), torch.randn(M, 768, generator=g).to(DEV), torch.randn(768, generator=g).to(DEV)

        def run():
            return ops.vitdec_wgrad(dy, x, want_bias=True) + ops.vitdec_ln_bwd(dy, x, w, 1e-5, add=x)

        a, b = run(), run()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = run()
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert len(a) == 5
        for p, q, r in zip(a, b, c):
            assert torch.equal(p, q) and torch.equal(p, r), M
