"""GPU (MI355X): the stage-1 transformer regulariser kernel by kernel on the device against the fp64 restatement (tests/transformer_ref.py
on the host) - the checks of tests/test_transformer.py with the device as their argument (same cases, same bars) - plus run-to-run bit
identity of the module at B = 2 and a non-default stream.  This is the first place the K = 512 embedding (down_rate = 4: 132 864 bytes
of dynamic LDS) and the N = 512 up-projection run on a device.

Measured on an MI355X (the whole table, with the emulator's and the models' figures beside it, is in tests/test_transformer.py): entry
points 1.8e-6 .. 7.7e-6 x max(1, max|ref|) (bar 3e-5) for all four patches, K = 512 included; whole module in "bf16x3" 1.3e-5 of the
output's range at the shipped patch (936 tokens) and 2.9e-5 at down_rate = 4 (bar 2e-4); with the default attention ("attn16") 9.0e-5
and 5.4e-4 against model figures of 1.0e-4 and 4.7e-4 (bar: 4 x the model); F31 7.9e-6 / 1.1e-5 ("bf16x3", against the reference) and
5.4e-4 / 1.1e-3 ("attn16", model 7.4e-4 / 1.2e-3).  The file takes about three seconds."""
import pytest
import torch

from test_fmt import LAYER_BAR, MODULE_BAR
from test_transformer import (ATTENTION_MODES, ATTENTION_N, MODULE_CASES, RATES, _dev, check_attention_small, check_attention_stress, check_f31,
                              check_linear, check_module, check_patch_kernels, check_positions, check_raw_and_encoding, check_refusals, figure,
                              make_module, module_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("epi", ["bias", "gelu", "res_ln"])
def test_linear(epi):
    worst, model = check_linear(DEV, epi)
    figure("tr_linear %s on the device, x max(1, max|ref|)" % epi, worst, model, LAYER_BAR)


@pytest.mark.parametrize("rate", RATES, ids=lambda r: "x".join(map(str, r)))
def test_embed_and_up_prob(rate):
    for what, (worst, model) in check_patch_kernels(DEV, rate).items():
        figure("tr_%s patch %s on the device, x max(1, max|ref|)" % (what, rate), worst, model, LAYER_BAR)


@pytest.mark.parametrize("shape", [(2, 8, 16, 24), (2, 8, 144, 192)], ids=["small", "grid_wraps"])
def test_positions(shape):
    e_pos, e_rng = check_positions(DEV, *shape)
    print("position3d %s on the device: |error| %.3g (bar 1e-5), ranges %.3g (bar 1e-3)" % (shape, e_pos, e_rng))


def test_raw_positions_and_encoding():
    e_raw, e_pe = check_raw_and_encoding(DEV)
    print("position3d_raw on the device |error| %.3g; position_encoding3d |error| %.3g (bar 2e-6)" % (e_raw, e_pe))


@pytest.mark.parametrize("mode", ATTENTION_MODES)
@pytest.mark.parametrize("n", ATTENTION_N)
def test_attention_at_padding_boundaries(n, mode):
    print("attention stress n = %d %s on the device: |error| %.3g" % (n, mode, check_attention_stress(DEV, n, mode)))


@pytest.mark.parametrize("mode", ATTENTION_MODES)
@pytest.mark.parametrize("n", [1, 2])
def test_attention_one_and_two_tokens(n, mode):
    err, bound = check_attention_small(DEV, n, mode)
    print("attention n = %d %s on the device: |error| %.3g (the formats allow %.3g)" % (n, mode, err, bound))


@pytest.mark.parametrize("precision", ["bf16x3", "attn16"])
@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_module_against_fp64(name, precision):
    frac, model = check_module(DEV, name, precision)
    figure("module %s %s on the device, of the output's range" % (name, precision), frac, model, MODULE_BAR if precision == "bf16x3" else "4 x model")


@pytest.mark.parametrize("precision", ["bf16x3", "attn16"])
def test_module_against_f31(precision):
    for (frac, model), key in zip(check_f31(DEV, precision), ("y", "y_nope")):
        figure("F31 %s %s on the device, of the output's range" % (key, precision), frac, model, MODULE_BAR if precision == "bf16x3" else "4 x model")


def test_refusals():
    check_refusals(DEV)


@pytest.mark.parametrize("precision", ["bf16x3", "attn16"])
@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_bit_identity_and_stream(name, precision):
    """Two runs of the module at B = 2 give the same bits, and so does a run on a non-default stream."""
    c = module_case(name)
    net = make_module(c["cfg"], c["sd"], DEV, precision)
    x, pos = _dev(c["x"], DEV), _dev(c["pos"], DEV)
    with torch.no_grad():
        a = net(x, pos)
        b = net(x, pos)
        assert torch.equal(a, b)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            s = net(x, pos)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert torch.equal(a, s)
