"""GPU (MI355X): the case functions of tests/test_conv3d_family.py on the device - every row of the two tile tables in every format at the
seam shapes, the two fused heads, and the persistent kernels with MORE THAN 8 x CU COUNT tiles per launch.

Eight 256-thread blocks (32 waves) is what a CU holds at most, so whatever the occupancy query of launch_conv_bf / launch_deconv_bf answers,
at more than 8 x CU count tiles every working block of a persistent launch walks a run of at least two tiles - the prefetch of the next
tile under the current one's contraction, the second barrier per tile - and some blocks find no work and return.  Kernel-level shapes with a
few dozen tiles never get there on 256 CUs.  The tiles are spread over all three axes (4 x 8 x (8 CU / 32 + 1): 2080 on 256 CUs) with a
ragged last tile on each, batch 1; inputs are 5 - 25 MB.  The float64 reference (the slow part, on the host) is computed once per operand
model and shared by the formats that see the same operands.  Every large launch runs twice on the default stream and once on another one:
the three results are bit-identical.  The two kd = 1 rows' one-term kernels are left to the emulator.

Bars: tests/test_conv3d_family.py.  Worst figures of the device run (pytest -s prints each):
  split-bf16 (x max(1, max|ref|), bar 3e-5)   bf16x3 8.4e-6, split 9.1e-6; deconv3d_prob 2.1e-6 / 3.5e-6, conv3d_logits 4.1e-6 / 4.1e-6
  fp32 (fraction of K 2^-24 S, bar 1)          0.11
  fp16 (a) (fraction of its bar, bar 1)        f16x2 0.99, f16 0.99; deconv3d_prob 3.6e-4, conv3d_logits 5.5e-3
  fp16 (b) (share of differing bits, cap 2 %)  f16x2 0.066 %, f16 0.060 % pooled per row, 0.083 % / 0.077 % on a single tensor
  many tiles (2080 on 256 CUs)                 bf16x3 5.0e-6, split 6.6e-6, fp16 (a) 0.99, (b) 0.032 %, deconv3d_prob 2.1e-6
The split-bf16 and fp32 figures are the emulator's.  The fp16 chain errors are two to three times SMALLER than the emulator's (share of
differing bits 0.06 % against 0.12 - 0.17 %, conv3d_logits 5.5e-3 against 1.4e-2 of the bar): the emulator's MFMA adds the 32 products
of a block one by one, each add rounded to fp32 (tests/hipemu/hip/hip_runtime.h); the hardware's block sum is evidently more exact.
"""
import pytest
import torch

from test_conv3d_family import (CONV_ROWS, DECONV_ROWS, FORMATS, MFMA, PERSISTENT_CONV, PERSISTENT_DECONV, REFUSED, case_conv_logits, case_conv_row,
                                case_deconv_prob, case_deconv_row, case_persistent, flat_id, persistent_instantiations)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCKS_PER_CU = 8          # 2048 work-items = 32 waves per CU: no kernel of 256-thread blocks holds more

# the persistent instantiations run at device size: the Cin = 8 convs and the 16 -> 8 transposed rows in every MFMA format, 16 -> 16 in f16
LARGE = [("conv", (8, 16, 3, (2, 2, 2))), ("conv", (8, 16, 3, (1, 2, 2))), ("conv", (8, 16, 3, (1, 1, 1))), ("conv", (16, 16, 3, (1, 1, 1))),
         ("deconv", (16, 8, 2)), ("deconv", (16, 8, 1))]


@pytest.mark.parametrize("key", CONV_ROWS, ids=lambda k: "%dto%d_k%d_s%d%d%d" % (k[0], k[1], k[2], *k[3]))
def test_conv_row(key):
    state, _ = case_conv_row(DEV, key)
    assert set(state) == set(FORMATS) and all((v == "refused") == (("conv", key, f) in REFUSED) for f, v in state.items())


@pytest.mark.parametrize("key", DECONV_ROWS, ids=lambda k: "%dto%d_sd%d" % k)
def test_deconv_row(key):
    state, _ = case_deconv_row(DEV, key)
    assert set(state) == set(FORMATS) and all((v == "refused") == (("deconv", key, f) in REFUSED) for f, v in state.items())


@pytest.mark.parametrize("sd", [2, 1])
def test_deconv_prob(sd):
    case_deconv_prob(DEV, sd)


def test_conv_logits():
    case_conv_logits(DEV)


def same_on_every_run(call):
    """call() twice on the current stream and once on a second one: bit-identical.  -> the first result."""
    a, b = call(), call()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = call()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "run to run"
    assert torch.equal(a, c), "stream to stream"
    return a


@pytest.mark.parametrize("kind,key", LARGE, ids=flat_id)
def test_persistent_many_tiles(kind, key):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (4, 8, BLOCKS_PER_CU * cus // 32 + 1)
    assert tiles[0] * tiles[1] * tiles[2] > BLOCKS_PER_CU * cus
    torch.set_num_threads(16)
    case_persistent(DEV, kind, key, tiles, 1, BLOCKS_PER_CU * cus, run=same_on_every_run)


def test_every_persistent_instantiation_is_run_at_device_size():
    left_to_the_emulator = [("conv", (16, 16, 1, (1, 1, 1))), ("conv", (16, 8, 1, (1, 1, 1)))]
    assert sorted(LARGE + left_to_the_emulator) == sorted(persistent_instantiations())
    assert all((PERSISTENT_CONV if kind == "conv" else PERSISTENT_DECONV)[key] in (MFMA, ("f16",)) for kind, key in LARGE)
