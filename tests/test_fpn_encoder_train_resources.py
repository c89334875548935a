"""CPU: no kernel of the FPN encoder's training unit (csrc/fpn_encoder_train_kernels.hip) uses scratch, read from the
compiler's kernel-resource-usage remarks that mvsformerplusplus_amd/build.py keeps per translation unit (csrc/.kernel_resources/).  The
64 x 64 x 3 x 3 weight-gradient instance keeps 36 MFMA accumulators (144 registers) per lane; a spill there would put per-lane memory traffic
into its inner loop.  Nothing is compiled here and no instruction is looked at: counts only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = os.path.join(ROOT, "mvsformerplusplus_amd", "csrc", ".kernel_resources")
UNIT = "fpn_encoder_train_kernels"
# kernel name prefix -> instances the unit must hold: BatchNorm + LeakyReLU forward and backward, the eight layers' weight gradients, the
# three stride-2 layers' parity-class data gradients, the ordered reduction of the weight gradients' partials
EXPECTED = {"fpn_bn_reduce_kernel": 2, "fpn_bn_finalize_kernel": 2, "fpn_bn_apply_kernel": 2, "fpn_wgrad_kernel": 8, "conv2d_split_kernel": 3,
            "fmt_partial_reduce_kernel": 1}


def _report():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    if not os.path.isfile(os.path.join(LOGS, UNIT + ".log")):
        pytest.skip("no resource log of %s: the library has not been built in this tree (python -m mvsformerplusplus_amd.build --force)" % UNIT)
    return list(_report().load(LOGS, UNIT).values())


def test_every_encoder_training_kernel_is_in_the_log(kernels):
    for prefix, count in EXPECTED.items():
        got = [r["name"] for r in kernels if r["name"].startswith(prefix)]
        assert len(got) == count, (prefix, count, got)
    assert len(kernels) == sum(EXPECTED.values()), [r["name"] for r in kernels]


def test_no_encoder_training_kernel_uses_scratch(kernels):
    for r in kernels:
        print(r["name"], "vgpr", r["vgpr"], "agpr", r["agpr"], "scratch", r["scratch"], "waves/SIMD", r["occ"])
        assert r["scratch"] == 0, r
