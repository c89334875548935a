"""CPU: no kernel of the ViT decoder's training unit (csrc/vitdec_train_kernels.hip) uses scratch, read from the
compiler's kernel-resource-usage remarks that mvsformerplusplus_amd/build.py keeps per translation unit (csrc/.kernel_resources/).  The
weight-gradient kernel keeps 16 MFMA accumulators (64 registers), 32 prefetched values and 16 operand fragments per lane; a spill there
would put per-lane memory traffic into its inner loop.  Nothing is compiled here and no instruction is looked at: counts only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = os.path.join(ROOT, "mvsformerplusplus_amd", "csrc", ".kernel_resources")
UNIT = "vitdec_train_kernels"
# kernel name prefix -> instances the unit must hold: the token weight-gradient GEMM, LayerNorm backward, the packed-split row pass, the
# ordered reduction of the partials
EXPECTED = {"vd_wgrad_kernel": 1, "vd_ln_bwd_kernel": 1, "vd_pack_kernel": 1, "fmt_partial_reduce_kernel": 1}


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


def test_every_decoder_training_kernel_is_in_the_log(kernels):
    for prefix, count in EXPECTED.items():
        got = [r["name"] for r in kernels if r["name"].startswith(prefix)]
        assert len(got) == count, (prefix, count, got)
    assert len(kernels) == sum(EXPECTED.values()), [r["name"] for r in kernels]


def test_no_decoder_training_kernel_uses_scratch(kernels):
    for r in kernels:
        print(r["name"], "vgpr", r["vgpr"], "agpr", r["agpr"], "scratch", r["scratch"], "waves/SIMD", r["occ"])
        assert r["scratch"] == 0, r
