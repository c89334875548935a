"""CPU: no kernel of the ViT decoder head's training unit (csrc/vitdec_head_train_kernels.hip) uses scratch, read
from the compiler's kernel-resource-usage remarks that mvsformerplusplus_amd/build.py keeps per translation unit
(csrc/.kernel_resources/).  The window GEMM keeps up to 16 MFMA accumulators per wave beside its prefetched fragments, the weight
gradient 16 accumulators, 32 prefetched values and 16 operand fragments; a spill in either would put per-lane memory traffic into the
inner loop.  Nothing is compiled here and no instruction is looked at: counts only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = os.path.join(ROOT, "mvsformerplusplus_amd", "csrc", ".kernel_resources")
UNIT = "vitdec_head_train_kernels"
# kernel name prefix -> instances the unit must hold: the window GEMM at 32 / 64 / 128 tokens per tile; the weight gradient with the row
# mapping on x (proj) and on d_z (upsamplers); the BatchNorm reduce (forward, backward from rows, backward from planar), finalize
# (forward, backward) and apply (forward rows / planar, backward rows / planar); the ordered reduction of the slab partials
EXPECTED = {"vh_gemm_kernel": 3, "vh_wgrad_kernel": 2, "vh_bn_reduce_kernel": 3, "vh_bn_finalize_kernel": 2, "vh_bn_apply_kernel": 4,
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


def test_every_head_training_kernel_is_in_the_log(kernels):
    for prefix, count in EXPECTED.items():
        got = [r["name"] for r in kernels if r["name"].startswith(prefix)]
        assert len(got) == count, (prefix, count, got)
    assert len(kernels) == sum(EXPECTED.values()), [r["name"] for r in kernels]


def test_no_head_training_kernel_uses_scratch(kernels):
    for r in kernels:
        print(r["name"], "vgpr", r["vgpr"], "agpr", r["agpr"], "scratch", r["scratch"], "waves/SIMD", r["occ"])
        assert r["scratch"] == 0, r
