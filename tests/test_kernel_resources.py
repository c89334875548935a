"""CPU: the register budget of the five gather launches of a reference view on the headline path (1152 x 1536, V = 5, planar fp32
features, policy "auto"), read from the compiler's kernel-resource-usage remarks that mvsformerplusplus_amd/build.py keeps per translation
unit (csrc/.kernel_resources/).  A kernel of 256 work-items shares a CU with three others - four waves per SIMD, which the 32 KiB
window allows - only while it needs at most 128 registers and no scratch; one register more and a quarter of the residency is gone
("four waves").  Nothing is compiled here and no instruction is looked at: counts only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = os.path.join(ROOT, "mvsformerplusplus_amd", "csrc", ".kernel_resources")

# launch -> (translation unit, kernel, waves/SIMD it ships with)
LAUNCHES = {
    "stage 4 pass 2": ("gather_lds_aggregate_w16_kernels", "gl_aggregate_kernel<0, 1, 1, false, true>", 4),
    "stage 3 pass 1 (keep)": ("gather_lds_keep_kernels", "gl_entropy_kernel<0, 2, 2, false, true, true>", 4),
    "stage 4 pass 1": ("gather_lds_entropy_w16_kernels", "gl_entropy_kernel<0, 1, 1, false, false, true>", 4),
    "stage 2 pass 1 (keep)": ("gather_lds_keep_kernels", "gl_entropy_kernel<0, 4, 4, false, true, true>", 4),
    "stage 1 pass 1 (keep)": ("gather_lds_keep_kernels", "gl_entropy_kernel<0, 8, 8, false, true, true>", 4),
}


def _report():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    if not os.path.isdir(LOGS) or not any(f.endswith(".log") for f in os.listdir(LOGS)):
        pytest.skip("no resource logs: the library has not been built in this tree (python -m mvsformerplusplus_amd.build --force)")
    return {(r["unit"], r["name"]): r for r in _report().load(LOGS, "gather_lds").values()}


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_gather_launch_keeps_its_waves(kernels, launch):
    unit, name, waves = LAUNCHES[launch]
    assert (unit, name) in kernels, "%s: %s is not in the log of %s" % (launch, name, unit)
    r = kernels[(unit, name)]
    print(launch, name, "vgpr", r["vgpr"], "agpr", r["agpr"], "scratch", r["scratch"], "lds", r["lds"], "waves/SIMD", r["occ"])
    assert r["scratch"] == 0, (launch, r)
    assert r["occ"] >= waves, (launch, r)
    assert r["vgpr"] + r["agpr"] <= 512 // waves, (launch, r)


def test_report_reads_a_remark_block():
    """The parser on a literal remark block (no build needed)."""
    tag = " [-Rpass-analysis=kernel-resource-usage]"
    text = "\n".join("x.h:1:1: remark: " + s + tag for s in (
        "Function Name: _ZN3mvs19gl_aggregate_kernelILi0ELi1ELi1ELb0ELb1EEEvPKvPKfS4_S4_PfS5_iiiiiiiii", "    TotalSGPRs: 100", "    VGPRs: 126",
        "    AGPRs: 0", "    ScratchSize [bytes/lane]: 0", "    Dynamic Stack: False", "    Occupancy [waves/SIMD]: 4", "    SGPRs Spill: 0",
        "    VGPRs Spill: 0", "    LDS Size [bytes/block]: 0"))
    (r,) = _report().parse(text, "unit")
    assert r["name"] == "gl_aggregate_kernel<0, 1, 1, false, true>"
    assert (r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]) == (126, 0, 100, 0, 4, 0)
