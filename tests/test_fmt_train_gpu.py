"""GPU (MI355X): training of FMT_with_pathway on the device - F26 cases a and b and one shape that spans several
workgroups, partials and key/value slabs with ragged edges, every gradient against fp64 autograd of tests/fmt_ref.py on the host at the
bar of tests/test_fmt_train.py (max|g - g64| <= 2e-4 x max|g64| per tensor); run-to-run and cross-stream bit identity of the pathway
gradients; and the allocator-peak proof that a level's forward + backward never materialises the merged map.

Measured on an MI355X, worst tensor x max|g64|: levels 6.7e-6, single blocks 9.8e-7, F26 case a 1.7e-5, case b 1.9e-5, the ragged shape
2.4e-5; the whole module's 70 gradients were bit-identical over two runs; the level's peak rise 21.9 MB against 19.7 MB of output +
gradients and a 7.9 MB map."""
import pytest
import torch

import fmt_ref as R
import test_fmt as T
import test_fmt_train as TT
from mvsformerplusplus_amd import training

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGES = T.STAGES


def test_f26_gradients_on_device():
    levels, blocks = TT.check_levels(DEV), TT.check_blocks(DEV)
    a, b = TT.check_module_case("a", DEV), TT.check_module_case("b", DEV)
    print("FMT training on the device vs fp64: levels %.3g, blocks %.3g, module case a %.3g, case b %.3g x max|g64| (bar %g)"
          % (levels, blocks, a, b, TT.BAR))


def ragged_inputs(seed=9):
    """B 1, V 3, stage1 9 x 25 -> levels 18 x 50, 36 x 100, 72 x 200: 225 tokens (two key/value slabs, a ragged last tile), up to 15
    coarse-pixel chunks and 72 tiles per view with ragged right edges."""
    g = torch.Generator().manual_seed(seed)
    return {"stage%d" % (k + 1): torch.randn(1, 3, c, 9 * 2 ** k, 25 * 2 ** k, generator=g) for k, c in enumerate((64, 32, 16, 8))}


def test_ragged_multi_workgroup_shape_against_fp64():
    _, sd, cfg = TT.fixture()
    base = ragged_inputs()
    torch.set_num_threads(16)
    feats64 = {s: t.double().requires_grad_(True) for s, t in base.items()}
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    out64 = R.fmt(feats64, sd64, cfg["layer_names"])
    cot = TT.cotangents({s: out64[s].shape for s in STAGES})
    sum((out64[s] * cot[s].double()).sum() for s in STAGES).backward()
    want = {("in", s): feats64[s].grad for s in STAGES}
    want.update({k: v.grad for k, v in sd64.items()})
    m = TT.trainable(DEV)
    out, grads = TT.native_grads(m, {s: t.clone().to(DEV).requires_grad_(True) for s, t in base.items()})
    for s in STAGES:
        T.within_range(out[s].detach().cpu(), out64[s].detach(), TT.BAR, s)
    worst = TT.worst_rel(grads, want, "ragged shape")
    print("fmt_forward_train at 9 x 25 tokens, V = 3 vs fp64: worst |error| = %.3g x max|g64| over 70 gradients (bar %g)" % (worst, TT.BAR))


def _level_grads(C, N, hw, HW, seed):
    prev, lat, w_red, w_sm, cot = (t.to(DEV) for t in TT.level_case(C, N, hw, HW, seed))
    leaves = [t.clone().requires_grad_(True) for t in (prev, lat, w_red, w_sm)]
    training.FmtPathLevelTrain.apply(*leaves).backward(cot)
    return [t.grad for t in leaves]


def test_bit_identity():
    """Pathway gradients (no atomics anywhere) are bit-identical from run to run and on a non-default stream: asserted.  Whole-module
    gradients are compared the same way and the result is printed: the blocks' GEMMs are rocBLAS's."""
    for C, N, hw, HW in ((32, 3, (36, 50), (72, 100)), (8, 3, (72, 100), (144, 200)), (16, 2, (7, 9), (13, 20))):
        a = _level_grads(C, N, hw, HW, 3)
        b = _level_grads(C, N, hw, HW, 3)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = _level_grads(C, N, hw, HW, 3)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z), (C, hw, HW)
    m = TT.trainable(DEV)
    base = ragged_inputs()
    runs = []
    for _ in range(2):
        _, g = TT.native_grads(m, {s: t.clone().to(DEV).requires_grad_(True) for s, t in base.items()})
        runs.append({k: v.clone() for k, v in g.items()})
    differ = [str(k) for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]
    print("whole-module gradients over two runs: %d of %d tensors differ bitwise %s" % (len(differ), len(runs[0]), differ[:6]))


def test_level_forward_backward_never_writes_the_merged_map():
    """Forward + backward of one full-resolution level (C = 8, 256 x 320, N = 3): the allocator's peak rises by less than the output, the
    gradients and ONE further [N, C, H, W] map - the merged map is materialised in neither direction (the workspaces of the weight
    gradients' partials, 3 MB at most, fit in the margin)."""
    N, C, H, W = 3, 8, 256, 320
    prev, lat, w_red, w_sm, cot = (t.to(DEV) for t in TT.level_case(C, N, (H // 2, W // 2), (H, W), 5))
    leaves = [t.clone().requires_grad_(True) for t in (prev, lat, w_red, w_sm)]

    def step():
        for t in leaves:
            t.grad = None
        y = training.FmtPathLevelTrain.apply(*leaves)
        y.backward(cot)
        return y

    step()                                                  # warm-up: allocator blocks
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    one_map = N * C * H * W * 4
    held = y.numel() * 4 + sum(t.grad.numel() * 4 for t in leaves)
    print("level 3 forward + backward at %dx%d N=%d: peak rise %.2f MB (output + gradients %.2f MB, one map %.2f MB)"
          % (H, W, N, rise / 1e6, held / 1e6, one_map / 1e6))
    assert rise < held + one_map, (rise, held, one_map)
