#!/usr/bin/env python3
"""Measure one training step (forward + backward) of the native CrossVITDecoder (training.vitdec_forward_train);
needs the MI355X.

    python scripts/bench_vit_decoder_train.py [--cases 512x640x4,1024x1280x2] [--views 5] [--reps 30] [--out profiles/vit_decoder_train_bench.json]
                                              [--no-profile] [--head-out profiles/vit_decoder_head_train_bench.json] [--head-only]

Cases are HxWxB, images of the shipped multi-scale training list: rescale 0.4375 and patch 14 give 16 x 20 tokens at 512 x 640 and 32 x 40
at 1024 x 1280.  Inputs are random fp32 tokens [B, V, n, 768].  One process, shapes warmed, legs alternated rep by rep, device events
around each leg, median milliseconds per step with the minimum and maximum of the repetitions as the measured spread (all B x V views,
all 93 parameter gradients):
  native         TrainableCrossVITDecoder in train mode: the inference launches forward; the backward's weight gradients on
                 mvs_vitdec_wgrad, data gradients on mvs_vitdec_linear_fwd, LayerNorms on mvs_vitdec_ln_bwd; the head on PyTorch ops
  torch_fp32     PyTorch-ROCm autograd over the fp32 restatement tests/vit_decoder_train_ref.py (same weights; its discarded eval head
                 is switched off)
Also per case: the allocator's peak of each leg, the device kernels of one step by torch's profiler (count, and time per kernel name
for the native leg), whether two native steps give the same bits (output and all 93 gradients), and mvs_vitdec_wgrad against
torch.matmul (dy^T x, fp32) on the four (N, K) shapes at the case's token count.  The per-kernel times are torch's profiler's, taken in
this process on one step: a guide to where the time goes, not a substitute for a kernel trace in a run of its own.  Reads nothing
outside the repository.

--head-out adds the native-head comparison and writes its own record: two modules with the same weights,
  torch_head     TrainableCrossVITDecoder(native_head=False): the parent's path, the head on PyTorch layers - the baseline
  native_head    TrainableCrossVITDecoder(native_head=True): the head on csrc/vitdec_head_train_kernels.hip
alternated rep by rep: step time and allocator peak; the head alone, forward + backward, on fixed tokens (nn.Sequential against
training.vitdec_head_train); the new launches (vh_*) of one step by torch's profiler; and for both heads whether the head alone and
the whole step give the same bits twice.  --head-only skips everything else.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OURS = ("vd_", "vh_", "fmt_partial_reduce_kernel")
WGRAD_SHAPES = ((768, 768), (1536, 768), (3072, 768), (768, 3072))
RESCALE, PATCH = 0.4375, 14


def timed(fn, reps):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def profile_step(fn):
    """-> {"kernels": device kernels of one step, "ours": of them the library's, "by_kernel": {name: [count, total us]}}"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        by = {}
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memset" not in e.name and "Memcpy" not in e.name:
                c = by.setdefault(e.name[:96], [0, 0.0])
                c[0] += 1
                c[1] += float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0)
        total = sum(c[0] for c in by.values())
        ours = sum(c[0] for k, c in by.items() if any(o in k for o in OURS))
        top = dict(sorted(by.items(), key=lambda kv: -kv[1][1])[:24])
        top.update({k: v for k, v in by.items() if "vh_" in k})       # every launch of the head's training unit, however small
        return {"kernels": total, "ours": ours, "by_kernel_count_us": top}
    except Exception as exc:                                                      # a report, never a reason to lose the timings
        return {"error": repr(exc)}


def spread(times):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def head_case(mods, x, shape, cot, reps, no_profile):
    """The native-head comparison of one case; mods = {"torch_head": module, "native_head": module} with the same weights."""
    from mvsformerplusplus_amd import training
    B, V, h, w, _ = shape

    def clear():
        for m in mods.values():
            for p in m.parameters():
                p.grad = None

    def step(m):
        return lambda: m(x, vit_shape=shape).backward(cot)

    legs = {k: step(m) for k, m in mods.items()}
    peak = {}
    for k, fn in legs.items():
        fn(); clear(); fn(); clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        clear()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k] += timed(fn, 1)
            clear()
    # the head alone on fixed tokens, forward + backward
    tokens = torch.randn(B * V * h * w, 768, generator=torch.Generator().manual_seed(h * w)).to(cot.device)

    def head_torch(m=mods["torch_head"]):
        t = tokens.clone().requires_grad_(True)
        o = m.upsampler1(m.upsampler0(m.proj(t.reshape(B * V, h, w, 768).permute(0, 3, 1, 2))))
        o.backward(cot)
        return o, t

    def head_native(m=mods["native_head"]):
        t = tokens.clone().requires_grad_(True)
        o = training.vitdec_head_train(m, t, B * V, h, w)
        o.backward(cot)
        return o, t

    heads = {"torch_head": head_torch, "native_head": head_native}
    for fn in heads.values():
        fn(); clear(); fn(); clear()
    torch.cuda.synchronize()
    htimes = {k: [] for k in heads}
    for _ in range(reps):
        for k, fn in heads.items():
            htimes[k] += timed(fn, 1)
            clear()
    # the same bits twice?  the head alone (output, token gradient, its 9 parameter gradients) and the whole step (output, 93 gradients)
    identity = {}
    for k, m in mods.items():
        runs = []
        for _ in range(2):
            o, t = heads[k]()
            runs.append([o.detach().clone(), t.grad.clone()] + [p.grad.clone() for seq in (m.proj, m.upsampler0, m.upsampler1) for p in seq.parameters()])
            clear()
        same = [bool(torch.equal(p, q)) for p, q in zip(*runs)]
        steps = []
        for _ in range(2):
            o = m(x, vit_shape=shape)
            o.backward(cot)
            steps.append([o.detach().clone()] + [p.grad.clone() for p in m.parameters()])
            clear()
        whole = [bool(torch.equal(p, q)) for p, q in zip(*steps)]
        identity[k] = {"head_alone_output": same[0], "head_alone_token_gradient": same[1], "head_alone_parameter_gradients": sum(same[2:]),
                       "head_alone_parameter_gradients_of": len(same) - 2, "step_output": whole[0], "step_gradients": sum(whole[1:]),
                       "step_gradients_of": len(whole) - 1}
    prof = None
    if not no_profile:
        prof = {k: profile_step(fn) for k, fn in legs.items()}
        by = prof["native_head"].get("by_kernel_count_us", {})
        prof["new_launches_count_us"] = {k: v for k, v in by.items() if "vh_" in k}
        clear()
    st, hd = spread(times), spread(htimes)
    base = st["torch_head"]
    return {"tokens": [h, w], "step": st, "peak_MiB": peak, "head_alone_fwd_bwd": hd,
            "native_step_within_baseline_spread": st["native_head"]["median_ms"] <= base["median_ms"] + (base["max_ms"] - base["min_ms"]),
            "bit_identity": identity, "profile": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="512x640x4,1024x1280x2")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-profile", action="store_true", help="skip torch's profiler (kernel counts and per-kernel times)")
    ap.add_argument("--head-out", default=None, help="also compare the native head with the PyTorch head and write that record here")
    ap.add_argument("--head-only", action="store_true", help="with --head-out: skip the native / torch_fp32 legs and the wgrad comparison")
    a = ap.parse_args()
    cases = [tuple(int(v) for v in s.split("x")) for s in a.cases.split(",")]
    V = a.views
    import vit_decoder_ref as R
    import vit_decoder_train_ref as RT
    from mvsformerplusplus_amd import ops, synth
    from mvsformerplusplus_amd.vit_decoder import TrainableCrossVITDecoder
    R.head = lambda o, tokens, h, w, cap=None: tokens                # the restatement's eval head: its output is discarded by RT anyway
    dev = torch.device("cuda", 0)
    cfg = {"dino_cfg": {"cross_interval_layers": 3, "decoder_cfg": {"attention_type": "Linear", "d_model": 768, "nhead": 12, "ffn_type": "ffn",
                                                                    "init_values": 1.0, "prev_values": 0.5}}, "out_ch": 64, "vit_ch": 768}
    mod = TrainableCrossVITDecoder(cfg)
    mod.load_state_dict(synth.seeded_state_dict(synth.state_dict_manifest(mod.state_dict()), 27), strict=True)
    mod = mod.train().to(dev)
    sd = {k: (torch.nn.Parameter(v.detach().clone()) if v.is_floating_point() and "running_" not in k else v.detach().clone())
          for k, v in mod.state_dict().items()}
    leaves = [v for v in sd.values() if isinstance(v, torch.nn.Parameter)]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "views": V, "cases": {}}
    head_result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "views": V, "cases": {}}
    if a.head_out:
        native_mod = TrainableCrossVITDecoder(cfg, native_head=True)
        native_mod.load_state_dict(mod.state_dict(), strict=True)
        native_mod = native_mod.train().to(dev)
    for H, W, B in cases:
        h, w = int(H * RESCALE) // PATCH, int(W * RESCALE) // PATCH
        n, shape = h * w, [B, V, h, w, 768]
        g = torch.Generator().manual_seed(H + W)
        x = [torch.randn(B, V, n, 768, generator=g).to(dev) for _ in range(3)]
        cot = torch.randn(B * V, 64, 4 * h, 4 * w, generator=g).to(dev)
        if a.head_out:
            hr = head_case({"torch_head": mod, "native_head": native_mod}, x, shape, cot, a.reps, a.no_profile)
            head_result["cases"]["%dx%d B=%d" % (H, W, B)] = hr
            print("%dx%d B=%d V=%d head: step %s; head alone %s; peak MiB %s" % (H, W, B, V, hr["step"], hr["head_alone_fwd_bwd"], hr["peak_MiB"]),
                  flush=True)
            if a.head_only:
                continue

        def native():
            mod(x, vit_shape=shape).backward(cot)

        def torch_fp32():
            RT.vit_decoder_train(x, sd, shape, dtype=torch.float32).backward(cot, inputs=leaves)

        def clear():
            for t in list(mod.parameters()) + leaves:
                t.grad = None

        legs = {"native": native, "torch_fp32": torch_fp32}
        peak = {}
        for k, fn in legs.items():                       # warm shapes (library searches, allocator), then the allocator's peak of one step
            fn(); clear(); fn(); clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            clear()
        times = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                times[k] += timed(fn, 1)
                clear()
        # two native steps: the same bits?
        outs, toks = [], []
        hook = mod.proj.register_forward_pre_hook(lambda m, inp: toks.append(inp[0].detach().clone()))
        for _ in range(2):
            o = mod(x, vit_shape=shape)
            o.backward(cot)
            outs.append([o.detach().clone()] + [p.grad.clone() for p in mod.parameters()])
            clear()
        hook.remove()
        same = [bool(torch.equal(p, q)) for p, q in zip(*outs)]
        # where a difference comes from: the tokens the five blocks hand to the head (the library's launches), and the head (PyTorch's
        # convolutions) run twice on the same tokens, forward and backward
        head = []
        for _ in range(2):
            t = toks[0].clone().requires_grad_(True)
            o = mod.upsampler1(mod.upsampler0(mod.proj(t)))
            o.backward(cot)
            head.append([o.detach().clone(), t.grad.clone(), mod.proj[0].weight.grad.clone()])
            clear()
        parts = {"tokens_into_the_head": bool(torch.equal(toks[0], toks[1])), "head_alone_output": bool(torch.equal(head[0][0], head[1][0])),
                 "head_alone_token_gradient": bool(torch.equal(head[0][1], head[1][1])),
                 "head_alone_proj_weight_gradient": bool(torch.equal(head[0][2], head[1][2]))}
        prof = None if a.no_profile else {"native": profile_step(native), "torch_fp32": profile_step(torch_fp32)}
        clear()
        # the weight-gradient kernel against rocBLAS on the same operands
        M = B * V * n
        wg = {}
        for N, K in WGRAD_SHAPES:
            dy, xx = torch.randn(M, N, device=dev), torch.randn(M, K, device=dev)
            ours, blas = (lambda: ops.vitdec_wgrad(dy, xx)), (lambda: torch.matmul(dy.t(), xx))
            ours(); blas(); ours(); blas()
            torch.cuda.synchronize()
            t_o, t_b = [], []
            for _ in range(a.reps):
                t_o += timed(ours, 1)
                t_b += timed(blas, 1)
            wg["%dx%d" % (N, K)] = {"M": M, "slabs": ops.vitdec_wgrad_slabs(M, N, K), "native_ms": statistics.median(t_o),
                                    "matmul_ms": statistics.median(t_b)}
        med = {k: statistics.median(v) for k, v in times.items()}
        r = {"tokens": [h, w], "ms_per_step": med, "min_ms": {k: min(v) for k, v in times.items()},
             "max_ms": {k: max(v) for k, v in times.items()}, "peak_MiB": peak,
             "speedup_vs_torch_fp32": med["torch_fp32"] / med["native"], "two_steps_bit_identical": dict(parts, output=same[0], gradients=sum(same[1:]), of=len(same) - 1),
             "profile": prof, "wgrad_vs_matmul": wg}
        result["cases"]["%dx%d B=%d" % (H, W, B)] = r
        print("%dx%d B=%d V=%d (%d x %d tokens): native %.3f ms, torch fp32 autograd %.3f ms per step; peak %.0f vs %.0f MiB; wgrad %s"
              % (H, W, B, V, h, w, med["native"], med["torch_fp32"], peak["native"], peak["torch_fp32"],
                 {k: (round(v["native_ms"], 3), round(v["matmul_ms"], 3)) for k, v in wg.items()}), flush=True)
    if a.head_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.head_out)), exist_ok=True)
        with open(a.head_out, "w") as f:
            json.dump(head_result, f, indent=1)
        if a.head_only:
            print(json.dumps(head_result))
            return
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
