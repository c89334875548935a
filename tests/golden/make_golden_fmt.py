#!/usr/bin/env python3
"""Generate fixture F26 (tests/golden/f26_fmt*.npz) by RUNNING the reference's own FMT_with_pathway (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fmt.py

Module: models/FMT.py FMT_with_pathway(**FMT_config) with the shipped FMT_config of config/mvsformer++.json, eval mode, fp32, CPU, with
synth.seeded_state_dict weights (ls*.gamma take synth's generic N(0, 2) branch: a fair stress).  The manifest, the seed, the config and
the SHA-256 of the regenerated state dict are stored IN the fixture ("fmt." prefix), not in weights_sha256.json.

Cases (every tensor fp32; each file stays under 1 MiB):
  case a = B 1, V 3, stage1 8 x 12 (n = 96), exact 2:1 levels
    f26_fmt.npz             manifest; inputs stage1..3; every block's input and output tokens [1, 96, 64] for the reference view (self
                            layers) and for source view 1 (all layers), from forward hooks on FMT.layers[i]; the refs list
    f26_fmt_a_out.npz       outputs stage1..3; the inputs of smooth_1 / smooth_2 (the merged maps, all three views, from hooks)
    f26_fmt_a_full.npz      input stage4; the input of smooth_3 for view 1
    f26_fmt_a_full_out.npz  output stage4
  case b = B 2, V 2, stage1 3 x 9 with levels 5 x 18, 10 x 36, 20 x 72 (ragged, not 2:1: F20's shapes)
    f26_fmt_b.npz           module inputs and outputs
"""
import hashlib
import json
import os
import sys

import numpy as np

REF = os.environ.get("MVS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.dont_write_bytecode = True

import torch  # noqa: E402

from models.FMT import FMT_with_pathway  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

SEED = 26
CHS = (64, 32, 16, 8)


def sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def feats(g, B, V, sizes):
    return {"stage%d" % (k + 1): torch.randn(B, V, c, *sizes[k], generator=g) for k, c in enumerate(CHS)}


def main():
    torch.manual_seed(0)
    cfg = json.load(open(os.path.join(REF, "config", "mvsformer++.json")))["arch"]["args"]["FMT_config"]
    mod = FMT_with_pathway(**cfg)
    man = synth.state_dict_manifest(mod.state_dict())
    sd = synth.seeded_state_dict(man, SEED)
    mod.load_state_dict(sd, strict=True)
    mod = mod.eval()
    meta = {"fmt.keys": np.array(list(man.keys())), "fmt.shapes": np.array([json.dumps(list(s)) for s in man.values()]),
            "fmt.seed": np.array(SEED), "fmt.sha256": np.array(sha(sd)), "fmt.config": np.array(json.dumps(cfg))}

    blocks = {i: [] for i in range(len(mod.FMT.layers))}
    smooth = {k: [] for k in (1, 2, 3)}
    hooks = []
    for i, layer in enumerate(mod.FMT.layers):
        hooks.append(layer.register_forward_hook(
            lambda m, args, kwargs, out, i=i: blocks[i].append((kwargs["x"].detach().clone(), out.detach().clone())), with_kwargs=True))
    for k in (1, 2, 3):
        hooks.append(getattr(mod, "smooth_%d" % k).register_forward_hook(lambda m, inp, out, k=k: smooth[k].append(inp[0].detach().clone())))

    g = torch.Generator().manual_seed(2026)
    fa = feats(g, 1, 3, [(8, 12), (16, 24), (32, 48), (64, 96)])
    fb = feats(g, 2, 2, [(3, 9), (5, 18), (10, 36), (20, 72)])
    names = cfg["layer_names"]
    with torch.no_grad():
        oa = mod(fa)
        a, a_out, a_full, a_full_out = dict(meta), {}, {}, {}
        for s in (1, 2, 3):
            a["a/stage%d" % s] = fa["stage%d" % s]
            a_out["a/out_stage%d" % s] = oa["stage%d" % s]
        a_full["a/stage4"] = fa["stage4"]
        a_full_out["a/out_stage4"] = oa["stage4"]
        refs = []
        for i, n in enumerate(names):
            calls = blocks[i]                               # self layers: reference view, source 1, source 2; cross layers: source 1, source 2
            assert len(calls) == (3 if n == "self" else 2), (i, len(calls))
            if n == "self":
                a["a/ref/blk%d_in" % i], a["a/ref/blk%d_out" % i] = calls[0]
                refs.append(calls[0][1])
            a["a/src/blk%d_in" % i], a["a/src/blk%d_out" % i] = calls[-2]
        a["a/refs"] = torch.stack(refs)
        for k in (1, 2):
            a_out["a/smooth%d_in" % k] = torch.cat(smooth[k])           # [3, C, H, W]
        a_full["a/smooth3_in_v1"] = smooth[3][1]
        ob = mod(fb)
        b = {}
        for s in (1, 2, 3, 4):
            b["b/stage%d" % s] = fb["stage%d" % s]
            b["b/out_stage%d" % s] = ob["stage%d" % s]
    for h in hooks:
        h.remove()
    for name, d in (("f26_fmt.npz", a), ("f26_fmt_a_out.npz", a_out), ("f26_fmt_a_full.npz", a_full), ("f26_fmt_a_full_out.npz", a_full_out),
                    ("f26_fmt_b.npz", b)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (name, size)
        print("%s: %d bytes, %d arrays" % (name, size, len(d)))


if __name__ == "__main__":
    main()
