#!/usr/bin/env python3
"""Generate fixture F32 (tests/golden/f32_fmt_train_*.npz) by RUNNING the reference's own FMT_with_pathway in train mode with autograd
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fmt_train.py

Module, config, weights and inputs are fixture F26's (tests/golden/make_golden_fmt.py): models/FMT.py FMT_with_pathway(**FMT_config),
synth.seeded_state_dict weights, case a (B 1, V 3, stage1 8 x 12, exact 2:1 levels), fp32 on the CPU - here in train() mode.  The loss
is sum_s <out[s], cot[s]> with cot[s] a standard normal of the output's shape drawn in stage order from torch.Generator().manual_seed(
COT_SEED).  Stored: the SHA-256 of the four train-mode outputs (fp32 bytes in stage order), COT_SEED, and the 70 gradients - "g/in/stageK"
for the four inputs, "g/<state-dict key>" for the 66 parameters - spread greedily over files that each stay under 1 MiB.  Data only.
"""
import glob
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

COT_SEED = 32
STAGES = ("stage1", "stage2", "stage3", "stage4")
FILE_BYTES = 900 * 1024


def load(name):
    z = np.load(os.path.join(HERE, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def main():
    fx = load("f26_fmt.npz")
    fx.update(load("f26_fmt_a_full.npz"))
    cfg = json.loads(str(fx["fmt.config"]))
    shapes = [tuple(json.loads(s)) for s in fx["fmt.shapes"].tolist()]
    sd = synth.seeded_state_dict(dict(zip([str(k) for k in fx["fmt.keys"].tolist()], shapes)), int(fx["fmt.seed"]))
    torch.manual_seed(0)
    mod = FMT_with_pathway(**cfg)
    mod.load_state_dict(sd, strict=True)
    mod = mod.train()
    feats = {s: torch.from_numpy(fx["a/" + s]).clone().requires_grad_(True) for s in STAGES}
    out = mod(feats)
    g = torch.Generator().manual_seed(COT_SEED)
    loss = 0.0
    h = hashlib.sha256()
    for s in STAGES:
        h.update(out[s].detach().contiguous().numpy().tobytes())
        loss = loss + (out[s] * torch.randn(out[s].shape, generator=g)).sum()
    loss.backward()
    grads = {"g/in/" + s: feats[s].grad.numpy() for s in STAGES}
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        grads["g/" + k] = p.grad.numpy()
    assert len(grads) == 70, len(grads)
    for old in glob.glob(os.path.join(HERE, "f32_fmt_train_*.npz")):
        os.remove(old)
    files = [{"out.sha256": np.array(h.hexdigest()), "cot.seed": np.array(COT_SEED)}]
    room = FILE_BYTES
    for k, v in grads.items():
        if v.nbytes > room:
            files.append({})
            room = FILE_BYTES
        files[-1][k] = v
        room -= v.nbytes
    for i, d in enumerate(files):
        path = os.path.join(HERE, "f32_fmt_train_%d.npz" % i)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("%s: %d bytes, %d arrays" % (os.path.basename(path), size, len(d)))


if __name__ == "__main__":
    main()
