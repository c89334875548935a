#!/usr/bin/env python3
"""Generate fixture F34 (tests/golden/f34_fpn_encoder_train_*.npz) by RUNNING the reference's own FPNEncoder(norm_type='BN') in train mode
with autograd (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fpn_encoder_train.py

Module and weights are fixture F25's (tests/golden/make_golden_fpn.py): models/module.py FPNEncoder([8, 16, 32, 64]) with
synth.seeded_state_dict weights (the "enc." manifest: non-trivial BatchNorm parameters and running statistics) - here in train() mode,
fp32 on the CPU.  Input: x [2, 3, 16, 16], standard normals from torch.Generator().manual_seed(IN_SEED); shape and seed are the module case's of
tests/test_fpn_encoder_train.py, whose docstring says how they were chosen (every pre-activation clear of the LeakyReLU kink).  The loss is sum_k <out_k, cot_k>
with cot_k a standard normal of the output's shape drawn in output order (conv01, conv11, conv21, conv31) from
torch.Generator().manual_seed(COT_SEED).  Stored: both seeds, the SHA-256 of the input (fp32 bytes), the four train-mode outputs
("out/<name>"), the 33 parameter gradients ("g/<state-dict key>") and the 33 buffers after the step ("run/<state-dict key>": 22 running
tensors, 11 num_batches_tracked), spread greedily over files that each stay under 1 MiB.  Data only.
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

from models.module import FPNEncoder  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

IN_SEED, COT_SEED = 29275, 34
SHAPE = (2, 3, 16, 16)
OUTPUTS = ("conv01", "conv11", "conv21", "conv31")
FILE_BYTES = 900 * 1024


def main():
    z = np.load(os.path.join(HERE, "f25_fpn.npz"), allow_pickle=False)
    keys = [str(k) for k in z["enc.keys"].tolist()]
    shapes = [tuple(json.loads(s)) for s in z["enc.shapes"].tolist()]
    sd = synth.seeded_state_dict(dict(zip(keys, shapes)), int(z["enc.seed"]))
    torch.manual_seed(0)
    enc = FPNEncoder([8, 16, 32, 64], norm_type="BN")
    enc.load_state_dict(sd, strict=True)
    enc = enc.train()
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(IN_SEED))
    outs = enc(x)
    g = torch.Generator().manual_seed(COT_SEED)
    loss = 0.0
    data = {}
    for n, o in zip(OUTPUTS, outs):
        data["out/" + n] = o.detach().clone().numpy()
        loss = loss + (o * torch.randn(o.shape, generator=g)).sum()
    loss.backward()
    for k, p in enc.named_parameters():
        assert p.grad is not None, k
        data["g/" + k] = p.grad.numpy()
    assert len(data) == 4 + 33, len(data)
    for k, b in enc.named_buffers():
        data["run/" + k] = b.detach().numpy()
    assert len(data) == 4 + 33 + 33, len(data)
    for old in glob.glob(os.path.join(HERE, "f34_fpn_encoder_train_*.npz")):
        os.remove(old)
    files = [{"in.seed": np.array(IN_SEED), "cot.seed": np.array(COT_SEED), "in.shape": np.array(SHAPE),
              "in.sha256": np.array(hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest())}]
    room = FILE_BYTES
    for k, v in data.items():
        if v.nbytes > room:
            files.append({})
            room = FILE_BYTES
        files[-1][k] = v
        room -= v.nbytes
    for i, d in enumerate(files):
        path = os.path.join(HERE, "f34_fpn_encoder_train_%d.npz" % i)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("%s: %d bytes, %d arrays" % (os.path.basename(path), size, len(d)))


if __name__ == "__main__":
    main()
