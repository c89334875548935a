#!/usr/bin/env python3
"""Generate fixture F33 (tests/golden/f33_fpn_decoder_train_*.npz) by RUNNING the reference's own FPNDecoder in train mode with autograd
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fpn_train.py

Module and weights are fixture F25's (tests/golden/make_golden_fpn.py): models/module.py FPNDecoder([8, 16, 32, 64]) with
synth.seeded_state_dict weights (non-trivial BatchNorm parameters and running statistics) - here in train() mode, fp32 on the CPU.
Inputs: N = 2, conv31 4 x 6 (full resolution 32 x 48), standard normals drawn in the order conv01, conv11, conv21, conv31 from
torch.Generator().manual_seed(IN_SEED).  The loss is sum_k <out_k, cot_k> with cot_k a standard normal of the output's shape drawn in
output order from torch.Generator().manual_seed(COT_SEED).  Stored: both seeds, the SHA-256 of the inputs (fp32 bytes in draw order),
the four train-mode outputs' SHA-256, the 26 gradients - "g/in/convK1" for the four inputs, "g/<state-dict key>" for the 22
parameters -, the 8 updated running tensors and the 4 num_batches_tracked ("run/<state-dict key>"), spread greedily over files that
each stay under 1 MiB.  Data only.
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

from models.module import FPNDecoder  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

IN_SEED, COT_SEED = 330, 33
N, H31, W31 = 2, 4, 6
INPUTS = ("conv01", "conv11", "conv21", "conv31")
FILE_BYTES = 900 * 1024


def input_shapes(n=N, h=H31, w=W31):
    return [(n, 8, 8 * h, 8 * w), (n, 16, 4 * h, 4 * w), (n, 32, 2 * h, 2 * w), (n, 64, h, w)]


def main():
    z = np.load(os.path.join(HERE, "f25_fpn.npz"), allow_pickle=False)
    keys = [str(k) for k in z["dec.keys"].tolist()]
    shapes = [tuple(json.loads(s)) for s in z["dec.shapes"].tolist()]
    sd = synth.seeded_state_dict(dict(zip(keys, shapes)), int(z["dec.seed"]))
    torch.manual_seed(0)
    dec = FPNDecoder([8, 16, 32, 64])
    dec.load_state_dict(sd, strict=True)
    dec = dec.train()
    g = torch.Generator().manual_seed(IN_SEED)
    xs = [torch.randn(s, generator=g).requires_grad_(True) for s in input_shapes()]
    hin = hashlib.sha256()
    for x in xs:
        hin.update(x.detach().contiguous().numpy().tobytes())
    outs = dec(*xs)
    g = torch.Generator().manual_seed(COT_SEED)
    loss, hout = 0.0, hashlib.sha256()
    for o in outs:
        hout.update(o.detach().contiguous().numpy().tobytes())
        loss = loss + (o * torch.randn(o.shape, generator=g)).sum()
    loss.backward()
    data = {"g/in/" + n: x.grad.numpy() for n, x in zip(INPUTS, xs)}
    for k, p in dec.named_parameters():
        assert p.grad is not None, k
        data["g/" + k] = p.grad.numpy()
    assert len(data) == 26, len(data)
    for k, b in dec.named_buffers():
        data["run/" + k] = b.detach().numpy()
    assert len(data) == 26 + 12, len(data)
    for old in glob.glob(os.path.join(HERE, "f33_fpn_decoder_train_*.npz")):
        os.remove(old)
    files = [{"in.seed": np.array(IN_SEED), "cot.seed": np.array(COT_SEED), "in.sha256": np.array(hin.hexdigest()),
              "out.sha256": np.array(hout.hexdigest()), "in.shape": np.array([N, H31, W31])}]
    room = FILE_BYTES
    for k, v in data.items():
        if v.nbytes > room:
            files.append({})
            room = FILE_BYTES
        files[-1][k] = v
        room -= v.nbytes
    for i, d in enumerate(files):
        path = os.path.join(HERE, "f33_fpn_decoder_train_%d.npz" % i)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("%s: %d bytes, %d arrays" % (os.path.basename(path), size, len(d)))


if __name__ == "__main__":
    main()
