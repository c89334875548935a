#!/usr/bin/env python3
"""Generate fixture F35 (tests/golden/f35_vitdec_train_*.npz) by RUNNING the reference's own CrossVITDecoder in train mode with autograd
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vit_decoder_train.py

Module, weights and inputs are fixture F27's (tests/golden/make_golden_vit_decoder.py): models/module.py CrossVITDecoder(args) with the
synth.seeded_state_dict weights of F27's manifest and F27's inputs of case a ([1, 3, 4, 6, 768]) and case b ([2, 2, 3, 5, 768], levels 1
and 2 scaled x30) - here in train() mode, fp32 on the CPU; every case starts from F27's weights and buffers.  The loss is <out, cot> with
cot a standard normal of the output's shape from torch.Generator().manual_seed(35).  The 93 gradients are about 150 MB, so F35 stores
DATA ONLY and little of it, per case under the prefix "a/" | "b/":
    out                  the train-mode output
    run/<key>            the nine buffers after the step (6 running tensors, 3 num_batches_tracked)
    g/<key>              every gradient with at most 16384 elements, whole
    gs/<key>             for each larger gradient [sum, sum of squares] in fp64 ...
    gx/<key>             ... and the sample g.flatten()[::numel // 4096 + 1] (the stride is coprime to every inner dimension of these shapes)
    in.sha256            SHA-256 of the three inputs (fp32 bytes, level order)
and "cot.seed".  Files stay under 1 MiB each.
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

from models.module import CrossVITDecoder  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

COT_SEED = 35
WHOLE = 16384
SAMPLES = 4096
FILE_BYTES = 900 * 1024
CASES = (("a", [1, 3, 4, 6, 768]), ("b", [2, 2, 3, 5, 768]))


def sample_stride(numel):
    return numel // SAMPLES + 1


def main():
    f27 = {}
    for name in ("f27_vitdec_a_in.npz", "f27_vitdec_b.npz"):
        z = np.load(os.path.join(HERE, name), allow_pickle=False)
        f27.update({k: z[k] for k in z.files})
    keys = [str(k) for k in f27["vitdec.keys"].tolist()]
    shapes = [tuple(json.loads(s)) for s in f27["vitdec.shapes"].tolist()]
    sd = synth.seeded_state_dict(dict(zip(keys, shapes)), int(f27["vitdec.seed"]))
    args = json.loads(str(f27["vitdec.config"]))
    data = {"cot.seed": np.array(COT_SEED)}
    for case, shape in CASES:
        torch.manual_seed(0)
        mod = CrossVITDecoder(args)
        mod.load_state_dict(sd, strict=True)
        mod = mod.train()
        x = [torch.from_numpy(f27["%s/x%d" % (case, i)]) for i in range(3)]
        h = hashlib.sha256()
        for t in x:
            h.update(t.contiguous().numpy().tobytes())
        data[case + "/in.sha256"] = np.array(h.hexdigest())
        out = mod(x, vit_shape=shape)
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(COT_SEED))
        (out * cot).sum().backward()
        data[case + "/out"] = out.detach().numpy()
        for k, b in mod.named_buffers():
            data["%s/run/%s" % (case, k)] = b.detach().numpy()
        count = 0
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            g = p.grad.detach()
            count += 1
            if g.numel() <= WHOLE:
                data["%s/g/%s" % (case, k)] = g.numpy()
            else:
                g64 = g.double()
                data["%s/gs/%s" % (case, k)] = np.array([float(g64.sum()), float((g64 * g64).sum())])
                data["%s/gx/%s" % (case, k)] = g.flatten()[::sample_stride(g.numel())].contiguous().numpy()
        assert count == 93 and len(list(mod.named_buffers())) == 9, count
    for old in glob.glob(os.path.join(HERE, "f35_vitdec_train_*.npz")):
        os.remove(old)
    files, room = [{}], FILE_BYTES
    for k, v in data.items():
        if v.nbytes > room:
            files.append({})
            room = FILE_BYTES
        files[-1][k] = v
        room -= v.nbytes
    for i, d in enumerate(files):
        path = os.path.join(HERE, "f35_vitdec_train_%d.npz" % i)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("%s: %d bytes, %d arrays" % (os.path.basename(path), size, len(d)))


if __name__ == "__main__":
    main()
