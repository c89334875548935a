#!/usr/bin/env python3
"""Generate fixture F25 (tests/golden/f25_fpn*.npz) by RUNNING the reference's own FPNEncoder / FPNDecoder (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fpn.py

Modules: models/module.py FPNEncoder(feat_chs = [8, 16, 32, 64], norm_type="BN") and FPNDecoder([8, 16, 32, 64]) - both shipped
configs - in eval mode, fp32, with synth.seeded_state_dict weights (non-trivial BatchNorm statistics).  The manifests, seeds and the
SHA-256 of the regenerated state dicts are stored IN the fixture ("enc." / "dec." prefixes), not in weights_sha256.json.

Cases (every tensor fp32; each file stays under 1 MiB):
  f25_fpn.npz          case a = x [1, 3, 64, 96]: the encoder's input and every layer's output (forward hooks: conv00 .. conv31;
                       each layer's input is the previous layer's output)
  f25_fpn_decoder.npz  case a, decoder on the encoder's outputs: out0 .. out3 and the merged maps intra1 / intra2 (inputs of out1 /
                       out2, captured with hooks); intra3 (input of out3) is not stored - the native path never forms it
  f25_fpn_n2.npz       case b = x [2, 3, 40, 56] (coarse maps 5 x 7: the align_corners upsample is not a plain 2:1): the module inputs
                       and outputs of both
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

from models.module import FPNDecoder, FPNEncoder  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

FEAT_CHS = [8, 16, 32, 64]
ENC_SEED, DEC_SEED = 25, 26
ENC_LAYERS = ["conv00", "conv01", "downsample1", "conv10", "conv11", "downsample2", "conv20", "conv21", "downsample3", "conv30", "conv31"]


def sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def seeded(mod, seed, prefix, meta):
    man = synth.state_dict_manifest(mod.state_dict())
    sd = synth.seeded_state_dict(man, seed)
    mod.load_state_dict(sd, strict=True)
    meta[prefix + "keys"] = np.array(list(man.keys()))
    meta[prefix + "shapes"] = np.array([json.dumps(list(s)) for s in man.values()])
    meta[prefix + "seed"] = np.array(seed)
    meta[prefix + "sha256"] = np.array(sha(sd))
    return mod.eval()


def main():
    torch.manual_seed(0)
    meta = {}
    enc = seeded(FPNEncoder(FEAT_CHS, norm_type="BN"), ENC_SEED, "enc.", meta)
    dec = seeded(FPNDecoder(FEAT_CHS), DEC_SEED, "dec.", meta)
    cap = {}

    def out_hook(name):
        return lambda m, i, o: cap.__setitem__(name, o.detach().clone())

    def in_hook(name):
        return lambda m, i, o: cap.__setitem__(name, i[0].detach().clone())

    hooks = [getattr(enc, n).register_forward_hook(out_hook(n)) for n in ENC_LAYERS]
    hooks += [dec.out1.register_forward_hook(in_hook("intra1")), dec.out2.register_forward_hook(in_hook("intra2"))]
    g = torch.Generator().manual_seed(2025)
    xa = torch.randn(1, 3, 64, 96, generator=g)
    xb = torch.randn(2, 3, 40, 56, generator=g)
    a, a_dec, b = dict(meta), {}, {}
    with torch.no_grad():
        cap.clear()
        ea = enc(xa)
        da = dec(*ea)
        a["a/x"] = xa
        for n in ENC_LAYERS:
            a["a/" + n] = cap[n]
        for k in range(4):
            a_dec["a/out%d" % k] = da[k]
        a_dec["a/intra1"], a_dec["a/intra2"] = cap["intra1"], cap["intra2"]
        eb = enc(xb)
        db = dec(*eb)
        b["b/x"] = xb
        for n, t in zip(["conv01", "conv11", "conv21", "conv31"], eb):
            b["b/" + n] = t
        for k in range(4):
            b["b/out%d" % k] = db[k]
    for h in hooks:
        h.remove()
    for name, d in (("f25_fpn.npz", a), ("f25_fpn_decoder.npz", a_dec), ("f25_fpn_n2.npz", b)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (name, size)
        print("%s: %d bytes, %d arrays" % (name, size, len(d)))


if __name__ == "__main__":
    main()
