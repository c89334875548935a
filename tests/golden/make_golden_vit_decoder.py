#!/usr/bin/env python3
"""Generate fixture F27 (tests/golden/f27_vitdec*.npz) by RUNNING the reference's own CrossVITDecoder (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vit_decoder.py

Module: models/module.py CrossVITDecoder(args) with arch.args of config/mvsformer++.json, eval mode, fp32, CPU, with
synth.seeded_state_dict weights (ls*.gamma and prev_values take synth's generic N(0, 2) branch: a fair stress).  The manifest, the seed,
the config and the SHA-256 of the regenerated state dict are stored IN the fixture ("vitdec." prefix), not in weights_sha256.json.

Cases (every tensor fp32; each file stays under 1 MiB):
  case a = B 1, V 3, h x w = 4 x 6 (n = 24)
    f27_vitdec_a_in.npz    manifest; the three inputs
    f27_vitdec_a_ref.npz   reference view: input and output tokens of both self blocks (forward hooks with kwargs); the two
                           AAS-normalised reference features (the keys of cross blocks 1 and 2, from the hooks' `key`)
    f27_vitdec_a_src.npz   source view 1: input and output tokens of the three cross blocks
    f27_vitdec_a_head.npz  the [3, 24, 768] token tensor before proj (hook on proj's input); outputs of proj, upsampler0, upsampler1
  case b = B 2, V 2, h x w = 3 x 5 (n = 15, not a multiple of 16); level-1 and level-2 inputs scaled x30 (the reference's own comment
    says the middle ViT levels are large)
    f27_vitdec_b.npz       inputs and output
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

from models.module import CrossVITDecoder  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

SEED = 27


def sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    torch.manual_seed(0)
    full = json.load(open(os.path.join(REF, "config", "mvsformer++.json")))["arch"]["args"]
    args = {"dino_cfg": full["dino_cfg"], "out_ch": full["out_ch"], "vit_ch": full["vit_ch"]}
    mod = CrossVITDecoder(args)
    man = synth.state_dict_manifest(mod.state_dict())
    sd = synth.seeded_state_dict(man, SEED)
    mod.load_state_dict(sd, strict=True)
    mod = mod.eval()
    meta = {"vitdec.keys": np.array(list(man.keys())), "vitdec.shapes": np.array([json.dumps(list(s)) for s in man.values()]),
            "vitdec.seed": np.array(SEED), "vitdec.sha256": np.array(sha(sd)), "vitdec.config": np.array(json.dumps(args))}

    calls = {}
    hooks = []
    for kind, blocks in (("self", mod.self_attn_blocks), ("cross", mod.cross_attn_blocks)):
        for i, blk in enumerate(blocks):
            hooks.append(blk.register_forward_hook(
                lambda m, a, kw, out, key=(kind, i): calls.setdefault(key, []).append(
                    (kw["x"].detach().clone(), None if kw.get("key") is None else kw["key"].detach().clone(), out.detach().clone())),
                with_kwargs=True))
    head = {}
    hooks.append(mod.proj.register_forward_hook(lambda m, inp, out: head.update(tokens=inp[0].detach().clone(), proj=out.detach().clone())))
    hooks.append(mod.upsampler0.register_forward_hook(lambda m, inp, out: head.update(upsampler0=out.detach().clone())))
    hooks.append(mod.upsampler1.register_forward_hook(lambda m, inp, out: head.update(upsampler1=out.detach().clone())))

    g = torch.Generator().manual_seed(2027)
    xa = [torch.randn(1, 3, 24, 768, generator=g) for _ in range(3)]
    xb = [torch.randn(2, 2, 15, 768, generator=g) * s for s in (1.0, 30.0, 30.0)]
    with torch.no_grad():
        oa = mod(xa, vit_shape=[1, 3, 4, 6, 768])
        a_in = dict(meta)
        a_ref, a_src, a_head = {}, {}, {}
        for i in range(3):
            a_in["a/x%d" % i] = xa[i]
        for i in range(2):
            assert len(calls[("self", i)]) == 1 and calls[("self", i)][0][1] is None
            a_ref["a/ref/blk%d_in" % i], _, a_ref["a/ref/blk%d_out" % i] = calls[("self", i)][0]
        for i in range(3):
            assert len(calls[("cross", i)]) == 2                      # source views 1 and 2
            a_src["a/src/blk%d_in" % i], key, a_src["a/src/blk%d_out" % i] = calls[("cross", i)][0]
            if i == 0:
                assert torch.equal(key, xa[0][:, 0])                  # ref_feat_list[0] is the raw level-0 input of view 0
            else:
                a_ref["a/ref/feat%d" % i] = key                       # the AAS-normalised reference feature
        # proj's input is [B V, 768, h, w]: store it token-major [B V, h w, 768]
        a_head["a/tokens"] = head["tokens"].permute(0, 2, 3, 1).reshape(3, 24, 768).contiguous()
        a_head["a/proj"], a_head["a/upsampler0"], a_head["a/upsampler1"] = head["proj"], head["upsampler0"], head["upsampler1"]
        assert torch.equal(oa, head["upsampler1"])
        ob = mod(xb, vit_shape=[2, 2, 3, 5, 768])
        b = {"b/x%d" % i: xb[i] for i in range(3)}
        b["b/out"] = ob
    for hk in hooks:
        hk.remove()
    for name, d in (("f27_vitdec_a_in.npz", a_in), ("f27_vitdec_a_ref.npz", a_ref), ("f27_vitdec_a_src.npz", a_src),
                    ("f27_vitdec_a_head.npz", a_head), ("f27_vitdec_b.npz", b)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (name, size)
        print("%s: %d bytes, %d arrays" % (name, size, len(d)))


if __name__ == "__main__":
    main()
