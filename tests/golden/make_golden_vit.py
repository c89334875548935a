#!/usr/bin/env python3
"""Generate fixture F28 (tests/golden/f28_vit_*.npz) by RUNNING the reference's own DINOv2 ViT (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vit.py

Module: models/dino/dinov2.py vit_base(img_size=518, patch_size=14, init_values=1.0, block_chunks=0, ffn_layer="mlp", **dino_cfg) with the
dino_cfg of config/mvsformer++.json, eval mode, fp32, CPU, forward_interval_features.  Weights: synth.seeded_state_dict over the
reference module's manifest, with ONE override: synth gives pos_embed a standard deviation of 0.0014 (its fan-in rule) and a small
cls_token, so the position embedding would not matter and a wrong interpolation would pass; both are replaced by seeded N(0, 1) values.
The manifest, the seed, the override, the config and the SHA-256 of the final state dict are stored IN the fixture ("vit." prefix).

Cases (every tensor fp32; each file stays under 1 MiB):
  case a = 3 views of 4 x 6 patches (56 x 84 images, 25 tokens)
    f28_vit_a_in.npz       manifest; the images; the tokens after prepare_tokens_with_masks
    f28_vit_a_blk{0,3,7,11}.npz   input and output tokens of that block (forward hooks)
    f28_vit_a_out.npz      the three levels
  case b = 2 views of 5 x 3 patches (70 x 42 images: TALL, 16 tokens)
    f28_vit_b.npz          images, tokens, the three levels
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

from models.dino.dinov2 import vit_base  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

SEED, OVERRIDE_SEED = 28, 2828
BLOCKS = (0, 3, 7, 11)


def sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def weights(manifest):
    """The fixture's state dict: synth's seeded weights with pos_embed and cls_token replaced by seeded N(0, 1) values."""
    sd = synth.seeded_state_dict(manifest, SEED)
    g = torch.Generator().manual_seed(OVERRIDE_SEED)
    for key in ("pos_embed", "cls_token"):
        sd[key] = torch.randn(tuple(manifest[key]), generator=g)
    return sd


def main():
    torch.manual_seed(0)
    dino_cfg = json.load(open(os.path.join(REF, "config", "mvsformer++.json")))["arch"]["args"]["dino_cfg"]
    kwargs = dict(img_size=518, patch_size=14, init_values=1.0, block_chunks=0, ffn_layer="mlp")
    mod = vit_base(**kwargs, **dino_cfg)
    man = synth.state_dict_manifest(mod.state_dict())
    sd = weights(man)
    mod.load_state_dict(sd, strict=True)
    mod = mod.eval()
    cfg = dict(kwargs, **{k: v for k, v in dino_cfg.items() if k != "decoder_cfg"})
    meta = {"vit.keys": np.array(list(man.keys())), "vit.shapes": np.array([json.dumps(list(s)) for s in man.values()]),
            "vit.seed": np.array(SEED), "vit.override_seed": np.array(OVERRIDE_SEED), "vit.override_keys": np.array(["pos_embed", "cls_token"]),
            "vit.sha256": np.array(sha(sd)), "vit.config": np.array(json.dumps(cfg))}

    calls = {}
    hooks = [mod.blocks[i].register_forward_hook(lambda m, a, out, i=i: calls.setdefault(i, []).append((a[0].detach().clone(), out.detach().clone())))
             for i in BLOCKS]
    g = torch.Generator().manual_seed(2028)
    xa = torch.randn(3, 3, 56, 84, generator=g)
    xb = torch.randn(2, 3, 70, 42, generator=g)
    files = {}
    with torch.no_grad():
        la = mod.forward_interval_features(xa)
        a_in = dict(meta)
        a_in["a/img"], a_in["a/tokens"] = xa, mod.prepare_tokens_with_masks(xa)
        files["f28_vit_a_in.npz"] = a_in
        for i in BLOCKS:
            assert len(calls[i]) == 1
            files["f28_vit_a_blk%d.npz" % i] = {"a/blk%d_in" % i: calls[i][0][0], "a/blk%d_out" % i: calls[i][0][1]}
        assert len(la) == 3 and tuple(la[0].shape) == (3, 24, 768)
        files["f28_vit_a_out.npz"] = {"a/level%d" % i: t.contiguous() for i, t in enumerate(la)}
        lb = mod.forward_interval_features(xb)
        b = {"b/img": xb, "b/tokens": mod.prepare_tokens_with_masks(xb)}
        assert len(lb) == 3 and tuple(lb[0].shape) == (2, 15, 768)
        b.update({"b/level%d" % i: t.contiguous() for i, t in enumerate(lb)})
        files["f28_vit_b.npz"] = b
    for hk in hooks:
        hk.remove()
    for name, d in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (name, size)
        print("%s: %d bytes, %d arrays" % (name, size, len(d)))


if __name__ == "__main__":
    main()
