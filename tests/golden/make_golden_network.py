#!/usr/bin/env python3
"""Generate fixture F29 (tests/golden/f29_network_*.npz, f29_network_args.json) by RUNNING the reference's own top-level network (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_network.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_network.py --check    # + patch_all on the same model, host emulator

Module: models/networks/DINOv2_mvsformer_model.py DINOv2MVSNet with the arch.args of config/mvsformer++.json (stored as the settings-only
f29_network_args.json; cases b and c change `rescale` alone), eval mode, fp32, CPU.  Weights: synth.seeded_state_dict over ALL 779 keys of
the reference model's manifest (LayerScale gammas and prev_values take its generic N(0, 2) branch: a fair stress, as in F26 - F28), with
two overrides (OVERRIDES below, stored in the fixture as JSON):
  vit.pos_embed, vit.cls_token      seeded N(0, 1), as in F28 (synth's fan-in rule gives the position table a standard deviation of 0.0014:
                                    it would not matter and a wrong interpolation would pass)
  FMT_module.dim_reduction_k.weight synth's draw x 0.7071, FMT_module.smooth_k.weight synth's draw x 0.2.  The pathway is linear (no
                                    activation between its convolutions), so synth's He draw doubles the features per level: stage 2 - 4
                                    features reach 35 / 73 / 146, the correlations their squares, and the U-Nets' logits (eval BatchNorm with
                                    seeded statistics does not normalise) put 0.98 - 0.999 of every pixel's probability on ONE hypothesis.
                                    Depth is then an argmax: the drop-ins' 1e-5 feature error flips pixels between hypotheses (measured:
                                    6e-3 relative depth, 0.16 confidence at stage 3 of case a) and nothing of the regression is tested.
                                    With the override the four stages' features are 22 / 5.5 / 2.1 / 2.9 and the mean top probability is
                                    0.05 / 0.40 / 0.19 / 0.45.
The manifest, the seeds, the override rule and the SHA-256 of the final state dict are stored IN the fixture ("net." prefix).

Cases (imgs = seeded U(0, 1); cameras = synth.make_cameras(V, H, W, baseline=30, rot_deg=1) + stage_proj_matrices; depth_values =
arange(425, 425 + 2.65 * 191.5, 2.65)):
  a  64 x 64,  V = 3, rescale 0.4375   bicubic -> 28 x 28;              ViT feature map 8 x 8 = conv31's size: the plain add
  b  96 x 128, V = 3, rescale 0.3      bicubic -> 28 x 28 (anisotropic, more than 3 x down);   8 x 8 -> 12 x 16 (up)
  c  32 x 64,  V = 2, rescale 1.0      bicubic -> 28 x 56;              8 x 16 -> 4 x 8 (down)
Recorded per case under "<case>/": imgs, proj.stageK, depth_values, vit_imgs (the bicubic output), conv31 (after the add, all views),
feat.stageK (the four FMT outputs), stageK.depth / stageK.conf, refined_depth, photometric_confidence, out_names.  Arrays are packed
greedily into files below 1 MiB; an array too large for one file is split along its view axis ("<key>#<part>", rejoined by the loader in
tests/test_network.py).
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
sys.path.insert(2, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import torch  # noqa: E402

from models.networks.DINOv2_mvsformer_model import DINOv2MVSNet  # noqa: E402  (reference)
from mvsformerplusplus_amd import synth  # noqa: E402

SEED, OVERRIDE_SEED = 29, 2929
CASES = {"a": dict(H=64, W=64, V=3, rescale=0.4375, seed=291), "b": dict(H=96, W=128, V=3, rescale=0.3, seed=292),
         "c": dict(H=32, W=64, V=2, rescale=1.0, seed=293)}
FILE_BYTES = 1000000            # uncompressed payload per file: every file stays below 1 MiB


def sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


OVERRIDES = {"normal": ["vit.pos_embed", "vit.cls_token"],
             "scale": {"FMT_module.dim_reduction_": 0.7071, "FMT_module.smooth_": 0.2}}


def weights(manifest):
    """synth's seeded state dict with OVERRIDES applied; tests/test_network.py applies the same rule from the JSON stored in the fixture."""
    sd = synth.seeded_state_dict(manifest, SEED)
    g = torch.Generator().manual_seed(OVERRIDE_SEED)
    for key in OVERRIDES["normal"]:
        sd[key] = torch.randn(tuple(manifest[key]), generator=g)
    for key in manifest:
        for prefix, factor in OVERRIDES["scale"].items():
            if key.startswith(prefix):
                sd[key] = sd[key] * factor
    return sd


def case_inputs(c):
    H, W, V = c["H"], c["W"], c["V"]
    imgs = torch.rand(1, V, 3, H, W, generator=torch.Generator().manual_seed(c["seed"]))
    projs = synth.stage_proj_matrices(synth.make_cameras(V, H, W, baseline=30.0, rot_deg=1.0, seed=c["seed"]), 4)
    dv = torch.arange(425.0, 425.0 + 2.65 * 191.5, 2.65)[None]
    return imgs, projs, dv


def run_reference(model, imgs, projs, dv):
    """The reference forward with its intermediates: the ViT's input, every view's conv31 after the add, the FMT's outputs."""
    rec = {"conv31": []}
    vit_fwd, dec_fwd, fmt_fwd = model.vit.forward_interval_features, model.decoder.forward, model.FMT_module.forward

    # the network calls .forward / .forward_interval_features directly (no hooks fire): spies as instance attributes
    def vit_spy(x, *a, **k):
        rec["vit_imgs"] = x.detach().clone()
        return vit_fwd(x, *a, **k)

    def dec_spy(conv01, conv11, conv21, conv31):
        rec["conv31"].append(conv31.detach().clone())
        return dec_fwd(conv01, conv11, conv21, conv31)

    def fmt_spy(features):
        out = fmt_fwd(features)
        rec["feat"] = {k: v.detach().clone() for k, v in out.items()}
        return out

    model.vit.forward_interval_features, model.decoder.forward, model.FMT_module.forward = vit_spy, dec_spy, fmt_spy
    try:
        with torch.no_grad():
            out = model(imgs, projs, dv)
    finally:
        del model.vit.forward_interval_features, model.decoder.forward, model.FMT_module.forward
    rec["conv31"] = torch.cat(rec["conv31"], 0)
    return out, rec


def case_arrays(name, imgs, projs, dv, out, rec):
    p = name + "/"
    arrs = {p + "imgs": imgs, p + "depth_values": dv, p + "vit_imgs": rec["vit_imgs"], p + "conv31": rec["conv31"],
            p + "refined_depth": out["refined_depth"], p + "photometric_confidence": out["photometric_confidence"],
            p + "out_names": np.array(sorted(out.keys()))}
    for s in range(1, 5):
        k = "stage%d" % s
        arrs[p + "proj." + k] = projs[k]
        arrs[p + "feat." + k] = rec["feat"][k]
        arrs[p + k + ".depth"] = out[k]["depth"]
        arrs[p + k + ".conf"] = out[k]["photometric_confidence"]
    return {k: (v.contiguous().numpy() if torch.is_tensor(v) else v) for k, v in arrs.items()}


def write_files(arrs):
    for old in glob.glob(os.path.join(HERE, "f29_network_*.npz")):
        os.remove(old)
    items = []
    for k, v in arrs.items():
        if v.nbytes > FILE_BYTES:                         # [1, V, ...]: split along the views
            assert v.ndim >= 2 and v.shape[0] == 1 and v[:, :1].nbytes <= FILE_BYTES, (k, v.shape)
            items += [("%s#%d" % (k, i), np.ascontiguousarray(v[:, i:i + 1])) for i in range(v.shape[1])]
        else:
            items.append((k, v))
    files, cur, size = [], {}, 0
    for k, v in items:
        if cur and size + v.nbytes > FILE_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    files.append(cur)
    for i, d in enumerate(files):
        path = os.path.join(HERE, "f29_network_%02d.npz" % i)
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 1024 * 1024, (path, os.path.getsize(path))
        print("%s: %d bytes, %d arrays" % (os.path.basename(path), os.path.getsize(path), len(d)))


def check_patch_all(model, name, imgs, projs, dv, out, rec):
    """The condition on the fixture: the five native drop-ins composed by patch_all inside the reference's own forward, on the host
    emulator, hold the bars of tests/test_network.py on this case."""
    import hipemu_build
    from mvsformerplusplus_amd import _lib, patch_all
    if _lib._LIB is None:
        _lib._LIB = _lib.bind(hipemu_build.build())
        _lib._REQUIRE_DEVICE = False
    got, grec = run_reference(patch_all(model), imgs, projs, dv)
    worst_feat = 0.0
    for s in range(1, 5):
        k = "stage%d" % s
        want = rec["feat"][k]
        frac = float((grec["feat"][k] - want).abs().max() / (want.max() - want.min()))
        rel = (got[k]["depth"] - out[k]["depth"]).abs() / out[k]["depth"].abs()
        conf = float((got[k]["photometric_confidence"] - out[k]["photometric_confidence"]).abs().max())
        print("  %s %s: features %.3g of the range; depth rel max %.3g mean %.3g; confidence %.3g"
              % (name, k, frac, float(rel.max()), float(rel.mean()), conf))
        worst_feat = max(worst_feat, frac)
        assert frac <= 2e-4 and float(rel.max()) <= 1e-3 and conf <= 3e-2, (name, k)
    conf = float((got["photometric_confidence"] - out["photometric_confidence"]).abs().max())
    assert conf <= 3e-2, (name, conf)
    return worst_feat


def main():
    check = "--check" in sys.argv[1:]
    torch.manual_seed(0)
    torch.set_num_threads(16)
    args = json.load(open(os.path.join(REF, "config", "mvsformer++.json")))["arch"]["args"]
    with open(os.path.join(HERE, "f29_network_args.json"), "w") as f:
        json.dump(args, f, indent=1, sort_keys=True)
        f.write("\n")
    arrs, sd, man = {}, None, None
    for name, c in CASES.items():
        model = DINOv2MVSNet(dict(args, rescale=c["rescale"]))
        if sd is None:
            man = synth.state_dict_manifest(model.state_dict())
            sd = weights(man)
            n_par = sum(p.numel() for p in model.parameters())
            print("state dict: %d keys, %d parameters" % (len(man), n_par))
            assert len(man) == 779 and n_par == 126054413
        model.load_state_dict(sd, strict=True)
        model = model.eval()
        imgs, projs, dv = case_inputs(c)
        out, rec = run_reference(model, imgs, projs, dv)
        d = out["refined_depth"]
        print("case %s: vit_imgs %s, conv31 %s, depth %.1f .. %.1f, confidence mean %.3f" % (
            name, tuple(rec["vit_imgs"].shape), tuple(rec["conv31"].shape), float(d.min()), float(d.max()), float(out["photometric_confidence"].mean())))
        arrs.update(case_arrays(name, imgs, projs, dv, out, rec))
        arrs[name + "/rescale"] = np.array(c["rescale"])
        if check:
            check_patch_all(model, name, imgs, projs, dv, out, rec)
    arrs.update({"net.keys": np.array(list(man.keys())), "net.shapes": np.array([json.dumps(list(s)) for s in man.values()]),
                 "net.seed": np.array(SEED), "net.override_seed": np.array(OVERRIDE_SEED), "net.overrides": np.array(json.dumps(OVERRIDES)), "net.sha256": np.array(sha(sd)),
                 "net.parameters": np.array(126054413)})
    write_files(arrs)


if __name__ == "__main__":
    main()
