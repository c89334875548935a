#!/usr/bin/env python3
"""Generate fixture F24 (tests/golden/f24_colmap2mvsnet.npz) by RUNNING the reference's colmap2mvsnet.py (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_colmap.py

The script runs in this process through runpy with two shims that exist only here: ``np.asscalar = lambda a: a.item()`` (numpy
removed it in 1.23) and a stub ``cv2`` module (the cases never pass --convert_format).  Its inputs are synthetic models written as
.bin (mvsformerplusplus_amd.synth.make_colmap_model) and placeholder image files.

Cases: a 12-image model at defaults, in which every image shares points with at least 10 others; the same model with max_d = 0 and
interval_scale = 1.06; the same model with theta0 = 3, sigma1 = 2, sigma2 = 7; a 24-image model in which every pair shares points;
a sparse 9-image model in which most pairs share nothing (rows end in zero-score ties, compared as sets).

Asserted against the fp64 oracle (tests/colmap_ref.py), so that every listing is exact except for zero-score ties: no printed
%f value lies within 1e-9 of a rounding boundary; the positive scores listed in a row are distinct with relative gaps above 1e-9;
no listed positive score lies within 1e-9 (relative) of the score ranked 11th.

What is committed is DATA: every input file's bytes ("<case>/in/<path>"), every file the reference wrote ("<case>/out/<path>":
pair.txt and cams/*.txt), the source image names in output order ("<case>/names") and the arguments ("<case>/args").
"""
import json
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("MVS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from mvsformerplusplus_amd import colmap, synth                    # noqa: E402
from mvsformerplusplus_amd.colmap2mvsnet import inverse_depth_count  # noqa: E402
import colmap_ref as R                                              # noqa: E402

ALL_MODELS = tuple(colmap.PARAM_TYPE)
MODELS = {
    "m12": dict(n_images=12, n_points=700, seed=11, duplicates=0.03, invalid=0.03, camera_models=ALL_MODELS),
    "m24": dict(n_images=24, n_points=1500, seed=5, tail=0.7, max_track=24, camera_models=("SIMPLE_RADIAL", "OPENCV")),
    "m9s": dict(n_images=9, n_points=120, seed=4, window=1, max_track=3, duplicates=0.05, invalid=0.05, shared_camera=True,
                camera_models=("PINHOLE",)),
}
CASES = {
    "a12": ("m12", {}),
    "a12_maxd0": ("m12", {"max_d": 0, "interval_scale": 1.06}),
    "a12_theta": ("m12", {"theta0": 3.0, "sigma1": 2.0, "sigma2": 7.0}),
    "b24": ("m24", {}),
    "s9": ("m9s", {}),
}
DEFAULTS = {"max_d": 256, "interval_scale": 1.0, "theta0": 5.0, "sigma1": 1.0, "sigma2": 10.0}


def write_inputs(model, root):
    colmap.write_model(model, os.path.join(root, "sparse"), ".bin")
    os.makedirs(os.path.join(root, "images_col"))
    g = np.random.default_rng(0)
    for name in model.images.names:
        with open(os.path.join(root, "images_col", name), "wb") as f:
            f.write(b"\xff\xd8 placeholder " + name.encode() + g.integers(0, 256, 16, dtype=np.uint8).tobytes())


def run_reference(root, args):
    np.asscalar = lambda a: a.item()
    sys.modules["cv2"] = types.ModuleType("cv2")
    argv = sys.argv
    sys.argv = ["colmap2mvsnet.py", "--dense_folder", root] + sum([["--%s" % k, repr(v)] for k, v in args.items()], [])
    try:
        runpy.run_path(os.path.join(REF, "colmap2mvsnet.py"), run_name="__main__")
    finally:
        sys.argv = argv
        del np.asscalar
        del sys.modules["cv2"]


def boundary_ok(x):
    r = float(x) * 1e6
    return abs((r - np.floor(r)) - 0.5) * 1e-6 > 1e-9


def check_margins(case, model, a):
    S = R.scores(model, a["theta0"], a["sigma1"], a["sigma2"])
    n = S.shape[0]
    lo, hi = R.depth_bounds(model)
    E = colmap.extrinsics(model.images)
    for i in range(n):
        K = colmap.intrinsic(model.cameras[int(model.images.camera_ids[i])])
        num = inverse_depth_count(K, E[i], float(lo[i]), float(hi[i])) if a["max_d"] == 0 else a["max_d"]
        for v in (lo[i], (hi[i] - lo[i]) / (num - 1) / a["interval_scale"], num, hi[i]):
            assert boundary_ok(v), (case, i, v)
        row = np.sort(S[i])[::-1]
        top = row[:10]
        assert all(boundary_ok(v) for v in top), (case, i)
        pos = top[top > 0]
        assert np.all(np.diff(pos) < -1e-9 * pos[1:]), (case, i, pos)
        if n > 10 and len(pos):
            assert row[10] == 0 or pos[-1] - row[10] > 1e-9 * pos[-1], (case, i)
    off = (S > 0).sum(1)
    if case.startswith("a12"):
        assert off.min() >= 10, off
    if case == "b24":
        assert off.min() == n - 1, off
    if case == "s9":
        assert off.max() < n - 1 and off.min() >= 1, off


def main():
    out = {}
    for case, (mname, extra) in CASES.items():
        a = dict(DEFAULTS, **extra)
        model = synth.make_colmap_model(**MODELS[mname])
        check_margins(case, model, a)
        root = tempfile.mkdtemp()
        try:
            write_inputs(model, root)
            for d in ("sparse", "images_col"):
                for f in sorted(os.listdir(os.path.join(root, d))):
                    out["%s/in/%s/%s" % (case, d, f)] = np.frombuffer(open(os.path.join(root, d, f), "rb").read(), np.uint8)
            run_reference(root, {k: v for k, v in a.items() if k in extra})
            out["%s/out/pair.txt" % case] = np.frombuffer(open(os.path.join(root, "pair.txt"), "rb").read(), np.uint8)
            for f in sorted(os.listdir(os.path.join(root, "cams"))):
                out["%s/out/cams/%s" % (case, f)] = np.frombuffer(open(os.path.join(root, "cams", f), "rb").read(), np.uint8)
            for i, name in enumerate(model.images.names):
                assert open(os.path.join(root, "images", "%08d.jpg" % i), "rb").read() == \
                    open(os.path.join(root, "images_col", name), "rb").read()
            out["%s/names" % case] = np.frombuffer("\n".join(model.images.names).encode(), np.uint8)
            out["%s/args" % case] = np.frombuffer(json.dumps(a, sort_keys=True).encode(), np.uint8)
        finally:
            shutil.rmtree(root)
        print(case, "ok")
    path = os.path.join(HERE, "f24_colmap2mvsnet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
