#!/usr/bin/env python3
"""Generate fixture F23 (tests/golden/f23_gipuma_formats.npz) by IMPORTING the reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gipuma.py

A 4-view 24x32 scene with uint8, float32 and float64 confidences, some exactly at the probability threshold (0.4 = 102 / 255 in
float64; float32(0.4) in float32), run through the reference's own misc/gipuma.py ``probability_filter`` and
``mvsnet_to_gipuma``.  ``depth_map_fusion`` / ``gipuma_filter`` are never run: they shell out to fusibile.

misc/gipuma.py imports ``datasets.data_io``, whose package __init__ needs torchvision; datasets/data_io.py is loaded by file
path and registered as ``datasets.data_io`` under a stub ``datasets`` package, then misc/gipuma.py is loaded by path.

What is committed is DATA: every input file's bytes ("in/<path>") and every file the reference wrote ("out/<path>": the
_prob_filtered.pfm depth maps, cams/*.P, images/, 2333__*/disp.dmb and normals.dmb), plus the threshold.
"""
import importlib.util
import os
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

PROB_THRESHOLD = 0.4


def load_reference():
    pkg = types.ModuleType("datasets")
    pkg.__path__ = []
    sys.modules["datasets"] = pkg
    spec = importlib.util.spec_from_file_location("datasets.data_io", os.path.join(REF, "datasets", "data_io.py"))
    dio = importlib.util.module_from_spec(spec)
    sys.modules["datasets.data_io"] = dio
    spec.loader.exec_module(dio)
    pkg.data_io = dio
    spec = importlib.util.spec_from_file_location("ref_gipuma", os.path.join(REF, "misc", "gipuma.py"))
    gip = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gip)
    return gip


def confidences(shape, g):
    c0 = g.integers(60, 160, shape).astype(np.uint8)
    c0[::3, ::2] = 102                                              # 102 / 255 == 0.4 in float64: dropped (strict >)
    c1 = g.integers(0, 256, shape).astype(np.uint8)
    c2 = g.uniform(0.2, 0.6, shape).astype(np.float32)
    c2[1::4] = np.float32(0.4)                                      # at the threshold in float32: dropped
    c2[2::4, ::3] = np.nextafter(np.float32(0.4), np.float32(1))    # one ulp above: kept
    c3 = g.uniform(0.2, 0.6, shape)
    c3[::5] = 0.4
    c3[1::5, ::2] = np.nextafter(0.4, 1.0)
    return [c0, c1, c2, c3]


def main():
    import gipuma_cases as GC
    gip = load_reference()
    sc = GC.make_scene(4, 24, 32, seed=23, outliers=0.1, holes=0.03)
    conf = confidences((24, 32), np.random.default_rng(23))
    arrays = {"prob_threshold": np.float64(PROB_THRESHOLD)}
    with tempfile.TemporaryDirectory() as tmp:
        dense = os.path.join(tmp, "scan")
        GC.write_scene_folder(dense, sc, conf)
        for dp, _, fs in os.walk(dense):
            for f in sorted(fs):
                p = os.path.join(dp, f)
                arrays["in/" + os.path.relpath(p, dense)] = np.frombuffer(open(p, "rb").read(), np.uint8)
        point = os.path.join(dense, "points_mvsnet")
        os.mkdir(point)
        gip.probability_filter(dense, PROB_THRESHOLD)
        gip.mvsnet_to_gipuma(dense, point)
        for dp, _, fs in os.walk(dense):
            for f in sorted(fs):
                rel = os.path.relpath(os.path.join(dp, f), dense)
                if "in/" + rel not in arrays:
                    arrays["out/" + rel] = np.frombuffer(open(os.path.join(dp, f), "rb").read(), np.uint8)
    out = os.path.join(HERE, "f23_gipuma_formats.npz")
    np.savez_compressed(out, **arrays)
    print("wrote %s: %d entries" % (out, len(arrays)))


if __name__ == "__main__":
    main()
