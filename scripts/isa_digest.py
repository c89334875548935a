#!/usr/bin/env python3
"""Digest of the gfx950 device assembly of every csrc/*.hip.  No GPU needed.

    python scripts/isa_digest.py                      sha256  kernels  lines  file
    python scripts/isa_digest.py --against OTHER_TREE  the same for both trees + identical / DIFFERENT per file; exit status 1 if any differs

Each unit is compiled with build.FLAGS + build.FILE_FLAGS[file] + `--cuda-device-only -S`.  Lines that contain `__hip_cuid_`
are dropped: that symbol is random per compilation and is the only thing in which two compilations of one source differ.  The
assembly carries no line information, so a refactor that leaves the device code alone leaves every digest alone.
"""
import argparse
import glob
import hashlib
import importlib.util
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_isa_build", os.path.join(tree, "mvsformerplusplus_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest_one(job):
    b, src = job
    cmd = [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(os.path.basename(src), []) + ["--cuda-device-only", "-S", src, "-o", "-"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), p.stderr.decode()))
    lines = [l for l in p.stdout.split(b"\n") if b"__hip_cuid_" not in l]
    kernels = sum(1 for l in lines if l.lstrip().startswith(b".amdhsa_kernel"))
    return os.path.basename(src), (hashlib.sha256(b"\n".join(lines)).hexdigest(), kernels, len(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--against", metavar="TREE", help="another checkout of this repository to compare with")
    ap.add_argument("-j", type=int, default=16, help="compilations at a time (at most 16)")
    args = ap.parse_args()
    trees = [ROOT] + ([os.path.abspath(args.against)] if args.against else [])
    builds = [load_build(t) for t in trees]
    jobs = [(b, s) for b in builds for s in sorted(glob.glob(os.path.join(b.CSRC, "*.hip")))]
    with ThreadPoolExecutor(max(1, min(args.j, 16))) as ex:
        done = list(ex.map(digest_one, jobs))
    res = [dict(d for (jb, _), d in zip(jobs, done) if jb is b) for b in builds]
    same = 0
    for f in sorted(set().union(*res)):
        for r, tree in zip(res, ("", "  (other tree)")):
            print(("%s  %4d  %7d  %s" % (r[f] + (f,)) if f in r else "%-64s  %4s  %7s  %s" % ("(absent)", "-", "-", f)) + tree)
        if args.against:
            same += res[0].get(f) == res[1].get(f)
            print("    -> %s" % ("identical" if res[0].get(f) == res[1].get(f) else "DIFFERENT"))
    if args.against:
        print("%d of %d translation units identical" % (same, len(set().union(*res))))
        return 0 if same == len(set().union(*res)) else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
