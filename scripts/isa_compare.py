#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device assembly of two checkouts: what a refactor must leave alone.  No GPU needed.

    python scripts/isa_compare.py --against PARENT_TREE [--keep DIR] [unit.hip ...]

Every csrc/*.hip (or the named units) of both trees is compiled as scripts/isa_digest.py compiles it.  Per unit: identical or DIFFERENT
(the digest of the assembly without its `__hip_cuid_` lines).  Per kernel of a differing unit: whether its text, its resources (VGPRs,
AGPRs, SGPRs, scratch, LDS, waves/SIMD: scripts/kernel_resources.py) and its per-mnemonic instruction counts are the parent's; every
kernel whose resources or counts differ is listed with both sides.  Exit status 1 if any kernel's resources or counts differ."""
import argparse
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402
from isa_digest import ROOT, load_build  # noqa: E402


def compile_unit(job):
    b, unit, out = job
    cmd = [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(unit, []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, unit), "-o", os.path.join(out, unit[:-4] + ".s")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), p.stdout.decode()))
    with open(os.path.join(out, unit[:-4] + ".log"), "w") as f:
        f.write(p.stdout.decode())


def kernels(lines):
    """symbol -> (Counter of mnemonics, the function's lines)"""
    out, cur = {}, None
    for l in lines:
        m = re.match(r"^([A-Za-z_]\w*):", l)
        if m:
            cur = m.group(1)
            out[cur] = (collections.Counter(), [])
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
            continue
        out[cur][1].append(l)
        m = re.match(r"^\t([a-z_0-9]+)", l)
        if m and not l.startswith("\t."):
            out[cur][0][m.group(1)] += 1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--against", metavar="TREE", required=True, help="the parent checkout")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly and the compiler logs under DIR/parent and DIR/child")
    ap.add_argument("units", nargs="*")
    a = ap.parse_args()
    top = a.keep or tempfile.mkdtemp(prefix="isa_compare_")
    trees = {"parent": load_build(os.path.abspath(a.against)), "child": load_build(ROOT)}
    units = a.units or sorted(os.path.basename(s) for s in glob.glob(os.path.join(trees["child"].CSRC, "*.hip")))
    for who in trees:
        os.makedirs(os.path.join(top, who), exist_ok=True)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(compile_unit, [(b, u, os.path.join(top, who)) for who, b in trees.items() for u in units]))
    same_units, bad = 0, 0
    for u in units:
        text, res = {}, {}
        for who in trees:
            text[who] = [l for l in open(os.path.join(top, who, u[:-4] + ".s")).read().split("\n") if "__hip_cuid_" not in l]
            res[who] = {r["symbol"]: r for r in KR.parse(open(os.path.join(top, who, u[:-4] + ".log")).read(), u)}
        if text["parent"] == text["child"]:
            same_units += 1
            print("%-36s identical  %d lines" % (u, len(text["child"])))
            continue
        print("%-36s DIFFERENT  parent %d lines, child %d lines" % (u, len(text["parent"]), len(text["child"])))
        ka, kb = kernels(text["parent"]), kernels(text["child"])
        if set(res["parent"]) != set(res["child"]):
            print("    kernels only in one tree: %s" % sorted(set(res["parent"]) ^ set(res["child"])))
            bad += 1
        n = collections.Counter()
        for sym, rb in res["child"].items():
            ra = res["parent"].get(sym)
            if ra is None:
                continue
            res_same = all(ra.get(k) == rb.get(k) for k, _ in KR.FIELDS)
            ha, hb = ka[sym][0], kb[sym][0]
            n["text"] += ka[sym][1] == kb[sym][1]
            n["res"] += res_same
            n["ops"] += ha == hb
            if res_same and ha == hb:
                continue
            bad += 1
            print("    %s" % rb["name"])
            if not res_same:
                for who, r in (("parent", ra), ("child ", rb)):
                    print("        %s %s sgpr %d" % (who, KR.line(r)[65:], r.get("sgpr", -1)))
            for op in sorted(set(ha) | set(hb)):
                if ha[op] != hb[op]:
                    print("        %-24s parent %5d  child %5d" % (op, ha[op], hb[op]))
            print("        %-24s parent %5d  child %5d" % ("all instructions", sum(ha.values()), sum(hb.values())))
        print("    %d kernels: %d with the parent's text, %d with the parent's resources, %d with the parent's per-mnemonic counts"
              % (len(res["child"]), n["text"], n["res"], n["ops"]))
    print("%d of %d translation units identical; %d kernels differ in resources or instruction counts" % (same_units, len(units), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
