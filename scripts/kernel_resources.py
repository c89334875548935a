#!/usr/bin/env python3
"""Per-kernel resource report (VGPRs, AGPRs, scratch, static LDS, waves/SIMD) from the compiler's kernel-resource-usage remarks.

mvsformerplusplus_amd/build.py compiles every translation unit with -Rpass-analysis=kernel-resource-usage and keeps each unit's
log in mvsformerplusplus_amd/csrc/.kernel_resources/<unit>.log (untracked).  This script reads those logs:

    scripts/kernel_resources.py [--units PREFIX] [name filter]           the library that was built last
    scripts/kernel_resources.py --logs DIR [--units PREFIX] [filter]     another build's logs
    scripts/kernel_resources.py --diff OLD NEW [--units PREFIX]          every kernel whose waves/SIMD or scratch changed between two log folders
    scripts/kernel_resources.py <file.hip> [name filter] [hipcc flags]   compile ONE unit now (scratch experiments) and report it

--units keeps the logs whose file name starts with PREFIX (gather_lds = the six units of the LDS-staged gather)."""
import argparse
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _demangle import demangle_mvs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = os.path.join(ROOT, "mvsformerplusplus_amd", "csrc", ".kernel_resources")
FIELDS = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r" AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def pretty(symbol):
    name = demangle_mvs(symbol)
    if name == symbol and symbol.startswith("_Z"):
        try:
            name = subprocess.run(["c++filt", symbol], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip() or symbol
        except OSError:
            pass
    return re.sub(r"\(.*", "", name).replace("void mvs::", "").replace("mvs::", "")


def parse(text, unit=""):
    """-> [{"symbol", "name", "unit", "vgpr", "agpr", "sgpr", "scratch", "occ", "lds"}] in the order of the remarks."""
    rows, cur = [], None
    for line in text.splitlines():
        if "kernel-resource-usage" not in line:
            continue
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"symbol": m.group(1), "unit": unit, "agpr": 0, "scratch": 0, "lds": 0}
            rows.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    for r in rows:
        r["name"] = pretty(r["symbol"])
    return rows


def load(folder, units=""):
    """Every kernel of the logs in `folder` (a file is read as one log), keyed by symbol."""
    files = [folder] if os.path.isfile(folder) else sorted(glob.glob(os.path.join(folder, units + "*.log")))
    out = {}
    for f in files:
        for r in parse(open(f, errors="replace").read(), os.path.basename(f)[:-4]):
            out[r["symbol"]] = r
    return out


def line(r):
    return "%-64s vgpr %3d agpr %3d scratch %4d lds %6d waves/SIMD %d" % (r["name"][:64], r.get("vgpr", -1), r["agpr"], r["scratch"], r["lds"], r.get("occ", -1))


def report(rows, flt=""):
    for r in rows:
        if not flt or flt in r["name"] or flt in r["symbol"]:
            print(line(r))


def diff(old, new, units=""):
    a, b = load(old, units), load(new, units)
    fewer, scratch, changed = [], [], []
    for sym, rb in b.items():
        ra = a.get(sym)
        if ra is None:
            continue
        if ra.get("occ") != rb.get("occ") or ra["scratch"] != rb["scratch"]:
            changed.append((ra, rb))
        if rb.get("occ", 0) < ra.get("occ", 0):
            fewer.append(rb)
        if rb["scratch"] > 0 and ra["scratch"] == 0:
            scratch.append(rb)
    print("# %d kernels in both (%d only old, %d only new); %d changed waves/SIMD or scratch" %
          (len(set(a) & set(b)), len(set(a) - set(b)), len(set(b) - set(a)), len(changed)))
    for ra, rb in changed:
        print("%-56s [%s]" % (rb["name"][:56], rb["unit"]))
        print("    old  vgpr %3d agpr %3d scratch %4d lds %6d waves/SIMD %d" % (ra.get("vgpr", -1), ra["agpr"], ra["scratch"], ra["lds"], ra.get("occ", -1)))
        print("    new  vgpr %3d agpr %3d scratch %4d lds %6d waves/SIMD %d" % (rb.get("vgpr", -1), rb["agpr"], rb["scratch"], rb["lds"], rb.get("occ", -1)))
    same = sum(1 for s in set(a) & set(b) if all(a[s].get(k) == b[s].get(k) for k, _ in FIELDS))
    print("# identical counts (vgpr, agpr, sgpr, scratch, lds, waves): %d kernels" % same)
    print("# fewer waves/SIMD than old: %d%s" % (len(fewer), "".join("\n#   " + r["name"] for r in fewer)))
    print("# scratch where old had none: %d%s" % (len(scratch), "".join("\n#   " + r["name"] for r in scratch)))
    return 1 if fewer or scratch else 0


def compile_one(src, flt, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-Wno-unused-value", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull] + extra
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    if "error:" in out:
        print(out)
        return 1
    report(parse(out, os.path.basename(src)), flt)
    return 0


def main(argv):
    if argv and argv[0].endswith(".hip"):
        flt = argv[1] if len(argv) > 1 and not argv[1].startswith("-") else ""
        return compile_one(argv[0], flt, [a for a in argv[1:] if a.startswith("-")])
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--diff", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--logs", default=LOGS)
    ap.add_argument("--units", default="")
    ap.add_argument("filter", nargs="?", default="")
    a = ap.parse_args(argv)
    if a.diff:
        return diff(a.diff[0], a.diff[1], a.units)
    rows = load(a.logs, a.units)
    if not rows:
        print("no resource logs in %s: build the library first (python -m mvsformerplusplus_amd.build --force)" % a.logs, file=sys.stderr)
        return 1
    report(rows.values(), a.filter)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
