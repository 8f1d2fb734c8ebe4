#!/usr/bin/env python3
"""Compare the kernels' instruction streams of two builds' device assembly (the rollout units' .s
files beside their objects): for every kernel symbol whose demangled name matches --match, the body
between its label and its .Lfunc_end, with labels renumbered and comments dropped.

usage: kernel_bodies_diff.py PARENT_OBJ_DIR BRANCH_OBJ_DIR [--match SUBSTRING] [--glob 'fr_coop*.s']

Prints one line per kernel (same / DIFFERENT, instruction counts) and a summary; exit status 1 when a
matched kernel differs or is missing on either side."""
import argparse
import glob
import os
import re
import subprocess
import sys


def kernels(path):
    """{symbol: [instruction lines]} of the .s file's amdgpu kernels."""
    out, cur, name = {}, None, None
    kern = set()
    lines = open(path).read().splitlines()
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kern.add(m.group(1))
    for ln in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and m.group(1) in kern:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end", ln):
            out[name] = cur
            cur = None
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            if s.startswith(".L") and s.endswith(":"):
                cur.append("<label>")
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
    return out


def demangle(names):
    if not names:
        return {}
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.splitlines()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--match", default="")
    ap.add_argument("--glob", default="fr_coop*.s")
    a = ap.parse_args()
    bad = same = 0
    for pf in sorted(glob.glob(os.path.join(a.parent, a.glob))):
        bf = os.path.join(a.branch, os.path.basename(pf))
        if not os.path.exists(bf):
            print("%s: missing in the branch" % os.path.basename(pf))
            bad += 1
            continue
        kp, kb = kernels(pf), kernels(bf)
        dm = demangle(sorted(set(kp) | set(kb)))
        for sym in sorted(set(kp) | set(kb)):
            if a.match and a.match not in dm.get(sym, sym):
                continue
            if sym not in kp or sym not in kb:
                print("%s: %s only on one side" % (os.path.basename(pf), dm.get(sym, sym)))
                bad += 1
                continue
            eq = kp[sym] == kb[sym]
            same += eq
            bad += not eq
            print("%s: %-9s %6d / %6d  %s" % (os.path.basename(pf), "same" if eq else "DIFFERENT", len(kp[sym]), len(kb[sym]),
                                              dm.get(sym, sym)))
    print("%d kernels the same, %d different or missing" % (same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
