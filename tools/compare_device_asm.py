#!/usr/bin/env python3
"""Has a kernel's device code changed?  Two gfx950 assembly files of the same source at two commits
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -S --cuda-device-only FILE.hip -o FILE.s), compared kernel by
kernel: the body between a kernel's label and its .Lfunc_end, comments stripped and the local labels (.LBBn_m, whose n
is the kernel's position in the file) renumbered in order of appearance.  Prints one line a kernel; exit status 1 if a
kernel both files have differs.
    python tools/compare_device_asm.py parent.s new.s"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z[^\n:]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        ids = {}
        body = re.sub(r'\s*;.*', '', m.group(2))
        body = re.sub(r'\.LBB\d+_\d+', lambda l: ids.setdefault(l.group(0), '.L%d' % len(ids)), body)
        out[m.group(1)] = [line for line in body.splitlines() if line.strip()]
    return out


def pretty(name):
    text = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(covest::.*", "", text).replace("covest::(anonymous namespace)::", "").replace("void ", "")


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
differs = False
for name in sorted(set(old) | set(new), key=pretty):
    if name not in new:
        print("%-40s only in %s" % (pretty(name), sys.argv[1]))
    elif name not in old:
        print("%-40s %6d lines, only in %s" % (pretty(name), len(new[name]), sys.argv[2]))
    else:
        same = old[name] == new[name]
        differs = differs or not same
        print("%-40s %6d lines, %s" % (pretty(name), len(old[name]), "identical" if same else
                                        "DIFFERENT (%d lines now)" % len(new[name])))
sys.exit(1 if differs else 0)
