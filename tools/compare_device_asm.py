#!/usr/bin/env python3
"""Has a kernel's device code changed?  Two gfx950 assembly files of the same source at two commits
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -S --cuda-device-only FILE.hip -o FILE.s), compared kernel by
kernel: the body between a kernel's label and its .Lfunc_end, comments stripped and the local labels (.LBBn_m, whose n
is the kernel's position in the file) renumbered in order of appearance, the kernel's own name replaced; and the registers, scratch, LDS and occupancy
of the "Kernel info" block behind it.  Prints one line a kernel; exit status 1 if a kernel both files have differs in
either.  --as OLD=NEW (names as printed) compares a kernel that was renamed; such a pair's instructions may differ (the
count of differing lines is printed) and it fails only where the new one takes more registers or scratch.
    python tools/compare_device_asm.py parent.s new.s [--as 'batch_pairs_grad_kernel<3>=batch_pairs_kernel<3>' ...]"""
import difflib
import re
import subprocess
import sys

RESOURCES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
MAY_NOT_GROW = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize")


def pretty(name):
    text = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*", "", text.replace("covest::(anonymous namespace)::", "").replace("void ", ""))  # (no arguments)


def kernels(path):
    """pretty name -> (instruction lines, resources)"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z[^\n:]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)^; COMPUTE_PGM_RSRC2', text, re.S | re.M):
        ids = {}
        body = re.sub(r'\s*;.*', '', m.group(2)).replace(m.group(1), "KERNEL")  # (its own name: a renamed kernel's differs)
        body = re.sub(r'\.LBB\d+_\d+', lambda l: ids.setdefault(l.group(0), '.L%d' % len(ids)), body)
        res = {k: int(v) for k, v in re.findall(r'^; (\w+): (\d+)', m.group(3), re.M) if k in RESOURCES}
        out[pretty(m.group(1))] = ([line for line in body.splitlines() if line.strip()], res)
    return out


def resources(res):
    return "vgpr %d agpr %d sgpr %d scratch %d lds %d occ %d" % tuple(res.get(k, -1) for k in RESOURCES)


args = sys.argv[1:]
renamed = {}
while "--as" in args:
    at = args.index("--as")
    old_name, new_name = args[at + 1].split("=", 1)
    renamed[old_name] = new_name
    del args[at:at + 2]
old, new = kernels(args[0]), kernels(args[1])
differs = False
for old_name, new_name in renamed.items():
    (a, ra), (b, rb) = old.pop(old_name), new.pop(new_name)
    changed = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
                  if tag != "equal")
    grew = [k for k in MAY_NOT_GROW if rb[k] > ra[k]]
    differs = differs or bool(grew)
    print("%-40s %6d lines -> %s %d lines, %s; %s -> %s%s" % (old_name, len(a), new_name, len(b),
          "identical" if a == b else "%d lines differ" % changed, resources(ra), resources(rb),
          "; MORE %s" % ", ".join(grew) if grew else ""))
for name in sorted(set(old) | set(new)):
    if name not in new:
        print("%-40s only in %s" % (name, args[0]))
    elif name not in old:
        print("%-40s %6d lines, only in %s; %s" % (name, len(new[name][0]), args[1], resources(new[name][1])))
    else:
        same, same_res = old[name][0] == new[name][0], old[name][1] == new[name][1]
        differs = differs or not (same and same_res)
        print("%-40s %6d lines, %s; %s%s" % (name, len(old[name][0]), "identical" if same else
                                             "DIFFERENT (%d lines now)" % len(new[name][0]), resources(old[name][1]),
                                             "" if same_res else " -> NOW " + resources(new[name][1])))
sys.exit(1 if differs else 0)
