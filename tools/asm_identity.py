#!/usr/bin/env python3
"""tools/asm_identity.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...] [-v]

Compare the gfx950 kernels of two sets of device assembly files (hipcc <the file's Makefile
flags> --cuda-device-only -S FILE.hip -o FILE.s), for moves and refactors that must not change
device code (profiles/r13/asm_identity.txt). Kernels are matched by demangled name; labels,
mangled symbol names and assembler comments are normalised; the instruction text and the
.amdhsa_* descriptor (VGPRs, SGPRs, LDS, scratch, wave limits) of every kernel are compared.
Only kernels are compared: a device function that is not inlined is emitted outside its
callers' bodies and is not looked at (this project's device helpers are all forceinline).
Exit status 1 when a kernel differs or exists on one side only."""
import collections
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(path):
    """-> ({mangled kernel: body lines}, {mangled kernel: descriptor lines})"""
    lines = open(path).read().split("\n")
    kernels = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    body, desc, cur, i = {}, {}, None, 0
    while i < len(lines):
        l = lines[i]
        m = re.match(r"^(\S+):\s*(;.*)?$", l)
        if m and m.group(1) in kernels and cur is None:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            if re.match(r"\s*\.Lfunc_end\d+:", l):
                cur = None
            else:
                body[cur].append(l)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            d = []
            i += 1
            while not re.match(r"\s*\.end_amdhsa_kernel", lines[i]):
                d.append(lines[i].strip())
                i += 1
            desc[m.group(1)] = d
        i += 1
    return body, desc


def normalise(lines, names):
    labels = {}
    out = []
    for l in lines:
        s = l.split(";")[0].strip()
        if not s or re.match(r"\.(loc|file|cfi|section|type|size|globl|protected|weak|set|text)", s):
            continue
        s = re.sub(r"\.LBB\d+_\d+|\.Ltmp\d+|\.LJTI\d+_\d+|\.L__unnamed_\d+",
                   lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), s)
        s = re.sub(r"_Z[\w$.]+", lambda m: names.get(m.group(0), m.group(0)), s)
        out.append(re.sub(r"__hip_cuid_\w+", "CUID", s))
    return out


def load(paths):
    parsed = [(p,) + parse(p) for p in paths]
    syms = set()
    for p in paths:
        for l in open(p):
            syms.update(re.findall(r"_Z[\w$.]+", l))
    names = demangle(sorted(syms))
    kernels = {}
    for p, body, desc in parsed:
        for k in desc:
            assert names[k] not in kernels, ("kernel in two files", names[k])
            kernels[names[k]] = (normalise(body[k], names), desc[k], p)
    return kernels


def main():
    old, new = load(sys.argv[1].split(",")), load(sys.argv[2].split(","))
    print("parent %d kernels, new %d" % (len(old), len(new)))
    for p, c in sorted(collections.Counter(v[2] for v in new.values()).items()):
        print("  %s: %d kernels" % (p, c))
    one_side = sorted(set(old) ^ set(new))
    for n in one_side:
        print("  only in %s: %s" % ("parent" if n in old else "new", n))
    same = diff = 0
    for n in sorted(set(old) & set(new)):
        if old[n][:2] == new[n][:2]:
            same += 1
            continue
        diff += 1
        if "-v" in sys.argv or diff <= 8:
            what = [w for w, i in (("text", 0), ("descriptor", 1)) if old[n][i] != new[n][i]]
            print("  different (%s): %s" % (", ".join(what), n))
    print("compared %d, identical %d, different %d" % (same + diff, same, diff))
    return 1 if diff or one_side else 0


if __name__ == "__main__":
    sys.exit(main())
