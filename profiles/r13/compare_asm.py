#!/usr/bin/env python3
"""Gate A of profiles/r13: compare two gfx950 compiles of kernels.hip kernel by kernel.

Each side is one compile with the flags of osqp-solver_amd/build.py plus
  --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o SIDE.s 2> SIDE.remarks

usage: compare_asm.py PARENT.s NEW.s [PARENT.remarks NEW.remarks]

Normalised before the comparison, and nothing else:
  * iterate_kernel's mangled name: the parent's last template argument (RE = false) is dropped;
  * the per-function ordinal k of local labels (.LBB<k>_<n>, BB<k>_<n> in loop comments, .Lfunc_begin/end<k>, .LJTI<k>_<n>),
    which shifts when instantiations vanish, and the column of the comment behind a label, which moves with k's width;
  * the COMDAT `.section .text.<name>` line that closes a function's block: it names the NEXT function;
  * the __hip_cuid_* symbol."""
import collections
import difflib
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")


def norm_name(s):
    return re.sub(r"(_ZN6miosqp14iterate_kernelI(?:L[ib]\d+E){7})Lb0E(EEvNS_10KernelArgsE)", r"\1\2", s)


def norm_line(s):
    s = norm_name(s)
    s = re.sub(r"(?<![A-Za-z0-9_])(\.L)?BB\d+_", "BB#_", s)
    s = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", s)
    s = re.sub(r"\.LJTI\d+_", ".LJTI#_", s)
    s = re.sub(r"__hip_cuid_\w+", "__hip_cuid_#", s)
    s = re.sub(r"  +;", " ;", s)
    if s.startswith("\t.section\t.text._Z"):
        s = "\t.section\t.text.<next function>"
    return s.rstrip("\n")


def split(path):
    """-> (code: kernel -> lines, metadata: kernel -> lines of its amdhsa.kernels entry, rest: module-level lines)"""
    lines = [norm_line(l) for l in open(path)]
    code, meta, rest = collections.OrderedDict(), collections.OrderedDict(), []
    md = next((k for k, l in enumerate(lines) if l.strip() == ".amdgpu_metadata"), len(lines))
    cur = None
    for l in lines[:md]:
        m = BEGIN.search(l)
        if m:
            cur = m.group(1)
            code[cur] = []
        (rest if cur is None else code[cur]).append(l)
    entry, name = [], None

    def close():
        if entry:
            if name:
                meta[name] = list(entry)
            else:
                rest.extend(entry)
    for l in lines[md:]:
        if l.startswith("  - ."):
            close()
            entry, name = [], None
        entry.append(l)
        m = re.match(r"    \.name:\s+(\S+)", l)
        if m:
            name = m.group(1)
    close()
    return code, meta, rest


def mnemonic(l):
    t = l.strip().split()
    return "(blank)" if not t else t[1] if t[0] == "-" and len(t) > 1 else t[0]      # ("- .offset: 8" counts as .offset:)


def remarks(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"remark: (.*?) \[-Rpass-analysis", l)
        if m:
            t = m.group(1).strip()
            m2 = re.match(r"Function Name: (\S+)", t)
            if m2:
                cur = norm_name(m2.group(1))
                out[cur] = []
            else:
                out[cur].append(t)
    return out


def main():
    ca, ma, ra = split(sys.argv[1])
    cb, mb, rb = split(sys.argv[2])
    print(f"kernels: parent {len(ca)}, new {len(cb)}")
    for k in ca:
        if k not in cb:
            print("  only in parent:", k)
    for k in cb:
        if k not in ca:
            print("  only in new:", k)
    hist, differing = collections.Counter(), set()
    for part, da, db in (("code", ca, cb), ("metadata", ma, mb)):
        for k in da:
            if k in db and da[k] != db[k]:
                differing.add(k)
                if len(da[k]) == len(db[k]):      # same lines, other operands: count line by line
                    for x, y in zip(da[k], db[k]):
                        if x != y:
                            hist[(part, mnemonic(x) if mnemonic(x) == mnemonic(y) else mnemonic(x) + " -> " + mnemonic(y))] += 1
                    continue
                for l in difflib.unified_diff(da[k], db[k], lineterm="", n=0):
                    if not l.startswith(("---", "+++", "@@")):
                        hist[(part, "(lines added / removed) " + mnemonic(l[1:]))] += 1
    if ra != rb:
        for l in difflib.unified_diff(ra, rb, lineterm="", n=0):
            if not l.startswith(("---", "+++", "@@")):
                print("  module level:", l[:160])
    print(f"kernels whose code or metadata entry differs: {len(differing)}")
    for (part, mn), c in sorted(hist.items()):
        print(f"  {part:8s} {mn:28s} {c} changed lines")
    if len(sys.argv) > 4:
        a, b = remarks(sys.argv[3]), remarks(sys.argv[4])
        diff = [k for k in a if k in b and a[k] != b[k]]
        print(f"resource remarks: parent {len(a)} kernels, new {len(b)}, in both {len([k for k in a if k in b])}, differing {len(diff)}")
        for k in diff:
            print("  DIFFERENT:", k)


main()
