#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 assembly listings of one source file (a refactor's check that the compiler
made the same kernels): registers, scratch and LDS from the metadata, instruction counts by class, total instructions,
and the s_waitcnt lines whose count differs -- by operand and by where they stand (pro: before the kernel's first
MFMA, k: between its first and last, epi: behind the last).  A markdown table; profiles/r09_isa_compare.md is one.
The listings: the Makefile's hipcc line for the file with `--offload-device-only -S -o file.s` in place of `-c -o`.
    python scripts/isa_compare.py parent.s new.s"""
import collections
import re
import shutil
import subprocess
import sys


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout
    return dict(zip(names, out.splitlines()))


def parse(path):
    kern = {}
    meta = {}
    cur = None
    txt = open(path).read()
    for line in txt.splitlines():
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1)
            kern[cur] = []
            continue
        if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
            cur = None if line.startswith(".Lfunc_end") else cur
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        kern[cur].append(s)
    # metadata
    for blk in re.split(r"\n  - \.agpr_count", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return kern, meta


CLASSES = [("mfma", r"^v_mfma"), ("ds_read", r"^ds_read"), ("ld_lds", r"^global_load_lds"),
           ("g_store", r"^global_store"), ("g_load", r"^global_load_dword"), ("barrier", r"^s_barrier")]


def counts(ins):
    c = {}
    for n, rx in CLASSES:
        c[n] = sum(1 for i in ins if re.match(rx, i))
    return c


def main():
    bk, bm = parse(sys.argv[1])
    nk, nm = parse(sys.argv[2])
    names = sorted(set(bm) | set(nm))
    dm = demangle(names)
    bad = 0
    print("| kernel | VGPR | SGPR | scratch | LDS | mfma | ds_read | load_lds | g_store | g_load | barrier | instr base | instr new | waitcnt diff |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for n in names:
        if n not in bm or n not in nm:
            print("| %s | ONLY IN %s |" % (dm[n], "base" if n in bm else "new"))
            bad += 1
            continue
        b, m = bm[n], nm[n]
        bc, nc = counts(bk[n]), counts(nk[n])

        def f(x, y):
            return str(x) if x == y else "**%s -> %s**" % (x, y)
        for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            if b[k] != m[k]:
                bad += 1
        for k, _ in CLASSES:
            if bc[k] != nc[k]:
                bad += 1
        def regions(ins):
            mf = [x for x, i in enumerate(ins) if i.startswith("v_mfma")]
            out = collections.Counter()
            for x, i in enumerate(ins):
                if i.startswith("s_waitcnt"):
                    reg = "all" if not mf else "pro" if x < mf[0] else ("epi" if x > mf[-1] else "k")
                    out[(reg, i.replace("s_waitcnt ", ""))] += 1
            return out
        bw, nw = regions(bk[n]), regions(nk[n])
        d = []
        for k in sorted(set(bw) | set(nw)):
            if bw[k] != nw[k]:
                d.append("%s %s: %d -> %d" % (k[0], k[1], bw[k], nw[k]))
        short = re.sub(r"^void merlin::\(anonymous namespace\)::", "", dm[n])
        short = re.sub(r"\(.*$", "", short)
        print("| `%s` | %s | %s | %s | %s | %s | %d | %d | %s |" % (
            short, f(b["vgpr_count"], m["vgpr_count"]), f(b["sgpr_count"], m["sgpr_count"]),
            f(b["private_segment_fixed_size"], m["private_segment_fixed_size"]),
            f(b["group_segment_fixed_size"], m["group_segment_fixed_size"]),
            " | ".join(f(bc[k], nc[k]) for k, _ in CLASSES), len(bk[n]), len(nk[n]),
            "; ".join(d) if d else ("same bytes" if bk[n] == nk[n] else "none")))
    print()
    print("kernels: %d, cells of registers / scratch / LDS / class counts that differ: %d" % (len(names), bad))


main()
