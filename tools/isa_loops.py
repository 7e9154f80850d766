#!/usr/bin/env python
"""Instruction mix of the MFMA loops of a kernel, from device assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -I include -S \\
        scflow_amd/csrc/conv.hip -o conv.s
    python tools/isa_loops.py conv.s 'conv_wino5_kernel<0, 32, 2, 1>' [more patterns ...]
    python tools/isa_loops.py conv.s --list          # the kernels of the file, demangled

Every pattern is a regular expression searched in the demangled (c++filt, when present) and the
mangled name of each kernel of the file.  For each match the tool finds the loops — a backward
branch to a label — keeps the innermost ones that hold MFMAs, and prints per loop the instruction
counts by class, the non-MFMA-VALU / MFMA ratio, the number of basic blocks and the VALU opcode
histogram.  A class is decided by the mnemonic's prefix alone:

    MFMA    v_mfma, v_smfmac          LDS     ds_
    VALU    any other v_              VMEM    buffer_, global_, flat_, scratch_
    SMEM    s_load, s_buffer_load     WAIT    s_waitcnt, s_barrier, s_nop, s_sleep
    BRANCH  s_branch, s_cbranch       SALU    any other s_

A loop body with more than one basic block has control flow inside it (exec-mask regions, peeled
cases); `blocks` and `BRANCH` show that.  The counts are static: one trip of the loop as laid out,
every block counted once — a block that a trip rarely enters (a peeled case) counts like any
other.  `--blocks` lists the blocks one by one, so such a block can be told apart and taken off.
"""
from __future__ import annotations

import argparse
import collections
import re
import shutil
import subprocess
import sys

CLASSES = ("MFMA", "VALU", "SALU", "SMEM", "LDS", "VMEM", "WAIT", "BRANCH")
PREFIXES = (  # first match wins
    ("v_mfma", "MFMA"), ("v_smfmac", "MFMA"), ("v_", "VALU"),
    ("s_load", "SMEM"), ("s_buffer_load", "SMEM"),
    ("s_waitcnt", "WAIT"), ("s_barrier", "WAIT"), ("s_nop", "WAIT"), ("s_sleep", "WAIT"),
    ("s_branch", "BRANCH"), ("s_cbranch", "BRANCH"), ("s_", "SALU"),
    ("ds_", "LDS"), ("buffer_", "VMEM"), ("global_", "VMEM"), ("flat_", "VMEM"),
    ("scratch_", "VMEM"),
)
LABEL = re.compile(r"^([.\w$]+):")
INSN = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b(.*)$")
TARGET = re.compile(r"(\.LBB\d+_\d+)")


def classify(mnemonic):
    for p, c in PREFIXES:
        if mnemonic.startswith(p):
            return c
    return None


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(lines):
    """{mangled name: (first line, one past the last line)} of the file's kernels: the symbols
    with an .amdhsa_kernel descriptor, their text from the label to .Lfunc_end."""
    names = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    spans, cur = {}, None
    for i, l in enumerate(lines):
        m = LABEL.match(l)
        if m and m.group(1) in names and cur is None:
            cur = (m.group(1), i + 1)
        elif cur and l.startswith(".Lfunc_end"):
            spans[cur[0]] = (cur[1], i)
            cur = None
    return spans


def loops(lines, lo, hi):
    """[(first, last)] line ranges of the innermost loops with MFMAs in lines[lo:hi]."""
    where = {}
    for i in range(lo, hi):
        m = LABEL.match(lines[i])
        if m:
            where[m.group(1)] = i
    found = []
    for i in range(lo, hi):
        m = INSN.match(lines[i])
        if not m or classify(m.group(1)) != "BRANCH":
            continue
        t = TARGET.search(m.group(2))
        if t and t.group(1) in where and where[t.group(1)] <= i:
            found.append((where[t.group(1)], i))

    def has_mfma(a, b):
        return any((m := INSN.match(lines[k])) and classify(m.group(1)) == "MFMA"
                   for k in range(a, b + 1))
    # Innermost: drop a range that holds another whole.  Then backward branches whose ranges
    # overlap without nesting are latches of one loop whose blocks the layout interleaved (a loop
    # with an if-chain at its head has several): merge them, and keep the merged ranges only.
    found = sorted(set(f for f in found if has_mfma(*f)))
    found = [f for f in found
             if not any(g != f and f[0] <= g[0] and g[1] <= f[1] for g in found)]
    merged = True
    while merged:
        merged = False
        for f in found:
            for g in found:
                if f[0] < g[0] <= f[1] < g[1]:
                    found = sorted(set(found) - {f, g} | {(f[0], g[1])})
                    merged = True
                    break
            if merged:
                break
    return [f for f in found
            if not any(g != f and g[0] <= f[0] and f[1] <= g[1] for g in found)]


def count(lines, a, b):
    """Class counts and opcode histograms of lines[a..b], and the same per basic block:
    [(label, class counts, VALU histogram)]."""
    by_class = collections.Counter()
    hist = {c: collections.Counter() for c in CLASSES}
    blocks = []
    for k in range(a, b + 1):
        lab = LABEL.match(lines[k])
        if lab or not blocks:
            blocks.append((lab.group(1) if lab else "(entry)", collections.Counter(),
                           collections.Counter()))
        m = INSN.match(lines[k])
        c = classify(m.group(1)) if m else None
        if c:
            by_class[c] += 1
            hist[c][m.group(1)] += 1
            blocks[-1][1][c] += 1
            if c == "VALU":
                blocks[-1][2][m.group(1)] += 1
    return by_class, hist, blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("patterns", nargs="*")
    ap.add_argument("--list", action="store_true", help="print the kernels' names and exit")
    ap.add_argument("--blocks", action="store_true", help="the counts of every basic block too")
    ap.add_argument("--all-classes", action="store_true",
                    help="opcode histograms of every class, not of VALU alone")
    a = ap.parse_args()
    with open(a.asm) as f:
        lines = f.read().splitlines()
    spans = kernels(lines)
    pretty = demangle(sorted(spans))
    if a.list:
        for n in sorted(spans, key=lambda n: pretty[n]):
            print(pretty[n])
        return 0
    missing = 0
    for pat in a.patterns:
        rx = re.compile(pat)
        hits = [n for n in sorted(spans) if rx.search(pretty[n]) or rx.search(n)]
        if not hits:
            print(f"no kernel matches {pat!r}", file=sys.stderr)
            missing += 1
        for n in hits:
            lo, hi = spans[n]
            ls = loops(lines, lo, hi)
            print(f"== {pretty[n]}")
            if not ls:
                print("   no loop with MFMAs")
            for idx, (x, y) in enumerate(ls):
                c, hist, blks = count(lines, x, y)
                ratio = c["VALU"] / c["MFMA"]
                print(f"   loop {idx} (lines {x + 1}-{y + 1}, {len(blks)} block{'s' * (len(blks) > 1)}): " +
                      " ".join(f"{k} {c[k]}" for k in CLASSES) + f" | VALU/MFMA {ratio:.2f}")
                for k in (CLASSES if a.all_classes else ("VALU",)):
                    if hist[k] and k != "MFMA":
                        print(f"      {k}: " + ", ".join(f"{op} {v}" for op, v in hist[k].most_common()))
                for lab, bc, bh in (blks if a.blocks else ()):
                    print(f"      block {lab}: " + " ".join(f"{k} {bc[k]}" for k in CLASSES if bc[k]) +
                          (" | " + ", ".join(f"{op} {v}" for op, v in bh.most_common()) if bh else ""))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
