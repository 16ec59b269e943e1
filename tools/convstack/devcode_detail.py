#!/usr/bin/env python3
"""Where two builds' device code differs, kernel by kernel (the follow-up of tools/devcode_compare.py when its answer is DIFFERENT).

    python tools/convstack/devcode_detail.py PARENT.co TREE.co

Per kernel whose disassembly or metadata differs: the metadata fields that matter for occupancy (registers, LDS, scratch, spills)
on both sides, the instruction counts, the opcode histogram's differences, and where the first and the last differing
instruction lie relative to the kernel's main loop (a loop = the span of a backward branch; the main loop = the longest
span that contains no other).  Needs no GPU.  Exit status 1 when a kernel's tree build has more VGPRs, AGPRs, LDS, scratch or spills than its parent's."""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import devcode_compare as D  # noqa: E402

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
          "sgpr_spill_count")
WORSE = ("vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def fields(record):
    return {f: int(m.group(1)) for f in FIELDS for m in [re.search(rf"\.{f}:\s+(\d+)", record)] if m}


def loops(path):
    """{symbol: [(first, last) instruction index of every backward branch's span]}"""
    out, cur, offs = {}, None, []
    for line in subprocess.run([D.LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur, base, offs = out.setdefault(m.group(2), []), int(m.group(1), 16), []
            continue
        m = re.match(r"^\s+(\S+).*//\s*([0-9A-Fa-f]+):.*?(?:<.+\+0x([0-9a-f]+)>)?$", line)
        if cur is None or not m:
            continue
        offs.append(int(m.group(2), 16) - base)
        if m.group(1).startswith(("s_cbranch", "s_branch")) and m.group(3) and int(m.group(3), 16) <= offs[-1]:
            cur.append((offs.index(int(m.group(3), 16)), len(offs) - 1))
    return out


def main_loop(spans):
    inner = [s for s in spans or [] if not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans)]
    return max(inner, key=lambda s: s[1] - s[0]) if inner else None


def where(i, spans):
    if not spans:
        return "no loop"
    lo, hi = main_loop(spans)
    return f"{'before' if i < lo else 'after' if i > hi else 'INSIDE'} main loop [{lo}, {hi}]"


def main(a, b):
    da, db, ma, mb, la, lb = D.disassembly(a), D.disassembly(b), D.metadata(a), D.metadata(b), loops(a), loops(b)
    worse = []
    names = sorted(s for s in set(da) | set(db) if da.get(s) != db.get(s) or ma.get(s + ".kd") != mb.get(s + ".kd"))
    print(f"{a} (parent) vs {b} (tree): {len(names)} of {len(da)} kernels differ")
    for s in names:
        A, B = da.get(s, []), db.get(s, [])
        fa, fb = fields(ma.get(s + ".kd", "")), fields(mb.get(s + ".kd", ""))
        print(f"\n{s}")
        print(f"  metadata record {'equal' if ma.get(s + '.kd') == mb.get(s + '.kd') else 'DIFFERS'}: "
              + ", ".join(f"{f} {fa.get(f)}" + ("" if fa.get(f) == fb.get(f) else f" -> {fb.get(f)}") for f in FIELDS))
        worse += [(s, f) for f in WORSE if fb.get(f, 0) > fa.get(f, 0)]
        ha, hb = collections.Counter(t.split()[0] for t in A), collections.Counter(t.split()[0] for t in B)
        delta = {k: hb[k] - ha[k] for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]}
        print(f"  instructions {len(A)} -> {len(B)}; opcode histogram " + ("equal" if not delta else "differs: "
              + ", ".join(f"{k} {ha[k]} -> {hb[k]}" for k in delta)))
        if A == B:
            print("  disassembly equal")
            continue
        first = next((i for i, (x, y) in enumerate(zip(A, B)) if x != y), min(len(A), len(B)))
        back = next((i for i, (x, y) in enumerate(zip(reversed(A), reversed(B))) if x != y), min(len(A), len(B)))
        print(f"  first differing instruction: index {first}, parent {where(first, la.get(s))}, tree {where(first, lb.get(s))}")
        print(f"  last differing instruction: parent index {len(A) - 1 - back} {where(len(A) - 1 - back, la.get(s))},"
              f" tree index {len(B) - 1 - back} {where(len(B) - 1 - back, lb.get(s))}")
        lo_a, lo_b = main_loop(la.get(s)), main_loop(lb.get(s))
        if lo_a and lo_b:
            same = A[lo_a[0]:lo_a[1] + 1] == B[lo_b[0]:lo_b[1] + 1]
            print(f"  main loop body: parent {lo_a[1] - lo_a[0] + 1} instructions, tree {lo_b[1] - lo_b[0] + 1}: "
                  + ("the same instruction text" if same else "DIFFERS -> timing list"))
    print(f"\nkernels with more VGPRs / AGPRs / LDS / scratch / spills than the parent: {worse if worse else 'none'}")
    return 1 if worse else 0


if __name__ == "__main__":
    assert len(sys.argv) == 3, __doc__
    sys.exit(main(sys.argv[1], sys.argv[2]))
