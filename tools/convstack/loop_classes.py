"""Instruction-class sequence of a kernel's hottest loop, read from `make asm` output (no GPU needed).

    python tools/convstack/loop_classes.py vq-vae-from-gaussian-vae_amd/csrc/gqhip_unet.gfx950.s conv3x3_gn_f16x3_kernelILi1ELi128E

Finds the kernel whose mangled name contains the pattern, takes the backward branch that spans the most MFMAs as the main
loop and prints its body run-length encoded: M = v_mfma, V = other vector ALU, T = transcendental (v_exp / v_rcp / ...),
Lr / Lw = LDS read / write, G = global load, W = s_waitcnt, B = branch, | = s_barrier, s = other scalar.  Labels inside
the body are shown as [label]: a trip without them is one basic block.
"""
import re
import sys


def classify(op):
    if op.startswith("v_mfma"):
        return "M"
    if re.match(r"v_(exp|rcp|rsq|sqrt|log|sin|cos)_", op):
        return "T"
    if op.startswith("v_"):
        return "V"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "Lr"
    if op.startswith("ds_"):
        return "Lw"
    if op.startswith("global_load") or op.startswith("buffer_load"):
        return "G"
    if op == "s_waitcnt":
        return "W"
    if op == "s_barrier":
        return "|"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "B"
    return "s"


def main():
    path, pat = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and pat in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    body = []       # (kind, text): kind "label" or an instruction class
    labels = {}
    for l in lines[start + 1:end]:
        s = l.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\w+):", s)
            if m:
                labels[m.group(1)] = len(body)
                body.append(("label", m.group(1)))
            continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(body)
            body.append(("label", m.group(1)))
            continue
        op = s.split()[0]
        body.append((classify(op), s))
    best = None
    for i, (k, s) in enumerate(body):
        if k == "B":
            tgt = s.split()[-1]
            if tgt in labels and labels[tgt] < i:
                n = sum(1 for kk, _ in body[labels[tgt]:i] if kk == "M")
                if best is None or n > best[0]:
                    best = (n, labels[tgt], i)
    n, lo, hi = best
    trip = body[lo:hi + 1]
    counts = {}
    for k, _ in trip:
        counts[k] = counts.get(k, 0) + 1
    print(f"kernel {lines[start].rstrip(':')}")
    print(f"main loop: {len(trip)} entries, " + ", ".join(f"{k} {v}" for k, v in sorted(counts.items())))
    inner = [s for k, s in trip[1:-1] if k in ("label", "B")]
    print(f"labels / branches inside the trip (besides its head and its back edge): {len(inner)}" + (": " + " ".join(x.split()[0] + "->" + x.split()[-1] if not x.startswith(".") else "[" + x + "]" for x in inner) if inner else ""))
    # run-length encoding, one line per MFMA-to-MFMA stretch
    out, run = [], []
    for k, s in trip:
        tok = "[" + s + "]" if k == "label" else k
        if run and run[-1][0] == tok:
            run[-1][1] += 1
        else:
            run.append([tok, 1])
    text = " ".join(t if c == 1 else f"{t}x{c}" for t, c in run)
    # wrap
    line = ""
    for w in text.split(" "):
        if len(line) + len(w) > 150:
            out.append(line)
            line = ""
        line += ("" if not line else " ") + w
    out.append(line)
    print("\n".join(out))
    # VALU between consecutive MFMAs
    gaps, g, seen = [], 0, False
    for k, _ in trip:
        if k == "M":
            if seen:
                gaps.append(g)
            seen, g = True, 0
        elif k in ("V", "T"):
            g += 1
    hist = {}
    for x in gaps:
        hist[x] = hist.get(x, 0) + 1
    print("VALU+transcendental instructions between consecutive MFMAs (count: how many gaps): " + ", ".join(f"{k}: {v}" for k, v in sorted(hist.items())))


if __name__ == "__main__":
    main()
