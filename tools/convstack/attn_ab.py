"""attn_ab.txt from the two kernel-stats files: the launches this change touches, parent and branch."""
import csv, re, sys
def load(path):
    out = {}
    for r in csv.DictReader(open(path)):
        out[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return out
def short(n):
    m = re.search(r"(conv1x1_f16x3_kernel<[^>]*>|gn_apply_nhwc_kernel<0>|attn_split_qkv_kernel|attn_softmax_split_kernel)", n)
    return m.group(1) if m else None
P, B = load(sys.argv[1]), load(sys.argv[2])
steps = None
rows = {}
for tag, d in (("parent", P), ("branch", B)):
    for n, (c, t) in d.items():
        s = short(n)
        if s: rows.setdefault(s, {})[tag] = (c, t)
        if tag == "parent" and s == "attn_split_qkv_kernel": steps = c / 5.0
print("rocprofv3 --kernel-trace --stats of bench.py --full --steps 6 --warmup 3 --no-cpu-baseline --no-reference-gpu, parent tree and")
print("this tree, each in a run of its own on one MI355X.  The launches this change touches; %g forward passes per run" % steps)
print("(5 attention blocks each).  us = mean per call; ms/step = total over the run / passes.")
print("%-44s %6s %9s %9s   %6s %9s %9s" % ("kernel", "calls", "us", "ms/step", "calls", "us", "ms/step"))
tp = tb = 0.0
for s in sorted(rows):
    if s == "attn_softmax_split_kernel": continue
    p, b = rows[s].get("parent"), rows[s].get("branch")
    f = lambda v: ("%6d %9.1f %9.4f" % (v[0], v[1] / v[0] / 1e3, v[1] / 1e6 / steps)) if v else "%6s %9s %9s" % ("-", "-", "-")
    print("%-44s %s   %s" % (s, f(p), f(b)))
    tp += p[1] if p else 0.0; tb += b[1] if b else 0.0
print("sum of the touched launches: parent %.4f ms/step, branch %.4f ms/step, saved %.4f ms/step = %.1f us per attention block"
      % (tp / 1e6 / steps, tb / 1e6 / steps, (tp - tb) / 1e6 / steps, (tp - tb) / 1e3 / steps / 5))
