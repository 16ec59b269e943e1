#!/usr/bin/env python3
"""Forward + backward of the LPIPS comparison head at the five VGG levels of bs 16, 256 x 256, in both layouts: the fused route
(one lpips_head_f32 + one lpips_head_backward_f32 call per level) against the op-by-op route (GQHIP_TRAIN_FUSED=0: the reference's
arithmetic, the yardstick), through ``LPIPS._head`` in the same process, three alternating rounds, with the peak memory of each
route; then the two fused calls on their own, with bytes moved (forward: two feature maps read; backward: two read, one written)
over time as a fraction of the achievable 6.3 TB/s.

Without ``--step`` this is a driver: every (level, layout) step is a child process of its own under its own time limit
(``--limit`` seconds), one after the other; the first step that fails, or runs out of time, ends the run.  One JSON line per
step goes to stdout and, with ``--out DIR``, to DIR/lpips_head_bench.jsonl.

    python tools/loss/bench_lpips_head.py --out profiles/rNN"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEVELS = [(16, 64, 256, 256), (16, 128, 128, 128), (16, 256, 64, 64), (16, 512, 32, 32), (16, 512, 16, 16)]
HBM = 6.3e12


def step(level: int, layout: str, rounds: int, iters: int):
    sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))
    import torch

    from pit_hip import _lib
    from pit_hip.modules.lpips.loss.lpips import LPIPS, _library_view

    dev = torch.device("cuda:0")
    shape = LEVELS[level]
    torch.manual_seed(level)
    lp = LPIPS(pretrained=False).eval()
    lin = getattr(lp, f"lin{level}").to(dev)
    fmt = torch.channels_last if layout == "blc" else torch.contiguous_format
    f0 = torch.randn(shape, device=dev).relu_().contiguous(memory_format=fmt)
    f1 = (f0 + 0.05 * torch.randn(shape, device=dev)).relu_().contiguous(memory_format=fmt).requires_grad_()
    nbytes = f0.numel() * 4

    def timed(fn, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in ev]     # us

    def fwd_bwd():
        f1.grad = None
        lp._head(f0, f1, lin).sum().backward()

    res = {"level": level, "shape": list(shape), "layout": layout, "tensor_MB": round(nbytes / 1e6, 1), "rounds": []}
    for r in range(rounds):
        row = {}
        for route, env in (("fused", "1"), ("op_by_op", "0")):
            os.environ["GQHIP_TRAIN_FUSED"] = env
            fwd_bwd()
            fwd_bwd()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t = timed(fwd_bwd, iters)
            row[route] = {"us_median": round(statistics.median(t), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                          "peak_extra_MB": round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)}
        row["speedup"] = round(row["op_by_op"]["us_median"] / row["fused"]["us_median"], 2)
        res["rounds"].append(row)
    os.environ["GQHIP_TRAIN_FUSED"] = "1"
    # the two library calls on their own
    (v0, lay), (v1, _) = _library_view(f0), _library_view(f1.detach())
    w = lin.model[-1].weight.reshape(-1)
    g = torch.ones(shape[0], device=dev)
    ws = _lib.LpipsHeadWorkspace()
    for name, fn, moved in (("forward", lambda: _lib.lpips_head(v0, v1, w, lay, ws=ws), 2 * nbytes),
                            ("backward", lambda: _lib.lpips_head_backward(v0, v1, w, g, lay), 3 * nbytes)):
        timed(fn, 3)
        t = statistics.median(timed(fn, iters))
        res[name] = {"us_median": round(t, 1), "bytes": moved, "TB_per_s": round(moved / t / 1e6, 3),
                     "of_6.3_TB_per_s": round(moved / (t * 1e-6) / HBM, 3)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", help="LEVEL:LAYOUT, e.g. 0:bchw (a child of the driver)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--out", help="directory for lpips_head_bench.jsonl")
    a = ap.parse_args()
    if a.step:
        level, layout = a.step.split(":")
        return step(int(level), layout, a.rounds, a.iters)
    lines = []
    for level in range(len(LEVELS)):
        for layout in ("bchw", "blc"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{level}:{layout}", "--rounds", str(a.rounds), "--iters", str(a.iters)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"step {level}:{layout} ran past {a.limit} s: stopping")
            if out.returncode != 0:
                sys.exit(f"step {level}:{layout} ended with status {out.returncode}: stopping\n{out.stderr[-2000:]}")
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "lpips_head_bench.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
