#!/usr/bin/env python3
"""Device timing of the fp64 moments kernel (csrc/gq_moments.h) against torch's own route on the same device, and the wall time of
evaluate_sharded without FID, with it, and with the reference's per-step treatment of the features.

  moments: at rows 16, D 2048 (the workload: a batch of pooled Inception features) and rows 16, D 768, device events around
    `--iters` calls, `--rounds` rounds with the variants alternating inside every round:
      kernel   _lib.moments_update(x, state)                       one launch, upper triangle only
      torch    state.addmm_(x64.T, x64), x64 = x.double()          torch's fp64 GEMM into a full D x D matrix (its own summation order)
    Per variant: median / min / max of the rounds' per-call microseconds, and `hbm_fraction` = the bytes the upper-triangle update
    must move (2 x 8 x D (D + 1) / 2 for the state, read and written once, plus the rows) over the median time, over 8 TB/s.  A
    33.6 MB state fits the 256 MB Infinity Cache, so the figure can exceed what HBM alone would give: it is a yardstick, not a
    counter.  The kernel's state after the timed calls is checked against the CPU rule's on a fresh pair of calls.
  eval: the loop of evaluate_sharded (sharded_eval_steps, bit-packed record) at world size 1 over `--eval-steps` batches of 16 images with an identity encoder / decoder around a
    VQQuantizer(n = 65536, dim = 4) (the stub of tools/wire_bits_bench.py) and a stub extractor (a fixed projection of the pooled
    image to D = 2048, relu), host clock around the call and a device synchronise:
      plain      no fid_features
      fid        fid_features: two kernel launches per step, nothing leaves the device inside the loop
      reference  the reference's per-step treatment (eval.py:186-203) added to the plain loop by the extractor wrapper: per feature
                 block one all_gather-shaped copy (world 1: a clone) and one .cpu() copy, the rows kept on the host, np.mean /
                 np.cov at the end
    The loop is timed in rounds; what follows it (moments() or np.mean / np.cov, then the Frechet distance: two 2048 x 2048
    eigendecompositions on the CPU either way) is timed once per mode and reported apart.
    More than one rank over RCCL is NOT measured here.

The default run starts each section as a child process under its own time limit and starts nothing after one that failed.
Prints one JSON line per section.

  python tools/fid_bench.py [--iters 200] [--rounds 9] [--eval-steps 50] [--only moments|eval] [--out DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))

HBM_PEAK = 8.0e12          # bytes / s, the specification's figure
SECTION_LIMIT_S = {"moments": 240, "eval": 300}


def _events_us(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _rounds(variants, iters, rounds, warmup=20):
    import torch

    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(_events_us(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3)}
            for k, v in times.items()}


def moments(a, dev):
    import torch

    from pit_hip import _lib
    from pit_hip.evaluations.fid.fid_score import FrechetStats

    out = {"section": "moments", "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    for rows, D in ((16, 2048), (16, 768)):
        g = torch.Generator().manual_seed(D)
        x = torch.relu(torch.randn(rows, D, generator=g) + 0.3).to(dev)
        x64 = x.double()
        state = torch.zeros(_lib.moments_state_words(D), dtype=torch.float64, device=dev)
        full = torch.zeros(D, D, dtype=torch.float64, device=dev)
        res = _rounds({"kernel": lambda: _lib.moments_update(x, state), "torch": lambda: full.addmm_(x64.T, x64)}, a.iters, a.rounds)
        traffic = 2 * 8 * D * (D + 1) // 2 + 4 * rows * D
        for v in res.values():
            v["hbm_fraction"] = round(traffic / (v["median_us"] * 1e-6) / HBM_PEAK, 3)
        fresh = FrechetStats(D, dev).update(x).update(x).state.cpu()
        want = FrechetStats(D, "cpu").update(x.cpu()).update(x.cpu()).state
        iu = torch.triu_indices(D, D)
        same = bool(torch.equal(fresh[: D * D].view(D, D)[iu[0], iu[1]], want[: D * D].view(D, D)[iu[0], iu[1]])
                    and torch.equal(fresh[D * D:], want[D * D:]))
        out["shapes"][f"rows{rows}_D{D}"] = {**res, "upper_triangle_traffic_bytes": traffic, "bits_equal_cpu_rule": same}
    print(json.dumps(out), flush=True)
    return 0 if all(s["bits_equal_cpu_rule"] for s in out["shapes"].values()) else 1


class _Model:
    def __init__(self, q):
        self.q = q

    def encode(self, x, return_reg_log=True):
        return self.q(x)

    def decode(self, z):
        return z


class _ReferenceTreatment:
    """eval.py:186-203 at world size 1 around an extractor: the gather-shaped copy and the host copy of every block, rows kept on
    the host; called through the same hook, it returns nothing to accumulate on the device."""

    def __init__(self, features):
        self.features, self.rows = features, []

    def __call__(self, images):
        import torch

        feats = self.features(images)
        gathered = [torch.zeros_like(feats)]
        gathered[0].copy_(feats)
        self.rows.append(gathered[0].detach().cpu())
        return feats


def eval_loop(a, dev):
    import numpy as np
    import torch

    from pit_hip import eval_dist as E
    from pit_hip.evaluations.fid.fid_score import calculate_frechet_distance
    from pit_hip.quantization.vq import VQQuantizer

    n, bs, steps, D = 65536, 16, a.eval_steps, 2048
    torch.manual_seed(2)
    q = VQQuantizer("bchw", n, 4)
    q.embedding.weight.data.normal_()
    model = _Model(q.eval().to(dev))
    images = torch.randn(bs * steps, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    ids = [torch.arange(s * bs, (s + 1) * bs, device=dev) for s in range(steps)]
    proj = (torch.randn(4 * 16, D, generator=torch.Generator().manual_seed(4)) * 0.2).to(dev)

    def features(x):
        return torch.relu(torch.nn.functional.adaptive_avg_pool2d(x, (4, 4)).reshape(x.shape[0], -1) @ proj + 0.3)

    def loop(mode):
        """(ms of the per-step loop ending in a device synchronise, what it accumulated)"""
        it = iter(ids)
        layout = E.StepRecord(bs, 256, n_metrics=1, n_codes=n)
        hist = torch.zeros(n, dtype=torch.int64, device=dev)
        acc = {"plain": None, "fid": E.FidAccumulator(features), "reference": _HostOnly(_ReferenceTreatment(features))}[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gathered = E.sharded_eval_steps(model, lambda _: images[next(it)], E.shard_batches(bs * steps, 1, 0, bs), layout, 1, dev, hist, acc)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert len(gathered) == steps
        return ms, acc

    def finish(mode, acc):
        """(ms from the loop's end to the FID value on the host, the value): once per mode, it is the same work every time"""
        t0 = time.perf_counter()
        if mode == "fid":
            value = acc.result()["fid"]
        else:
            rows = [torch.cat(acc.wrapper.rows[k::2]).numpy() for k in (0, 1)]
            stats = [(np.mean(r, axis=0), np.cov(r, rowvar=False)) for r in rows]
            value = calculate_frechet_distance(*stats[1], *stats[0])
        return (time.perf_counter() - t0) * 1e3, value

    modes = ("plain", "fid", "reference")
    times, last = {m: [] for m in modes}, {}
    for r in range(a.rounds + 1):                 # round 0 warms every path up
        for m in modes:
            ms, last[m] = loop(m)
            if r:
                times[m].append(ms)
    ends = {m: finish(m, last[m]) for m in ("fid", "reference")}
    print(json.dumps({"section": "eval", "steps": steps, "bs": bs, "D": D, "rounds": a.rounds,
                      "loop": {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                                   "per_step_us": round(statistics.median(v) * 1e3 / steps, 1)} for k, v in times.items()},
                      "after_the_loop": {m: {"ms": round(ms, 1), "fid": value} for m, (ms, value) in ends.items()}}), flush=True)
    return 0


class _HostOnly:
    """The `fid` hook of sharded_eval_steps for the reference's treatment: both feature blocks go through the wrapper, nothing is
    accumulated on the device."""

    def __init__(self, wrapper):
        self.wrapper = wrapper

    def update(self, x, x_rec):
        self.wrapper(x)
        self.wrapper(x_rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--eval-steps", type=int, default=50)
    ap.add_argument("--only", choices=("moments", "eval"), default=None, help="run this one section in this process")
    ap.add_argument("--out", default=None, help="directory for fid_bench.jsonl (default: print only)")
    a = ap.parse_args()
    if a.only:
        import torch

        assert torch.cuda.is_available(), "fid_bench needs a HIP device"
        return {"moments": moments, "eval": eval_loop}[a.only](a, torch.device("cuda:0"))
    lines = []
    for section, limit in SECTION_LIMIT_S.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--only", section, "--iters", str(a.iters), "--rounds", str(a.rounds),
               "--eval-steps", str(a.eval_steps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"fid_bench: section {section} exceeded {limit} s; nothing further is started", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            print(f"fid_bench: section {section} ended with status {r.returncode}; nothing further is started", file=sys.stderr)
            return r.returncode
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "fid_bench.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
