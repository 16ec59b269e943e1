#!/usr/bin/env python3
"""Device timing of the quantiser at codebook dims outside {4, 8, 16, 32}: the exhaustive kernel against the padded filter route
(gqhip.h: gqhip_set_odd_dims), at 16 384 rows x 65 536 codes.

  gq   GaussianQuantRegularizer("bchw", 65536, group=d) eval forward on z [16, 2 d, 32, 32] (K = 1: 16 384 rows), trained-like z
       (mu ~ N(0, 1), sd 0.05 .. 0.3), fixed noise generator
  vq   VQQuantizer("bchw", 65536, d) eval forward on z [16, d, 32, 32]

Device events around `iters` back-to-back forwards after a warm-up; `iters` is sized per variant from one timed call so that a
round lasts about `--round-ms`.  Every round runs the variants one after the other (exhaustive, padded, and the call at the next
filter dim as a yardstick), `--rounds` rounds in one process.  A library without gqhip_set_odd_dims (a build from before the
route) is timed on its only route.  The outputs of the two routes on the timed input are compared bit for bit.  With `--scan`
the rows the re-rank finished by its in-block scan (gqhip_debug_counters) are read on trained-like and on flat z
(sd = |randn| + 0.5).  Prints one JSON line per (kind, dim).

  python tools/odd_dims_bench.py [--dims 5,6,7,9,12,15,17,24,31] [--vq-dims 12] [--rounds 3] [--round-ms 300] [--scan] [--out FILE]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))

N_CODES = 65536


def _events_ms(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _next_filter_dim(d):
    return 8 if d <= 8 else (16 if d <= 16 else 32)


def _gq_z(d, kind, dev, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(16, d, 32, 32, generator=g)
    if kind == "flat":
        sd = torch.randn(16, d, 32, 32, generator=g).abs() + 0.5
    else:
        sd = torch.rand(16, d, 32, 32, generator=g) * 0.25 + 0.05
    return torch.cat([mu, 2.0 * torch.log(sd)], dim=1).to(dev)


def _module(kind, d, dev):
    import torch

    from pit_hip.quantization.gaussian import GaussianQuantRegularizer
    from pit_hip.quantization.vq import VQQuantizer

    if kind == "gq":
        return GaussianQuantRegularizer("bchw", N_CODES, group=d).eval().to(dev)
    torch.manual_seed(d)
    q = VQQuantizer("bchw", N_CODES, d)
    q.embedding.weight.data.normal_()
    return q.eval().to(dev)


def _forward(m, z):
    import torch

    torch.manual_seed(7)                       # the same noise draw on every route
    with torch.no_grad():
        out, info = m(z)[:2]
    return out, info["indices"]


def run(kind, d, a, dev):
    import torch

    from pit_hip import _lib

    routes = ["exhaustive", "padded"] if hasattr(_lib, "set_odd_dims") else ["exhaustive"]
    dp = _next_filter_dim(d)
    z = {"gq": lambda dd: _gq_z(dd, "trained", dev, 100 + dd), "vq": lambda dd: torch.randn(16, dd, 32, 32, generator=torch.Generator().manual_seed(dd)).to(dev)}[kind]
    m, zd = _module(kind, d, dev), z(d)
    mp, zp = _module(kind, dp, dev), z(dp)
    calls = {r: (m, zd, r) for r in routes}
    calls[f"dim{dp}"] = (mp, zp, None)

    def set_route(r):
        if r is not None and len(routes) > 1:
            _lib.set_odd_dims(r)

    res = {"kind": kind, "dim": d, "rows": 16 * 32 * 32, "n": N_CODES, "rounds": a.rounds, "variants": {}}
    try:
        outs, iters = {}, {}
        for name, (mod, zz, r) in calls.items():
            set_route(r)
            outs[name] = _forward(mod, zz)                     # warm-up (sizes the workspace), and the outputs to compare
            one = _events_ms(lambda: _forward(mod, zz), 1)
            iters[name] = max(3, min(200, int(a.round_ms / max(one, 1e-3))))
        if len(routes) > 1:
            res["bit_equal"] = bool(torch.equal(outs["exhaustive"][0], outs["padded"][0]) and torch.equal(outs["exhaustive"][1], outs["padded"][1]))
        times = {k: [] for k in calls}
        for _ in range(a.rounds):
            for name, (mod, zz, r) in calls.items():
                set_route(r)
                times[name].append(_events_ms(lambda: _forward(mod, zz), iters[name]))
        for k, v in times.items():
            res["variants"][k] = {"iters": iters[k], "ms": [round(t, 4) for t in v]}
        if len(routes) > 1:
            ex, pd = times["exhaustive"], times["padded"]
            res["padded_faster_every_round_by_more_than_spread"] = bool(all(e - p > max(ex) - min(ex) for e, p in zip(ex, pd)))
        if a.scan and kind == "gq" and len(routes) > 1:
            _lib.set_odd_dims("padded")
            _lib.debug_enable(True)
            res["rows_finished_by_scan"] = {}
            for zk in ("trained", "flat"):
                _forward(m, _gq_z(d, zk, dev, 200 + d))
                torch.cuda.synchronize()
                res["rows_finished_by_scan"][zk] = _lib.debug_counters(m._ws)[0]
            _lib.debug_enable(False)
    finally:
        set_route("exhaustive")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="5,6,7,9,12,15,17,24,31")
    ap.add_argument("--vq-dims", default="12")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--round-ms", type=float, default=300.0)
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON lines are appended to (default: print only)")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "odd_dims_bench needs a HIP device"
    dev = torch.device("cuda:0")
    todo = [("gq", int(d)) for d in a.dims.split(",") if d] + [("vq", int(d)) for d in a.vq_dims.split(",") if d]
    for kind, d in todo:
        line = json.dumps(run(kind, d, a, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
