#!/usr/bin/env python3
"""Device timing of the quantiser at codebook dims 1, 2 and 3: the exhaustive kernel against the pruned exact search
(gqhip.h: gqhip_set_low_dims), at 65 536 codes.

  g = 1  GaussianQuantRegularizer("bchw", 65536, group=1) eval forward on z [16, 32, 32, 32]  (262 144 rows)
  g = 2  ... group=2 on z [16, 32, 32, 32]                                                    (131 072 rows)
  g = 3  ... group=3 on z [16, 24, 32, 32]                                                    ( 65 536 rows)
  dim4   ... group=4 on z [16,  8, 32, 32]  (16 384 rows), the yardstick: the dim-4 grid search

z is trained-like (mu ~ N(0, 1), sd 0.05 .. 0.3) with a fixed noise generator.  Device events around `iters` back-to-back
forwards after a warm-up; `iters` is sized per variant from one timed call so that a round lasts about `--round-ms`.  Every
round runs the variants one after the other (exhaustive, search, dim4), `--rounds` rounds in one process.  A library without
gqhip_set_low_dims (a build from before the route) is timed on its only route.  The outputs of the two routes on the timed
input are compared bit for bit.  With `--finish` the rows the finish launch took (gqhip_debug_counters) are read on
trained-like and on flat z (sd = |randn| + 0.5).  `--once GROUP` runs a few search forwards only, for a kernel trace.
Prints one JSON line per group.

  python tools/low_dims_bench.py [--groups 1,2,3] [--rounds 3] [--round-ms 300] [--finish] [--out FILE] [--once G]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))

N_CODES = 65536
CHANNELS = {1: 32, 2: 32, 3: 24, 4: 8}          # z channels (mean and log-variance halves together) per group


def _events_ms(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _gq_z(g, kind, dev, seed):
    import torch

    gen = torch.Generator().manual_seed(seed)
    c = CHANNELS[g] // 2
    mu = torch.randn(16, c, 32, 32, generator=gen)
    if kind == "flat":
        sd = torch.randn(16, c, 32, 32, generator=gen).abs() + 0.5
    else:
        sd = torch.rand(16, c, 32, 32, generator=gen) * 0.25 + 0.05
    return torch.cat([mu, 2.0 * torch.log(sd)], dim=1).to(dev)


def _module(g, dev):
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    return GaussianQuantRegularizer("bchw", N_CODES, group=g).eval().to(dev)


def _forward(m, z):
    import torch

    torch.manual_seed(7)                       # the same noise draw on every route
    with torch.no_grad():
        out, info = m(z)[:2]
    return out, info["indices"]


def run(g, a, dev):
    import torch

    from pit_hip import _lib

    routes = ["exhaustive", "search"] if hasattr(_lib, "set_low_dims") else ["exhaustive"]
    m, zd = _module(g, dev), _gq_z(g, "trained", dev, 100 + g)
    m4, z4 = _module(4, dev), _gq_z(4, "trained", dev, 104)
    calls = {r: (m, zd, r) for r in routes}
    calls["dim4"] = (m4, z4, None)

    def set_route(r):
        if r is not None and len(routes) > 1:
            _lib.set_low_dims(r)

    res = {"group": g, "rows": 16 * 32 * 32 * (CHANNELS[g] // 2) // g, "n": N_CODES, "rounds": a.rounds, "variants": {}}
    try:
        outs, iters = {}, {}
        for name, (mod, zz, r) in calls.items():
            set_route(r)
            outs[name] = _forward(mod, zz)                     # warm-up (sizes the workspace), and the outputs to compare
            one = _events_ms(lambda: _forward(mod, zz), 1)
            iters[name] = max(3, min(200, int(a.round_ms / max(one, 1e-3))))
        if len(routes) > 1:
            res["bit_equal"] = bool(torch.equal(outs["exhaustive"][0], outs["search"][0]) and torch.equal(outs["exhaustive"][1], outs["search"][1]))
        times = {k: [] for k in calls}
        for _ in range(a.rounds):
            for name, (mod, zz, r) in calls.items():
                set_route(r)
                times[name].append(_events_ms(lambda: _forward(mod, zz), iters[name]))
        for k, v in times.items():
            res["variants"][k] = {"iters": iters[k], "ms": [round(t, 4) for t in v]}
        if len(routes) > 1:
            ex, se = times["exhaustive"], times["search"]
            res["search_faster_every_round_by_more_than_spread"] = bool(all(e - s > max(ex) - min(ex) for e, s in zip(ex, se)))
            res["ratio"] = round(min(ex) / max(se), 2)
        if a.finish and len(routes) > 1:
            _lib.set_low_dims("search")
            _lib.debug_enable(True)
            res["finish_rows"] = {}
            for zk in ("trained", "flat"):
                _forward(m, _gq_z(g, zk, dev, 200 + g))
                torch.cuda.synchronize()
                res["finish_rows"][zk] = _lib.debug_counters(m._ws)[0]
            _lib.debug_enable(False)
    finally:
        set_route("exhaustive")
    return res


def once(g, dev):
    import torch

    from pit_hip import _lib

    _lib.set_low_dims("search")
    m, z = _module(g, dev), _gq_z(g, "trained", dev, 100 + g)
    for _ in range(5):
        _forward(m, z)
    torch.cuda.synchronize()
    _lib.set_low_dims("exhaustive")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,2,3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--round-ms", type=float, default=300.0)
    ap.add_argument("--finish", action="store_true")
    ap.add_argument("--once", type=int, default=0, help="run five search forwards at this group and exit (for a kernel trace)")
    ap.add_argument("--out", default=None, help="file the JSON lines are appended to (default: print only)")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "low_dims_bench needs a HIP device"
    dev = torch.device("cuda:0")
    if a.once:
        once(a.once, dev)
        return 0
    for g in [int(x) for x in a.groups.split(",") if x]:
        line = json.dumps(run(g, a, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
