#!/usr/bin/env python3
"""Device timing of the quantiser at codebook dims 33-64: the exhaustive kernel against the dim-64 filter route (gqhip.h:
gqhip_set_wide_dims), at 16 384 rows x 65 536 codes.

  gq   GaussianQuantRegularizer("bchw", 65536, group=d) eval forward on z [16, 2 d, 32, 32] (K = 1: 16 384 rows), trained-like z
       (mu ~ N(0, 1), sd 0.05 .. 0.3), fixed noise generator
  vq   VQQuantizer("bchw", 65536, d) eval forward on z [16, d, 32, 32]

Device events around `iters` back-to-back forwards after a warm-up; `iters` is sized per variant from one timed call so that a
round lasts about `--round-ms`.  Every round runs the variants one after the other (exhaustive, filter, and the dim-32 call as a
yardstick), `--rounds` rounds in one process.  A library without gqhip_set_wide_dims (a build from before the route) is timed on
its only route.  The outputs of the two routes on the timed input are compared bit for bit.  With `--scan` the candidates per row
and the rows the re-rank finished by its in-block scan (gqhip_debug_counters) are read on trained-like and on flat z
(sd = |randn| + 0.5).  Prints one JSON line per (kind, dim).

  python tools/wide_dims_bench.py [--dims 33,40,48,63,64] [--vq-dims 40,64] [--rounds 3] [--round-ms 300] [--scan] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))

N_CODES = 65536
YARDSTICK_DIM = 32


def _events_ms(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


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

    routes = ["exhaustive", "filter"] if hasattr(_lib, "set_wide_dims") else ["exhaustive"]
    z = {"gq": lambda dd: _gq_z(dd, "trained", dev, 100 + dd),
         "vq": lambda dd: torch.randn(16, dd, 32, 32, generator=torch.Generator().manual_seed(dd)).to(dev)}[kind]
    m, zd = _module(kind, d, dev), z(d)
    my, zy = _module(kind, YARDSTICK_DIM, dev), z(YARDSTICK_DIM)
    calls = {r: (m, zd, r) for r in routes}
    calls[f"dim{YARDSTICK_DIM}"] = (my, zy, None)

    def set_route(r):
        if r is not None and len(routes) > 1:
            _lib.set_wide_dims(r)

    res = {"kind": kind, "dim": d, "rows": 16 * 32 * 32, "n": N_CODES, "rounds": a.rounds, "variants": {}}
    try:
        outs, iters = {}, {}
        for name, (mod, zz, r) in calls.items():
            set_route(r)
            if r == "filter":
                res["filter_dim"] = _lib.filter_dim(N_CODES, d)
            outs[name] = _forward(mod, zz)                     # warm-up (sizes the workspace), and the outputs to compare
            one = _events_ms(lambda: _forward(mod, zz), 1)
            iters[name] = max(3, min(200, int(a.round_ms / max(one, 1e-3))))
        if len(routes) > 1:
            res["bit_equal"] = bool(torch.equal(outs["exhaustive"][0], outs["filter"][0]) and torch.equal(outs["exhaustive"][1], outs["filter"][1]))
        times = {k: [] for k in calls}
        for _ in range(a.rounds):
            for name, (mod, zz, r) in calls.items():
                set_route(r)
                times[name].append(_events_ms(lambda: _forward(mod, zz), iters[name]))
        for k, v in times.items():
            res["variants"][k] = {"iters": iters[k], "ms": [round(t, 4) for t in v]}
        if len(routes) > 1:
            res["filter_faster_every_round"] = bool(all(p < e for e, p in zip(times["exhaustive"], times["filter"])))
        if a.scan and kind == "gq" and len(routes) > 1:
            _lib.set_wide_dims("filter")
            _lib.debug_enable(True)
            res["rows_finished_by_scan"], res["candidates_per_decided_row"] = {}, {}
            for zk in ("trained", "flat"):
                _forward(m, _gq_z(d, zk, dev, 200 + d))
                torch.cuda.synchronize()
                fb, cand = _lib.debug_counters(m._ws)
                res["rows_finished_by_scan"][zk] = fb
                res["candidates_per_decided_row"][zk] = round(cand / max(1, 16 * 32 * 32 - fb), 3)
            _lib.debug_enable(False)
    finally:
        set_route("exhaustive")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="33,40,48,63,64")
    ap.add_argument("--vq-dims", default="40,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--round-ms", type=float, default=300.0)
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON lines are appended to (default: print only)")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "wide_dims_bench needs a HIP device"
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
