#!/usr/bin/env python3
"""Device timing of the bit-packed step records (csrc/gq_aux.h: step_record_bits_kernel) against the uint16 records, and the wall
time of evaluate_sharded with and without the per-step host range check.

  records: at bs 16 x 3 x 256^2, 4096 indices, raw library calls on one preallocated record and workspace, device events around
    `--iters` calls, `--rounds` rounds with the variants alternating inside every round:
      parent16   gq_step_record_f32 of --parent-lib (a libgqhip.so built from the parent commit; left out when not given)
      this16     gq_step_record_f32 of this tree
      bits16     gq_step_record_bits_f32, index_bits 16, n_codes 65536
      bits18     gq_step_record_bits_f32, index_bits 18, n_codes 2^18
    and the same four for the three-metric records (gq_step_record_ssim_f32 / gq_step_record_ssim_bits_f32).  Per variant:
    median / min / max of the rounds' per-call microseconds; `spread` = max - min.
  eval: evaluate_sharded at world size 1 over `--eval-steps` batches of 16 images with an identity encoder / decoder around a
    VQQuantizer(n = 65536, dim = 4) (256 tokens per image), host clock around the call and a device synchronise:
      check_range  the uint16 record, int(max) / int(min) of the indices on the host every step (today's evaluate_sharded)
      n_codes      the bit-packed record, no host read in the loop, the running histogram on the device
    The model is a stub, so the step is short and the host read is a large share of it; with the real 32 ms step the same
    absolute saving per step is a small share.

Prints one JSON line per section.

  python tools/wire_bits_bench.py [--parent-lib PATH] [--iters 200] [--rounds 9] [--eval-steps 50] [--only records|eval]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))
from pit_hip import _lib  # noqa: E402
from pit_hip import eval_dist as E  # noqa: E402


def _parent(path):
    """The four uint16-record entry points of another libgqhip.so."""
    L = ctypes.CDLL(path)
    for name in ("gq_step_record_workspace_bytes", "gq_step_record_f32", "gq_step_record_ssim_workspace_bytes", "gq_step_record_ssim_f32"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return L


def _events_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _rounds(variants, iters, rounds, warmup=20):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(_events_us(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "spread_us": round(max(v) - min(v), 3)} for k, v in times.items()}


def records(a, dev):
    B, C, S = 16, 3, 256
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(B, C, S, S, generator=g) * 2 - 1).to(dev).contiguous(memory_format=torch.channels_last)
    y = (x + 0.05 * torch.randn(B, C, S, S, generator=g).to(dev)).contiguous(memory_format=torch.channels_last)
    idx = torch.randint(0, 65536, (B * 256,), generator=g).to(dev)
    per, n_idx, st = C * S * S, idx.numel(), torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    libs = {"this16": L}
    if a.parent_lib:
        libs = {"parent16": _parent(a.parent_lib), "this16": L}
    rec = torch.zeros(3 * B + n_idx + 1, dtype=torch.int32, device=dev)
    ws = torch.zeros(L.gq_step_record_ssim_bits_workspace_bytes(B, C, S, S), dtype=torch.uint8, device=dev)
    one, three = {}, {}
    for name, lib in libs.items():
        one[name] = lambda lib=lib: lib.gq_step_record_f32(x.data_ptr(), y.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, per, n_idx,
                                                          ws.data_ptr(), ws.numel(), st)
        three[name] = lambda lib=lib: lib.gq_step_record_ssim_f32(x.data_ptr(), y.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, C, S, S, 1,
                                                                 n_idx, ws.data_ptr(), ws.numel(), st)
    for name, w in (("bits16", 16), ("bits18", 18)):
        one[name] = lambda w=w: L.gq_step_record_bits_f32(x.data_ptr(), y.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, per, n_idx, w,
                                                          1 << w, ws.data_ptr(), ws.numel(), st)
        three[name] = lambda w=w: L.gq_step_record_ssim_bits_f32(x.data_ptr(), y.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, C, S, S,
                                                                 1, n_idx, w, 1 << w, ws.data_ptr(), ws.numel(), st)
    for k, fn in {**one, **{k + "_3": v for k, v in three.items()}}.items():
        assert fn() == 0, k
    out = {"section": "records", "shape": [B, C, S, S], "n_idx": n_idx, "iters": a.iters, "rounds": a.rounds,
           "one_metric": _rounds(one, a.iters, a.rounds), "three_metric": _rounds(three, max(a.iters // 4, 10), a.rounds)}
    assert int(ws.count_nonzero()) == 0
    print(json.dumps(out), flush=True)


class _Model:
    def __init__(self, q):
        self.q = q

    def encode(self, x, return_reg_log=True):
        return self.q(x)

    def decode(self, z):
        return z


def eval_loop(a, dev):
    from pit_hip.quantization.vq import VQQuantizer

    n, bs, steps = 65536, 16, a.eval_steps
    torch.manual_seed(2)
    q = VQQuantizer("bchw", n, 4)
    q.embedding.weight.data.normal_()
    model = _Model(q.eval().to(dev))
    images = torch.randn(bs * steps, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    ids = [torch.arange(s * bs, (s + 1) * bs, device=dev) for s in range(steps)]

    def run(n_codes):
        it = iter(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = E.evaluate_sharded(model, lambda _: images[next(it)], bs * steps, bs, 0, 1, dev, 256, n_codes=n_codes)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    times = {"check_range": [], "n_codes": []}
    for r in range(a.rounds + 1):                 # round 0 warms both paths up
        for name, n_codes in (("check_range", None), ("n_codes", n)):
            ms, out = run(n_codes)
            if r:
                times[name].append(ms)
    same = torch.equal(run(None)[1]["indices"], run(n)[1]["indices"])
    print(json.dumps({"section": "eval", "steps": steps, "bs": bs, "tokens_per_image": 256, "codes": n, "rounds": a.rounds,
                      "indices_equal": same,
                      **{k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                             "per_step_us": round(statistics.median(v) * 1e3 / steps, 1)} for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--eval-steps", type=int, default=50)
    ap.add_argument("--only", choices=("records", "eval"), default=None, help="one section (records: the workload of a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "wire_bits_bench needs a HIP device"
    dev = torch.device("cuda:0")
    if a.only != "eval":
        records(a, dev)
    if a.only != "records":
        eval_loop(a, dev)


if __name__ == "__main__":
    main()
