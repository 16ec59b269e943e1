#!/usr/bin/env python3
"""Device timing of TRAINING the BSQ-ViT backbone on the kernel route (pit_hip.modules.vit.HIP_ATTN_TRAIN), with device events
after warm-up, everything in one process:

  (a) attention forward + backward alone (_lib.mha_fwd_lse + _lib.mha_bwd, csrc/gq_attn.h / gq_attn_bwd.h) at ViT-B/8's two
      shapes, B 16 x H 12 x L 1024 (256^2) and B 2 x H 12 x L 4096 (512^2), d 64: us per forward, per backward and per pair, TF/s
      counting 4 B H L^2 d FLOPs forward and 10 B H L^2 d backward (the five products of the formulas; the kernels issue seven,
      S and dP are formed in both), against torch's fp32 F.scaled_dot_product_attention forward + backward on the same operands;
  (b) forward + backward of the full-size bsqvit_gq_0.25 encoder + decoder (tests/golden copy of the shipped YAML, random init,
      train() mode, loss = mean of the reconstruction) at bs 16, 256^2, with HIP_ATTN_TRAIN on and off (off = torch's route for
      every grad-enabled call, the route before the flag existed).  The decoder is fed the encoder's mean half, so that the
      gradient runs through all 24 layers without the quantiser.

Prints one JSON line per measurement (and appends them to --out when given).

  python tools/vit_train_bench.py [--iters 20] [--warmup 5] [--bs 16] [--rounds 2] [--skip-steps] [--skip-attention] [--out FILE]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))
from pit_hip import _lib  # noqa: E402
from pit_hip.modules import vit  # noqa: E402
from pit_hip.util import instantiate_from_config, load_config  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def bench_attention(args):
    for B, H, L in ((16, 12, 1024), (2, 12, 4096)):
        d = 64
        g = torch.Generator(device=DEV).manual_seed(0)
        qkv = torch.randn(B, L, 3 * H * d, device=DEV, generator=g)
        dout = torch.randn(B, L, H * d, device=DEV, generator=g)
        out, lse = _lib.mha_fwd_lse(qkv, H)
        ms_f = timed(lambda: _lib.mha_fwd_lse(qkv, H), args.iters, args.warmup)
        ms_b = timed(lambda: _lib.mha_bwd(qkv, out, lse, dout, H), args.iters, args.warmup)

        def pair():
            o, s = _lib.mha_fwd_lse(qkv, H)
            _lib.mha_bwd(qkv, o, s, dout, H)

        ms_p = timed(pair, args.iters, args.warmup)

        E = H * d
        t = qkv.clone().requires_grad_(True)
        do4 = dout.reshape(B, L, H, d).transpose(1, 2)

        def sdpa_fwd():
            q, k, v = (t[..., i * E:(i + 1) * E].reshape(B, L, H, d).transpose(1, 2) for i in range(3))
            return F.scaled_dot_product_attention(q, k, v)

        def sdpa_pair():
            t.grad = None
            sdpa_fwd().backward(do4)

        with torch.no_grad():
            ms_tf = timed(sdpa_fwd, args.iters, args.warmup)
        ms_tp = timed(sdpa_pair, args.iters, args.warmup)
        unit = B * H * L * L * d / 1e9
        emit(dict(bench="vit_attention_train", B=B, H=H, L=L, d=d, hip_fwd_lse_us=round(ms_f * 1e3, 1),
                  hip_bwd_us=round(ms_b * 1e3, 1), hip_fwd_bwd_us=round(ms_p * 1e3, 1),
                  hip_bwd_tflops=round(10 * unit / ms_b, 1), hip_bwd_over_fwd=round(ms_b / ms_f, 2),
                  torch_sdpa_fp32_fwd_us=round(ms_tf * 1e3, 1), torch_sdpa_fp32_fwd_bwd_us=round(ms_tp * 1e3, 1),
                  speedup_fwd_bwd=round(ms_tp / ms_p, 2)), args.out)


def bench_step(args):
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "bsqvit_gq_0.25.yaml"))
    torch.manual_seed(0)
    eng = instantiate_from_config(cfg["model"]).train().to(DEV)
    x = torch.rand(args.bs, 3, 256, 256, device=DEV) * 2 - 1
    params = list(eng.encoder.parameters()) + list(eng.decoder.parameters())

    def step():
        for p in params:
            p.grad = None
        z = eng.encoder(x)
        eng.decoder(z[..., :z.shape[-1] // 2]).mean().backward()

    res = {True: [], False: []}
    for _ in range(args.rounds):                                 # the two routes alternate: drift of a shared machine shows
        for route in (True, False):
            vit.HIP_ATTN_TRAIN = route
            res[route].append(timed(step, args.iters, args.warmup))
    vit.HIP_ATTN_TRAIN = False
    for route in (True, False):
        ms = min(res[route])
        emit(dict(bench="vit_train_step", config="bsqvit_gq_0.25", bs=args.bs, size=256, what="encoder + decoder fwd + bwd",
                  route="hip_attn_train" if route else "torch_attn", ms_per_step=round(ms, 2),
                  ms_per_step_rounds=[round(m, 2) for m in res[route]], images_per_s=round(args.bs / ms * 1e3, 1)), args.out)
    emit(dict(bench="vit_train_step_ratio", torch_over_hip=round(min(res[False]) / min(res[True]), 3)), args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2, help="alternating rounds of the two routes of the train step")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not args.skip_attention:
        bench_attention(args)
    if not args.skip_steps:
        bench_step(args)


if __name__ == "__main__":
    main()
