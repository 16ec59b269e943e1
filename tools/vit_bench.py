#!/usr/bin/env python3
"""Device timing of the BSQ-ViT backbone (pit_hip.modules.vit) with device events after warm-up:

  * the fused attention kernel (_lib.mha_fwd, csrc/gq_attn.h) at ViT-B/8's two shapes, B 16 x H 12 x L 1024 (256^2) and
    B 2 x H 12 x L 4096 (512^2), d 64: us per call and TF/s counting 4 B H L^2 d FLOPs, against torch's fp32
    F.scaled_dot_product_attention on the same operands in the same process (the kernels torch launched are named);
  * bsqvit_gq_{0.25,0.50,1.00} (tests/golden copies of the shipped YAMLs, random init), encode -> GQ -> decode at bs 16,
    256^2, with the HIP attention route and with torch's route (HIP_ATTN = False): images/s, ms per step and the
    encoder / quantiser / decoder split.

Prints one JSON line per measurement (and appends them to --out when given).

  python tools/vit_bench.py [--iters 20] [--warmup 5] [--bs 16] [--configs 0.25,0.50,1.00] [--out FILE]"""
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


def sdpa(qkv, H):
    B, L, E3 = qkv.shape
    E = E3 // 3
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, L, H, E // H).transpose(1, 2) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, E)


def sdpa_kernels(qkv, H):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        sdpa(qkv, H)
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if e.device_type.name == "CUDA"}, key=len)
    return [n[:80] for n in names][:6]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def bench_attention(args):
    for B, H, L in ((16, 12, 1024), (2, 12, 4096)):
        d = 64
        qkv = torch.randn(B, L, 3 * H * d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
        flops = 4.0 * B * H * L * L * d
        with torch.no_grad():
            ms_hip = timed(lambda: _lib.mha_fwd(qkv, H), args.iters, args.warmup)
            ms_t = timed(lambda: sdpa(qkv, H), args.iters, args.warmup)
            kern = [] if args.no_kernel_names else sdpa_kernels(qkv, H)
        emit(dict(bench="vit_attention", B=B, H=H, L=L, d=d, hip_us=round(ms_hip * 1e3, 1),
                  hip_tflops=round(flops / ms_hip / 1e9, 1), torch_sdpa_fp32_us=round(ms_t * 1e3, 1),
                  torch_sdpa_fp32_tflops=round(flops / ms_t / 1e9, 1), speedup=round(ms_t / ms_hip, 2),
                  torch_sdpa_kernels=kern), args.out)


def bench_steps(args):
    for name in args.configs.split(","):
        cfg = load_config(os.path.join(ROOT, "tests", "golden", f"bsqvit_gq_{name}.yaml"))
        torch.manual_seed(0)
        eng = instantiate_from_config(cfg["model"]).eval().to(DEV)
        x = torch.rand(args.bs, 3, 256, 256, device=DEV) * 2 - 1
        for route in (True, False):
            vit.HIP_ATTN = route
            with torch.no_grad():
                z = eng.encoder(x)
                zq, _ = eng.regularization(z)
                ms_step = timed(lambda: eng.decode(eng.encode(x)), args.iters, args.warmup)
                ms_enc = timed(lambda: eng.encoder(x), args.iters, args.warmup)
                ms_q = timed(lambda: eng.regularization(z), args.iters, args.warmup)
                ms_dec = timed(lambda: eng.decoder(zq), args.iters, args.warmup)
            emit(dict(bench="vit_step", config=f"bsqvit_gq_{name}", bs=args.bs, size=256,
                      route="hip_attn" if route else "torch_attn", ms_per_step=round(ms_step, 2),
                      images_per_s=round(args.bs / ms_step * 1e3, 1), encoder_ms=round(ms_enc, 2),
                      quantiser_ms=round(ms_q, 2), decoder_ms=round(ms_dec, 2)), args.out)
        vit.HIP_ATTN = True
        del eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--configs", default="0.25,0.50,1.00")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--no-kernel-names", action="store_true", help="skip the torch profiler pass (e.g. under rocprofv3)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    bench_attention(args)
    if not args.skip_steps:
        bench_steps(args)


if __name__ == "__main__":
    main()
