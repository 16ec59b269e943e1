#!/usr/bin/env python3
"""Device timing of SSIM / MS-SSIM (csrc/gq_ssim.h) at bs 16 x 3 x 256^2 and 512^2, with device events after warm-up:

  * the fused SSIM + MS-SSIM call (gq_ssim_f32, five launches),
  * the three-metric step record (gq_step_record_ssim_f32) against the one-metric record (gq_step_record_f32),
  * the torch restatement of pytorch_msssim's op sequence on the same device (grouped conv2d + avg_pool2d in fp32: what the
    reference's pit/evaluations/ssim.py costs on a GPU).

FLOPs and bytes come from the shapes (the algorithm's need, not what the tiles re-read); the share of peak is the larger of
fp64 FLOPs / 78.6 TFLOP/s (the MI355X's published fp64 vector peak) and bytes / 6.3 TB/s (achievable HBM), over the measured
time, and the bound that gives it is named.  Prints one JSON line per shape.

  python tools/ssim_bench.py [--iters 50] [--warmup 10] [--sizes 256,512]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))
from pit_hip import _lib  # noqa: E402
from pit_hip.eval_dist import StepRecord, _ms_ssim_torch, _ssim_torch, ssim_window  # noqa: E402

FP64_PEAK = 78.6e12
HBM_BW = 6.3e12


def model(B, C, H, W):
    """(fp64 FLOPs, bytes) of SSIM + MS-SSIM over the five levels: per level the W pass at H x Wo positions and the H pass at
    Ho x Wo, 5 moments x 11 taps x 2 FLOPs each, 3 products per input and ~15 FLOPs per map position; bytes: level 0 reads
    both fp32 images, every later level reads its fp64 planes, each pooling step reads its level and writes the next."""
    flops = byts = 0.0
    h, w = H, W
    for lvl in range(5):
        ho, wo = max(h - 10, 1), max(w - 10, 1)
        flops += B * C * (h * w * 3 + h * wo * 5 * 22 + ho * wo * (5 * 22 + 15))
        byts += B * C * h * w * 2 * (4 if lvl == 0 else 8)
        if lvl < 4:
            hn, wn = (h + 1) // 2, (w + 1) // 2
            byts += B * C * (h * w * 2 * (4 if lvl == 0 else 8) + hn * wn * 2 * 8)
            h, w = hn, wn
    return flops, byts


def time_ms(fn, iters, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--bs", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ssim_bench needs a HIP device"
    dev = torch.device("cuda:0")
    B, C = a.bs, 3
    for size in [int(s) for s in a.sizes.split(",")]:
        g = torch.Generator().manual_seed(size)
        x = (torch.rand(B, C, size, size, generator=g) * 2 - 1).to(dev).contiguous(memory_format=torch.channels_last)
        y = (x + 0.05 * torch.randn(B, C, size, size, generator=g).to(dev)).contiguous(memory_format=torch.channels_last)
        tokens = (size // 16) ** 2
        idx = torch.randint(0, 65536, (B, 1, size // 16, size // 16), generator=g).to(dev)
        ws = {}
        fused = time_ms(lambda: _lib.image_quality(x, y, True, True, ws), a.iters, a.warmup)
        lay3, lay1 = StepRecord(B, tokens, 3), StepRecord(B, tokens, 1)
        rec3 = time_ms(lambda: lay3.pack_with_metrics(idx, x, y), a.iters, a.warmup)
        rec1 = time_ms(lambda: lay1.pack_with_psnr(idx, x, y), a.iters, a.warmup)
        win = ssim_window()

        def torch_seq():
            X, Y = (x + 1) * 127.5, (y + 1) * 127.5
            _ssim_torch(X, Y, win)[0].mean(1)
            _ms_ssim_torch(X, Y, win)

        ref = time_ms(torch_seq, max(a.iters // 5, 3), max(a.warmup // 5, 2))
        flops, byts = model(B, C, size, size)
        t_f, t_b = flops / FP64_PEAK, byts / HBM_BW
        bound = "fp64 vector" if t_f >= t_b else "HBM"
        print(json.dumps({
            "shape": [B, C, size, size], "fused_ssim_msssim_ms": round(fused, 4), "record3_ms": round(rec3, 4),
            "record1_psnr_ms": round(rec1, 4), "torch_sequence_ms": round(ref, 4),
            "speedup_vs_torch": round(ref / fused, 2), "gflop_fp64": round(flops / 1e9, 3), "mbytes": round(byts / 1e6, 2),
            "fused_tflops": round(flops / fused / 1e9, 2), "fused_tbps": round(byts / fused / 1e9, 3),
            "bound": bound, "share_of_peak": round(max(t_f, t_b) / (fused * 1e-3), 3)}), flush=True)


if __name__ == "__main__":
    main()
