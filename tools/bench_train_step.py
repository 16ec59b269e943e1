#!/usr/bin/env python3
"""Time one training step (forward + backward) through the Gaussian regularizers, or through VQQuantizer, alone on the device.

    python tools/bench_train_step.py [--root TREE] [--iters 200] [--warmup 20] [--label NAME]

Modules: GaussianQuantRegularizer("bchw", 65536, group=16) in train() and GaussianQuantRegularizer2(16, 65536) under autograd, on
z = [16, 32, 32, 32] and [16, 32, 64, 64] (gq_0.25 at 256^2 and 512^2), NCHW and channels_last.  A step is
    zhat, info = m(z);  ((zhat * w).sum() + 0.37 * info["kl_loss"]).backward()
With `--only vq` (VQ cases run only when asked for by name): VQQuantizer("bchw", 65536, 16) in train() with a trained-like codebook
(codes ~ N(0, 1) * 0.5) on z = [16, 16, 32, 32] and [16, 16, 64, 64] (sd3unet_vq_16 at 256^2 and 512^2), NCHW and channels_last; a step is
    zq, info = m(z);  ((zq * w).sum() + 0.37 * info["codebook_loss"]).backward()
with z.grad and embedding.weight.grad both wanted.
With `--only lfq`: LFQQuantizer("bchw", 256, 2) (sd3unet_lfq_16) and LFQQuantizer("bchw", 65536, 1) in train() on
z = [16, 16, 32, 32] ~ 0.02 N(0, 1) (entropies not saturated), NCHW and channels_last; a step is
    q, info = m(z);  ((q * w).sum() + 0.37 * info["entropy_aux_loss"] + 1.3 * info["commit_loss"]).backward()
(the op-by-op path of the 65 536-code case builds the [16 384, 65 536] logits: several GB and tens of ms per step, so time it with a
small `--iters`).
With `--only bsq`: BSQQuantizer("bchw", 2, 16) (sd3unet_bsq_16) in train() on z = [16, 16, 32, 32] ~ N(0, 1); with `--only fsq`:
FSQQuantizer([8, 8, 8, 5, 5, 5], "bchw") (sd3unet_fsq_16) in train() on z = [16, 6, 32, 32] ~ N(0, 1); NCHW and channels_last; a step is
    q, info = m(z);  ((q * w).sum() + 0.37 * info["entropy_aux_loss"]).backward()        (FSQ: without the loss term)
Their fused routes are opt-in (GQHIP_BSQ_TRAIN_FUSED=1 / GQHIP_FSQ_TRAIN_FUSED=1); the JSON line says which route ran ("opt_in").
`--iters` timed steps after `--warmup`, in 10 batches, each between two device events (the time between the events includes whatever
the host makes the device wait for, which is the point: the op-by-op path stops the host three times per step).  Prints one JSON line
per (module, shape, layout): median / min / max over the batches of the per-step time in microseconds.

`--root TREE` imports pit_hip from another checkout (its libgqhip.so must be built): the A/B against a parent commit runs this same
script against both trees, alternating, in one session (profiles/README.md).  GQHIP_TRAIN_FUSED=0 in the environment selects the
torch path of the current tree instead."""
import argparse
import json
import os
import statistics
import sys


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--only", default="", help="substring filter on 'gq1' / 'gq2'; 'vq' / 'lfq' / 'bsq' / 'fsq' run those cases instead")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.root, "vq-vae-from-gaussian-vae_amd"))
    import torch

    from pit_hip.quantization.gaussian import GaussianQuantRegularizer, GaussianQuantRegularizer2

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    batches = 10
    per = max(1, a.iters // batches)

    def timed(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        times = []
        for _ in range(batches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                step()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / per)
        return times

    if a.only == "vq":
        from pit_hip.quantization.vq import VQQuantizer

        for hw in (32, 64):
            for channels_last in (False, True):
                g = torch.Generator().manual_seed(hw)
                z, w = 0.5 * torch.randn(16, 16, hw, hw, generator=g).to(dev), torch.randn(16, 16, hw, hw, generator=g).to(dev)
                if channels_last:
                    z, w = z.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last)
                z.requires_grad_(True)
                m = VQQuantizer("bchw", 65536, 16)
                m.embedding.weight.data = 0.5 * torch.randn(65536, 16, generator=g)
                m = m.to(dev).train()

                def step():
                    z.grad = None
                    m.embedding.weight.grad = None
                    zq, info = m(z)
                    ((zq * w).sum() + 0.37 * info["codebook_loss"]).backward()

                times = timed(step)
                print(json.dumps({"label": a.label, "module": "vq", "z": [16, 16, hw, hw], "channels_last": channels_last,
                                  "steps": per * batches, "us_median": round(statistics.median(times), 2),
                                  "us_min": round(min(times), 2), "us_max": round(max(times), 2),
                                  "fused": os.environ.get("GQHIP_TRAIN_FUSED", "1") != "0"}), flush=True)
        return 0
    if a.only == "lfq":
        from pit_hip.quantization.lfq import LFQQuantizer

        for size, nc in ((256, 2), (65536, 1)):
            for channels_last in (False, True):
                g = torch.Generator().manual_seed(size)
                z, w = 0.02 * torch.randn(16, 16, 32, 32, generator=g).to(dev), torch.randn(16, 16, 32, 32, generator=g).to(dev)
                if channels_last:
                    z, w = z.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last)
                z.requires_grad_(True)
                m = LFQQuantizer("bchw", size, nc).to(dev).train()

                def step():
                    z.grad = None
                    q, info = m(z)
                    ((q * w).sum() + 0.37 * info["entropy_aux_loss"] + 1.3 * info["commit_loss"]).backward()

                torch.cuda.reset_peak_memory_stats()
                times = timed(step)
                print(json.dumps({"label": a.label, "module": f"lfq_{size}x{nc}", "z": [16, 16, 32, 32], "channels_last": channels_last,
                                  "steps": per * batches, "us_median": round(statistics.median(times), 2),
                                  "us_min": round(min(times), 2), "us_max": round(max(times), 2),
                                  "peak_mb": round(torch.cuda.max_memory_allocated() / 1e6, 1),
                                  "fused": os.environ.get("GQHIP_TRAIN_FUSED", "1") != "0"}), flush=True)
        return 0
    if a.only in ("bsq", "fsq"):
        from pit_hip.quantization.bsq import BSQQuantizer
        from pit_hip.quantization.fsq import FSQQuantizer

        c = 16 if a.only == "bsq" else 6
        var = f"GQHIP_{a.only.upper()}_TRAIN_FUSED"
        for channels_last in (False, True):
            g = torch.Generator().manual_seed(c)
            z, w = torch.randn(16, c, 32, 32, generator=g).to(dev), torch.randn(16, c, 32, 32, generator=g).to(dev)
            if channels_last:
                z, w = z.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last)
            z.requires_grad_(True)
            m = (BSQQuantizer("bchw", 2, 16) if a.only == "bsq" else FSQQuantizer([8, 8, 8, 5, 5, 5], "bchw")).to(dev).train()

            def step():
                z.grad = None
                q, info = m(z)
                loss = (q * w).sum()
                (loss + 0.37 * info["entropy_aux_loss"] if a.only == "bsq" else loss).backward()

            times = timed(step)
            fused = os.environ.get("GQHIP_TRAIN_FUSED", "1") != "0"
            print(json.dumps({"label": a.label, "module": a.only, "z": [16, c, 32, 32], "channels_last": channels_last,
                              "steps": per * batches, "us_median": round(statistics.median(times), 2),
                              "us_min": round(min(times), 2), "us_max": round(max(times), 2), "fused": fused,
                              "opt_in": fused and os.environ.get(var, "0") == "1"}), flush=True)
        return 0
    for kind in ("gq1", "gq2"):
        if a.only and a.only not in kind:
            continue
        for hw in (32, 64):
            for channels_last in (False, True):
                g = torch.Generator().manual_seed(hw)
                z = torch.cat([0.95 * torch.randn(16, 16, hw, hw, generator=g), -0.9 + 0.5 * torch.randn(16, 16, hw, hw, generator=g)], 1)
                z, w = z.to(dev), torch.randn(16, 16, hw, hw, generator=g).to(dev)
                if channels_last:
                    z, w = z.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last)
                z.requires_grad_(True)
                m = (GaussianQuantRegularizer("bchw", 65536, group=16) if kind == "gq1" else GaussianQuantRegularizer2(16, 65536))
                m = m.to(dev).train()

                def step():
                    z.grad = None
                    zhat, info = m(z)
                    ((zhat * w).sum() + 0.37 * info["kl_loss"]).backward()

                times = timed(step)
                print(json.dumps({"label": a.label, "module": kind, "z": [16, 32, hw, hw], "channels_last": channels_last,
                                  "steps": per * batches, "us_median": round(statistics.median(times), 2),
                                  "us_min": round(min(times), 2), "us_max": round(max(times), 2),
                                  "fused": os.environ.get("GQHIP_TRAIN_FUSED", "1") != "0"}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
