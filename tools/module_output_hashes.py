#!/usr/bin/env python3
"""Print a sha256 of every output and gradient of one seeded forward (and backward) of each quantiser module, at tiny shapes.

    python tools/module_output_hashes.py [--root TREE] [--bsq-fsq] > listing.txt

For a change that must not move a bit at module level (a refactor of the Python layer between the modules and libgqhip.so): run it
against the parent tree and against the branch (`--root TREE` imports pit_hip from another checkout, whose libgqhip.so must be
built) and compare the two listings line for line.  Cases: GaussianQuantRegularizer in eval() and train(); GaussianQuantRegularizer2
with use_ste on and off, dim_idx 1 and -1, 4-d and 5-d inputs, under autograd and without; VQQuantizer with 1 and 2 sub-codebooks in
train() and eval(); LFQQuantizer with 8 and 16 bits in train(); dequant(indices) after every forward without autograd.  Each on a contiguous, a channels_last (4-d inputs) and a "blc"
tensor.  `--bsq-fsq` appends BSQQuantizer (1 and 2 bits per codebook) and FSQQuantizer in train() and eval() (their fused train steps are
opt-in: unset, the listing must equal the parent's).  A line is `case | name | dtype shape stride | sha256 of the values in logical order`; scalars print their repr."""
import argparse
import hashlib
import os
import sys


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--bsq-fsq", action="store_true", help="append the BSQQuantizer / FSQQuantizer cases")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.root, "vq-vae-from-gaussian-vae_amd"))
    import torch

    from pit_hip.quantization.gaussian import GaussianQuantRegularizer, GaussianQuantRegularizer2
    from pit_hip.quantization.lfq import LFQQuantizer
    from pit_hip.quantization.vq import VQQuantizer

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")

    def emit(case, name, v):
        if isinstance(v, torch.Tensor):
            t = v.detach()
            h = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
            print(f"{case} | {name} | {str(t.dtype)[6:]} {tuple(t.shape)} {tuple(t.stride())} | {h}")
        else:
            print(f"{case} | {name} | {v!r}")

    def tensors(seed, shape, scale=1.0, logvar=None):
        """(input, weight of the loss) as CPU tensors; ``logvar``: the channel axis whose second half holds log-variances."""
        g = torch.Generator().manual_seed(seed)
        x = scale * torch.randn(*shape, generator=g)
        if logvar is not None:
            half = x.shape[logvar] // 2
            x.narrow(logvar, half, half).mul_(0.4).sub_(1.2)
        return x, torch.randn(*shape, generator=g)

    def layouts(shape4, seed, **kw):
        """name -> (format, input, loss weight) for [b, C, h, w]: contiguous, channels_last, and the same values as [b, h w, C]."""
        x, w = tensors(seed, shape4, **kw)
        b, c, hh, ww = shape4
        blc = lambda t: t.permute(0, 2, 3, 1).reshape(b, hh * ww, c).contiguous()
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        return {"contiguous": ("bchw", x, w), "channels_last": ("bchw", cl(x), cl(w)), "blc": ("blc", blc(x), blc(w))}

    def like(w, t, caxis):
        """the loss weight cut to t's channel count"""
        return w.narrow(caxis, 0, t.shape[caxis])

    def run(case, m, x, w, caxis, loss_keys, grad=True, params=()):
        x, w = x.to(dev), w.to(dev)
        x.requires_grad_(grad)
        torch.manual_seed(4321)                       # the modules draw their noise from the device generator
        with torch.enable_grad() if grad else torch.no_grad():
            out, info = m(x)
            emit(case, "out", out)
            for k in sorted(info):
                emit(case, f"info[{k}]", info[k])
            if grad:
                loss = (out * like(w, out, caxis)).sum()
                for k, f in loss_keys:
                    v = info[k]
                    loss = loss + (f * v if v.dim() == 0 else (v * like(w, v, caxis)).sum() * f)
                loss.backward()
                emit(case, "grad_in", x.grad)
                for name, p in params:
                    emit(case, f"grad_{name}", p.grad)
        if not grad and hasattr(m, "dequant") and not isinstance(m, LFQQuantizer):
            with torch.no_grad():
                emit(case, "dequant(indices)", m.dequant(info["indices"]))
        for k in ("lam", "lam_min", "lam_max"):
            if hasattr(m, k):
                emit(case, k, getattr(m, k))

    # ---- GQ1: eval and train -------------------------------------------------------------------------------------------------
    for lay, (fmt, x, w) in layouts((2, 32, 6, 6), 11, logvar=1).items():
        caxis = 1 if fmt == "bchw" else 2
        for mode in ("eval", "train"):
            m = GaussianQuantRegularizer(fmt, 4096, group=8).to(dev)
            m = m.train() if mode == "train" else m.eval()
            run(f"gq1 {mode} {lay}", m, x.clone(), w, caxis, (("kl_loss", 0.37),) if mode == "train" else (), grad=mode == "train")

    # ---- GQ2: use_ste on / off, dim_idx 1 / -1, 4-d and 5-d, autograd and not ------------------------------------------------
    gq2_inputs = []
    for lay, (fmt, x, w) in layouts((2, 32, 6, 6), 12, logvar=1).items():
        gq2_inputs.append((lay, 1 if fmt == "bchw" else -1, x, w))
    x5, w5 = tensors(13, (2, 32, 2, 3, 5), logvar=1)
    gq2_inputs.append(("5d", 1, x5, w5))
    x5l, w5l = tensors(14, (2, 2, 3, 5, 32), logvar=4)
    gq2_inputs.append(("5d_last", -1, x5l, w5l))
    gq2_inputs.append(("5d_moved", -1, x5.movedim(1, -1), w5.movedim(1, -1)))         # not contiguous: the one copy
    for lay, dim_idx, x, w in gq2_inputs:
        for ste in (True, False):
            for mode, grad in (("train", True), ("eval", True), ("eval", False)):
                m = GaussianQuantRegularizer2(8, 4096, dim_idx=dim_idx, use_ste=ste).to(dev)
                m = m.train() if mode == "train" else m.eval()
                run(f"gq2 ste={int(ste)} dim_idx={dim_idx} {mode} grad={int(grad)} {lay}", m, x.clone(), w, dim_idx % x.dim(),
                    (("kl_loss", 0.37), ("zhat_noquant", 0.5), ("std", 0.25)), grad=grad)

    # ---- VQ: 1 and 2 sub-codebooks ------------------------------------------------------------------------------------------
    for K in (1, 2):
        for lay, (fmt, x, w) in layouts((2, 8 * K, 6, 6), 20 + K, scale=0.5).items():
            for mode, grad in (("train", True), ("eval", False)):
                torch.manual_seed(77)
                m = VQQuantizer(fmt, 1024, 8, codebook_num=K)
                m.embedding.weight.data = 0.5 * torch.randn(1024, 8, generator=torch.Generator().manual_seed(5))
                m = m.to(dev)
                m = m.train() if mode == "train" else m.eval()
                run(f"vq K={K} {mode} {lay}", m, x.clone(), w, 1 if fmt == "bchw" else 2, (("codebook_loss", 0.37),), grad=grad,
                    params=(("embedding", m.embedding.weight),) if grad else ())

    # ---- LFQ: 8 and 16 bits --------------------------------------------------------------------------------------------------
    for d in (8, 16):
        for lay, (fmt, x, w) in layouts((2, d, 6, 6), 30 + d, scale=0.02).items():
            m = LFQQuantizer(fmt, 1 << d, 1).to(dev).train()
            run(f"lfq d={d} train {lay}", m, x.clone(), w, 1 if fmt == "bchw" else 2,
                (("entropy_aux_loss", 0.37), ("commit_loss", 1.3)))
    # ---- BSQ (1 and 2 bits per codebook) and FSQ, on request ----------------------------------------------------------------
    if a.bsq_fsq:
        from pit_hip.quantization.bsq import BSQQuantizer
        from pit_hip.quantization.fsq import FSQQuantizer

        for d in (1, 2):
            for lay, (fmt, x, w) in layouts((2, 16 * d, 6, 6), 40 + d).items():
                for mode in ("train", "eval"):
                    m = BSQQuantizer(fmt, 1 << d, 16).to(dev)
                    m = m.train() if mode == "train" else m.eval()
                    run(f"bsq d={d} {mode} {lay}", m, x.clone(), w, 1 if fmt == "bchw" else 2,
                        (("entropy_aux_loss", 0.37),) if mode == "train" else (), grad=mode == "train")
        for lay, (fmt, x, w) in layouts((2, 6, 6, 6), 50, scale=2.0).items():
            for mode in ("train", "eval"):
                m = FSQQuantizer([8, 8, 8, 5, 5, 5], fmt).to(dev)
                m = m.train() if mode == "train" else m.eval()
                run(f"fsq {mode} {lay}", m, x.clone(), w, 1 if fmt == "bchw" else 2, (), grad=mode == "train")
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
