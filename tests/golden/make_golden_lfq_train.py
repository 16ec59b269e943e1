"""LFQ train-step fixture (same rules as make_golden*.py: build container only, imports the reference, stores DATA).

    python tests/golden/make_golden_lfq_train.py <path of the reference checkout>

  g25_lfq_train_step.npz   one train() step of the reference's LFQQuantizer on the CPU under autograd for the cases of
                      tests/lfq_train_ref.py:CASES, once in fp32 and once in fp64 (module.double(): the codebook buffer is cast
                      too).  loss = sum(quantized * w) + g_aux * info["entropy_aux_loss"] + g_commit * info["commit_loss"];
                      backward().  x and w hold float16-exact values and are stored as float16.
                      Stored per case: x, w, g_aux, g_commit; the fp32 outputs quantized, indices, the four scalars and the fp32
                      autograd grad_x; the fp64 scalars ({name}64) and grad_x64; the sums of |terms| of tests/lfq_train_ref.py
                      ({name}_abs, grad_x_abs); and per output {name}_ref_err / grad_x_ref_err =
                      max |reference fp32 - reference fp64| / (2^-24 sum |terms|): the reference's own fp32 error, the yardstick
                      of the GPU tests.
Asserted here: the factorised fp64 formulas equal the reference's fp64 run (scalars to 1e-12 relative, grad_x to 1e-7 of its sum of
|terms|), so a wrong checker cannot make a fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pit.quantization.lfq import LFQQuantizer as RefLFQ  # noqa: E402

import lfq_train_ref as R  # noqa: E402


def run(ref, x, w, cl):
    xt = x.clone()
    if cl:
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt.requires_grad_(True)
    quantized, info = ref(xt)
    (quantized * w).sum().add(R.G_AUX * info["entropy_aux_loss"]).add(R.G_COMMIT * info["commit_loss"]).backward()
    return quantized.detach(), info, xt.grad


def make_case(tag, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = (cfg["scale"] * torch.randn(cfg["shape"], generator=g)).half().float()
    if cfg.get("special"):
        flat = x.reshape(-1)
        for k, v in enumerate((0.0, 1e-4, -1e-4, 50.0, -50.0, 0.0)):
            flat[7 * k + 3] = float(np.float16(v))
    w = torch.randn(cfg["shape"], generator=g).half().float()
    kw = dict(sample_minimization_weight=cfg.get("w_s", 1.0), batch_maximization_weight=cfg.get("w_b", 1.0))
    cl = bool(cfg.get("channels_last"))
    q32, i32, g32 = run(RefLFQ(cfg["format"], 1 << cfg["d"], cfg["nc"], **kw).train(), x, w, cl)
    q64, i64, g64 = run(RefLFQ(cfg["format"], 1 << cfg["d"], cfg["nc"], **kw).double().train(), x.double(), w.double(), cl)
    assert torch.equal(i32["indices"], i64["indices"]) and torch.equal(q32.double(), q64)
    s = R.factorised64(x.numpy(), cfg, w.numpy(), R.G_AUX, R.G_COMMIT)
    out = {"x": x.numpy().astype(np.float16), "w": w.numpy().astype(np.float16), "g_aux": np.float64(R.G_AUX),
           "g_commit": np.float64(R.G_COMMIT), "quantized": q32.numpy(), "indices": i32["indices"].numpy(),
           "grad_x": g32.numpy(), "grad_x64": g64.numpy(), "grad_x_abs": s["grad_x_abs"].astype(np.float32)}
    assert np.array_equal(out["x"].astype(np.float32), x.numpy()) and np.array_equal(out["w"].astype(np.float32), w.numpy())
    # (the reference's fp64 softmax backward cancels among logits of magnitude 1e4 where x = +-50: 2e-8 of the sum of |terms| there)
    assert np.all(np.abs(s["grad_x"] - out["grad_x64"]) <= 1e-7 * s["grad_x_abs"])
    out["grad_x_ref_err"] = np.float64(R.err_units(out["grad_x"], out["grad_x64"], out["grad_x_abs"].astype(np.float64)))
    line = [f"grad_x {float(out['grad_x_ref_err']):.1f}"]
    for name in R.SCALARS:
        v32, v64 = float(i32[name].detach()), float(i64[name].detach())
        assert abs(s[name] - v64) <= 1e-12 * max(abs(v64), s[name + "_abs"]), (name, s[name], v64)
        out[name], out[name + "64"], out[name + "_abs"] = np.float32(v32), np.float64(v64), np.float64(s[name + "_abs"])
        out[name + "_ref_err"] = np.float64(R.err_units(v32, v64, s[name + "_abs"]))
        line.append(f"{name} {float(out[name + '_ref_err']):.1f}")
    print(f"{tag}: rows {x.numel() // cfg['d']} max|grad| {np.abs(out['grad_x64']).max():.3g} ref_err: " + ", ".join(line))
    return {f"{tag}_{k}": v for k, v in out.items()}


if __name__ == "__main__":
    out = {}
    for i, (tag, cfg) in enumerate(R.CASES.items()):
        out.update(make_case(tag, cfg, 2500 + i))
    path = os.path.join(HERE, "g25_lfq_train_step.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))
