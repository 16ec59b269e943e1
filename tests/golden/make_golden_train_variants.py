"""Train-step fixtures for the kernel variants g25 / g26 never launch (same rules as make_golden*.py: build container only, imports
the reference, stores DATA).

    python tests/golden/make_golden_train_variants.py <path of the reference checkout>

  g28_lfq_train_variants.npz   the reference's LFQQuantizer for tests/lfq_train_ref.py:VARIANT_CASES, run exactly as
                      make_golden_lfq_train.py runs CASES (fp32 and fp64 CPU autograd of the same loss, G_AUX, G_COMMIT).
  g29_bsq_train_variants.npz   the reference's BSQQuantizer for tests/bsq_fsq_train_ref.py:BSQ_VARIANT_CASES, run as
                      make_golden_bsq_fsq_train.py runs BSQ_CASES.
Stored per case: x and w (float16-exact, as float16), g_aux (g_commit), the fp32 indices and scalars, the fp64 scalars ({name}64),
their sums of |terms| ({name}_abs), and {name}_ref_err / grad_x_ref_err = max |reference fp32 - reference fp64| / (2^-24 sum
|terms|).  The files stay under 400 KB, so of the tensors of x's shape only these are kept:
  LFQ  x, w and grad_x64, the reference's fp64 autograd.  Asserted here: the checker (tests/lfq_train_ref.py:factorised64) equals it
       to 1e-7 of the sum of |terms|, the bound of g25, and the scalars to 1e-12.  A tighter bound would measure the reference, not
       the checker: its fp64 softmax backward over 2^d logits is off by up to 3.6e-12 of the sum of |terms| at d = 13 (printed per
       case), where the checker lies within 6e-16 of the same dense formula evaluated in 80-bit arithmetic.
       "blc_d13x4" is the memory of "blc_d13" viewed as [1, 75, 52]: its three tensors are not stored twice
       (lfq_train_ref.variant); asserted here: the reference's grad_x64 of the two views is the same, bit for bit.
  BSQ  x and w.  grad_x64 is the checker's (tests/bsq_fsq_train_ref.py:bsq64); asserted here: it equals the reference's fp64
       autograd to 1e-12 of the sum of |terms| on every case (measured: <= 7e-16).  quantized is +-q_scale within three roundings,
       asserted here as the tests assert it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_bsq_fsq_train as MB  # noqa: E402  (both put the reference and tests/ on the path)
import make_golden_lfq_train as ML  # noqa: E402

from pit.quantization.bsq import BSQQuantizer as RefBSQ  # noqa: E402
from pit.quantization.lfq import LFQQuantizer as RefLFQ  # noqa: E402

import bsq_fsq_train_ref as RB  # noqa: E402
import lfq_train_ref as RL  # noqa: E402

AGREE = 1e-12


def finish(R, out, s, i32, i64, g32, g64, agree):
    """The shared tail: the checker against the fp64 run, the fp32 run's error against it, the scalars."""
    dev = float((np.abs(s["grad_x"] - g64.numpy()) / s["grad_x_abs"]).max())
    assert dev <= agree, dev
    out["grad_x_ref_err"] = np.float64(R.err_units(g32.numpy(), g64.numpy(), s["grad_x_abs"]))
    line = [f"checker - fp64 autograd {dev:.1e}", f"grad_x {float(out['grad_x_ref_err']):.1f}"]
    for name in R.SCALARS:
        v32, v64 = float(i32[name].detach()), float(i64[name].detach())
        assert abs(s[name] - v64) <= AGREE * max(abs(v64), s[name + "_abs"]), (name, s[name], v64)
        out[name], out[name + "64"], out[name + "_abs"] = np.float32(v32), np.float64(v64), np.float64(s[name + "_abs"])
        out[name + "_ref_err"] = np.float64(R.err_units(v32, v64, s[name + "_abs"]))
        line.append(f"{name} {float(out[name + '_ref_err']):.2f}")
    return ", ".join(line)


def inputs(cfg, seed, made):
    if "same_as" in cfg:
        return (made[cfg["same_as"] + "_" + k].astype(np.float32).reshape(cfg["shape"]) for k in ("x", "w"))
    g = torch.Generator().manual_seed(seed)
    x = (cfg["scale"] * torch.randn(cfg["shape"], generator=g)).half().float()
    return x.numpy(), torch.randn(cfg["shape"], generator=g).half().float().numpy()


def make_lfq(tag, cfg, seed, made):
    x, w = (torch.from_numpy(a.copy()) for a in inputs(cfg, seed, made))
    cl = bool(cfg.get("channels_last"))
    q32, i32, g32 = ML.run(RefLFQ(cfg["format"], 1 << cfg["d"], cfg["nc"]).train(), x, w, cl)
    q64, i64, g64 = ML.run(RefLFQ(cfg["format"], 1 << cfg["d"], cfg["nc"]).double().train(), x.double(), w.double(), cl)
    assert torch.equal(i32["indices"], i64["indices"]) and torch.equal(q32.double(), q64)
    assert torch.equal(q32, x + (torch.where(x > 0, 1.0, -1.0) - x))
    s = RL.factorised64(x.numpy(), cfg, w.numpy(), RL.G_AUX, RL.G_COMMIT)
    out = {"x": x.numpy().astype(np.float16), "w": w.numpy().astype(np.float16), "g_aux": np.float64(RL.G_AUX),
           "g_commit": np.float64(RL.G_COMMIT), "indices": i32["indices"].numpy(), "grad_x64": g64.numpy()}
    assert np.array_equal(out["x"].astype(np.float32), x.numpy()) and np.array_equal(out["w"].astype(np.float32), w.numpy())
    print(f"lfq {tag}: rows {x.numel() // cfg['d']}: " + finish(RL, out, s, i32, i64, g32, g64, 1e-7))
    if "same_as" in cfg:                                       # lfq_train_ref.variant views the other case's tensors
        assert np.array_equal(out["grad_x64"].reshape(-1), made[cfg["same_as"] + "_grad_x64"].reshape(-1))
        for k in ("x", "w", "grad_x64"):
            del out[k]
    return {f"{tag}_{k}": v for k, v in out.items()}


def make_bsq(tag, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = MB.bsq_x(cfg, g)
    w = torch.randn(cfg["shape"], generator=g).half().float()
    cl = bool(cfg.get("channels_last"))
    q32, i32, g32 = MB.run_bsq(RefBSQ(cfg["format"], 1 << cfg["d"], 16).train(), x, w, cl)
    q64, i64, g64 = MB.run_bsq(RefBSQ(cfg["format"], 1 << cfg["d"], 16).double().train(), x.double(), w.double(), cl)
    assert torch.equal(i32["indices"], i64["indices"])
    s = RB.bsq64(x.numpy(), cfg, w.numpy(), RB.G_AUX)
    assert np.array_equal(s["indices"], i64["indices"].numpy())
    qs = np.float32(1.0 / np.sqrt(16 * cfg["d"]))
    assert np.all(np.abs(q32.numpy() - np.where(s["u"] > 0, qs, -qs)) <= 3 * RB.U * qs)          # quantized is +-q_scale: not stored
    out = {"x": x.numpy().astype(np.float16), "w": w.numpy().astype(np.float16), "g_aux": np.float64(RB.G_AUX),
           "indices": i32["indices"].numpy()}
    assert np.array_equal(out["x"].astype(np.float32), x.numpy()) and np.array_equal(out["w"].astype(np.float32), w.numpy())
    print(f"bsq {tag}: positions {x.numel() // (16 * cfg['d'])}: " + finish(RB, out, s, i32, i64, g32, g64, AGREE))
    return {f"{tag}_{k}": v for k, v in out.items()}


def save(name, out):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(name, "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < (400 << 10)


if __name__ == "__main__":
    out = {}
    for i, (tag, cfg) in enumerate(RL.VARIANT_CASES.items()):
        out.update(make_lfq(tag, cfg, 2800 + i, out))
    save("g28_lfq_train_variants.npz", out)
    out = {}
    for i, (tag, cfg) in enumerate(RB.BSQ_VARIANT_CASES.items()):
        out.update(make_bsq(tag, cfg, 2900 + i))
    save("g29_bsq_train_variants.npz", out)
