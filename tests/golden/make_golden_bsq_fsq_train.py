"""BSQ / FSQ train-step fixtures (same rules as make_golden*.py: build container only, imports the reference, stores DATA).

    python tests/golden/make_golden_bsq_fsq_train.py <path of the reference checkout>

  g26_bsq_train_step.npz   one train() step of the reference's BSQQuantizer on the CPU under autograd for the cases of
                      tests/bsq_fsq_train_ref.py:BSQ_CASES, once in fp32 and once in fp64 (module.double()).
                      loss = sum(quantized * w) + g_aux * info["entropy_aux_loss"]; backward().  x and w hold float16-exact values
                      and are stored as float16.  Stored per case: x, w, g_aux; the fp32 outputs quantized, indices, the three
                      scalars and the fp32 autograd grad_x; the fp64 scalars ({name}64) and grad_x64; the sums of |terms| of
                      tests/bsq_fsq_train_ref.py ({name}_abs, grad_x_abs); and per output {name}_ref_err / grad_x_ref_err =
                      max |reference fp32 - reference fp64| / (2^-24 sum |terms|): the reference's own fp32 error, the yardstick of
                      the GPU tests.  Plus ``underflow_*``: a forward-only fp32 run (x stored as float32) with a row holding 1e18,
                      1e-30, -1e-30 and zeros, whose quotient underflows: the fp64 run gives the 1e-30 element bit 1, the fp32 run
                      bit 0, so only the fp32 run is stored.
  g27_fsq_train_step.npz   the reference's FSQQuantizer for FSQ_CASES: forward() in fp32 under autograd with loss = sum(zhat * w)
                      (zhat, indices, grad_z), its _quantize() on a float64 tensor for the fp64 gradient (forward() itself casts to
                      float32), the oracle's rounding margin per position, grad_z_abs and grad_z_ref_err as above.  z ~ 2 N(0, 1),
                      float16-exact, with +-20 and 0 planted.
Asserted here: the fp64 formulas of tests/bsq_fsq_train_ref.py equal the reference's fp64 run (scalars to 1e-12 relative, gradients
to 1e-7 of their sum of |terms|), so a wrong checker cannot make a fixture; and the reference's fp32 FSQ indices differ from its fp64
ones only where the margin is below 1e-5, on fewer than 1 % of the positions.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from pit.quantization.bsq import BSQQuantizer as RefBSQ  # noqa: E402
from pit.quantization.fsq import FSQQuantizer as RefFSQ  # noqa: E402

import bsq_fsq_train_ref as R  # noqa: E402
from oracle import gq_oracle as O  # noqa: E402


def as_input(x, cl):
    xt = x.clone()
    if cl:
        xt = xt.contiguous(memory_format=torch.channels_last)
    return xt.requires_grad_(True)


def run_bsq(ref, x, w, cl):
    xt = as_input(x, cl)
    quantized, info = ref(xt)
    (quantized * w).sum().add(R.G_AUX * info["entropy_aux_loss"]).backward()
    return quantized.detach(), info, xt.grad


def bsq_x(cfg, g):
    x = cfg["scale"] * torch.randn(cfg["shape"], generator=g)
    if cfg["kind"] == "positive":
        x = x.abs() + 0.5
    x = x.half().float()
    if cfg["kind"] == "special":                        # "blc": row (0, 3) all zero, row (1, 5) holds +-50 and +-1e-4
        x[0, 3, :] = 0.0
        for k, v in enumerate((50.0, -50.0, 1e-4, -1e-4)):
            x[1, 5, 5 * k + 2] = float(np.float16(v))
    return x


def make_bsq_case(tag, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = bsq_x(cfg, g)
    w = torch.randn(cfg["shape"], generator=g).half().float()
    kw = dict(sample_minimization_weight=cfg.get("w_s", 1.0), batch_maximization_weight=cfg.get("w_b", 1.0))
    cl = bool(cfg.get("channels_last"))
    q32, i32, g32 = run_bsq(RefBSQ(cfg["format"], 1 << cfg["d"], 16, **kw).train(), x, w, cl)
    q64, i64, g64 = run_bsq(RefBSQ(cfg["format"], 1 << cfg["d"], 16, **kw).double().train(), x.double(), w.double(), cl)
    assert torch.equal(i32["indices"], i64["indices"])
    s = R.bsq64(x.numpy(), cfg, w.numpy(), R.G_AUX)
    assert np.array_equal(s["indices"], i64["indices"].numpy())
    out = {"x": x.numpy().astype(np.float16), "w": w.numpy().astype(np.float16), "g_aux": np.float64(R.G_AUX),
           "quantized": q32.numpy(), "indices": i32["indices"].numpy(), "grad_x": g32.numpy(), "grad_x64": g64.numpy(),
           "grad_x_abs": s["grad_x_abs"]}
    assert np.array_equal(out["x"].astype(np.float32), x.numpy()) and np.array_equal(out["w"].astype(np.float32), w.numpy())
    assert np.isfinite(out["grad_x"]).all() and np.isfinite(out["grad_x64"]).all()
    assert np.all(np.abs(s["grad_x"] - out["grad_x64"]) <= 1e-7 * s["grad_x_abs"])
    out["grad_x_ref_err"] = np.float64(R.err_units(out["grad_x"], out["grad_x64"], out["grad_x_abs"]))
    line = [f"grad_x {float(out['grad_x_ref_err']):.1f}"]
    for name in R.SCALARS:
        v32, v64 = float(i32[name].detach()), float(i64[name].detach())
        assert abs(s[name] - v64) <= 1e-12 * max(abs(v64), s[name + "_abs"]), (name, s[name], v64)
        out[name], out[name + "64"], out[name + "_abs"] = np.float32(v32), np.float64(v64), np.float64(s[name + "_abs"])
        out[name + "_ref_err"] = np.float64(R.err_units(v32, v64, s[name + "_abs"]))
        line.append(f"{name} {float(out[name + '_ref_err']):.1f}")
    print(f"bsq {tag}: positions {x.numel() // (16 * cfg['d'])} max|grad| {np.abs(out['grad_x64']).max():.3g} ref_err: " + ", ".join(line))
    return {f"{tag}_{k}": v for k, v in out.items()}


def make_bsq_underflow():
    cfg = R.BSQ_UNDERFLOW
    g = torch.Generator().manual_seed(2690)
    x = torch.randn(cfg["shape"], generator=g)
    x[0, 1, :] = 0.0
    x[0, 1, 0], x[0, 1, 5], x[0, 1, 9] = 1e18, 1e-30, -1e-30
    with torch.no_grad():
        q32, i32 = RefBSQ(cfg["format"], 1 << cfg["d"], 16).train()(x)
        _, i64 = RefBSQ(cfg["format"], 1 << cfg["d"], 16).double().train()(x.double())
    d32, d64 = int(i32["indices"][0, 1, 0]), int(i64["indices"][0, 1, 0])
    assert d32 == 1 << 15 and d64 == (1 << 15) | (1 << 10), (d32, d64)          # bit of channel 5: fp32 quotient 0, fp64 1e-48
    print(f"bsq underflow: fp32 index {d32:#x}, fp64 index {d64:#x}")
    return {"underflow_x": x.numpy(), "underflow_quantized": q32.numpy(), "underflow_indices": i32["indices"].numpy()}


def make_fsq_case(tag, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    z = (2.0 * torch.randn(cfg["shape"], generator=g)).half().float()
    flat = z.reshape(-1)
    for k, v in enumerate((20.0, -20.0, 0.0, 20.0, -20.0, 0.0)):
        flat[11 * k + 4] = v
    w = torch.randn(cfg["shape"], generator=g).half().float()
    cl = bool(cfg.get("channels_last"))
    fmt, levels = cfg["format"], cfg["levels"]
    zt = as_input(z, cl)
    zhat, info = RefFSQ(levels, fmt).train()(zt)
    (zhat * w).sum().backward()
    z64 = torch.from_numpy(R.to_pos(z.double().numpy(), fmt)[0].copy()).reshape(z.shape[0], -1, len(levels)).requires_grad_(True)
    w64 = torch.from_numpy(R.to_pos(w.double().numpy(), fmt)[0].copy()).reshape(z64.shape)
    zhat64, ind64 = RefFSQ(levels, fmt)._quantize(z64)
    (zhat64 * w64).sum().backward()
    packed64 = torch.zeros_like(ind64[:, :, 0:1])
    for l in range(len(levels)):
        packed64 = packed64 * levels[l] + ind64[:, :, l:l + 1]
    _, back = R.to_pos(z.numpy(), fmt)
    grad64 = back(z64.grad.numpy().reshape(-1, len(levels)))
    ind = info["indices"].numpy()
    ind64m = packed64.numpy().reshape(z.shape[0], -1, 1)
    ind64m = ind64m.transpose(0, 2, 1).reshape(ind.shape) if fmt == "bchw" else ind64m
    o_zhat, o_ind, margin = O.fsq_forward(z.numpy(), levels, fmt, with_margin=True)
    differ = ind != ind64m
    assert np.all(margin[differ] < 1e-5) and differ.mean() < 0.01, (tag, differ.sum())
    assert np.array_equal(o_ind, ind)
    s = R.fsq64(z.numpy(), levels, fmt, w.numpy())
    assert np.all(np.abs(s["grad_z"] - grad64) <= 1e-7 * s["grad_z_abs"])
    out = {"z": z.numpy().astype(np.float16), "w": w.numpy().astype(np.float16), "zhat": zhat.detach().numpy(), "indices": ind,
           "margin": margin.astype(np.float32), "grad_z": zt.grad.numpy(), "grad_z64": grad64, "grad_z_abs": s["grad_z_abs"]}
    assert np.array_equal(out["z"].astype(np.float32), z.numpy()) and np.array_equal(out["w"].astype(np.float32), w.numpy())
    out["grad_z_ref_err"] = np.float64(R.err_units(out["grad_z"], grad64, s["grad_z_abs"]))
    print(f"fsq {tag}: positions {ind.size}, fp32/fp64 indices differ at {int(differ.sum())}, min margin {margin.min():.3g}, "
          f"grad_z ref_err {float(out['grad_z_ref_err']):.2f}")
    return {f"{tag}_{k}": v for k, v in out.items()}


if __name__ == "__main__":
    out = {}
    for i, (tag, cfg) in enumerate(R.BSQ_CASES.items()):
        out.update(make_bsq_case(tag, cfg, 2600 + i))
    out.update(make_bsq_underflow())
    path = os.path.join(HERE, "g26_bsq_train_step.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))
    out = {}
    for i, (tag, cfg) in enumerate(R.FSQ_CASES.items()):
        out.update(make_fsq_case(tag, cfg, 2700 + i))
    path = os.path.join(HERE, "g27_fsq_train_step.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))
