"""Train-step fixture (same rules as make_golden*.py: build container only, imports /root/reference, stores DATA).

  g22_gq_train_step.npz   two consecutive train() steps of the reference's GaussianQuantRegularizer / GaussianQuantRegularizer2 on
                      the CPU (backend "torch") under autograd, for the cases of tests/train_step_ref.py:CASES -- GQ1 bchw group 16
                      n 1024, GQ1 blc group 8 n 4096, GQ1 bchw group 4, GQ2 dim 4 dim_idx 1, GQ2 dim 16 dim_idx -1, and one with
                      logvar_range [-8, 4] whose logvar clamps on both sides -- from the lambda state (1.3, 0.7, 1.9), so that the
                      three row weights differ.  While the reference runs, torch.randn_like is replaced by a function that records
                      what it returns: the fixture holds the noise (in the layout of zhat).
                      loss = sum(zhat * w) [+ sum(info["std"] * w_std) for GQ2] + g_kl * info["kl_loss"]; backward().
                      Per step: z, noise, w, (w_std,) g_kl, lams_before; zhat, scalars (kl_loss, bits-mean / -min / -max), lams_after,
                      grad_z (the reference's fp32 autograd); grad64 / grad_abs (the fp64 formulas of tests/train_step_ref.py and
                      the sum of |terms|), ref_err = max |grad_z - grad64| / (2^-24 grad_abs): the reference's own fp32 error.
Asserted here: at least one case has every class (above / inside / below the thresholds) at >= 2 % of its rows; no row of any case
has its fp64 kl2 within 16 * 2^-24 * (sum of |terms of the row|) of a threshold (else the next seed is tried), so a GPU test can
compare every element without an exclusion list; the helper's lambdas are the reference's Python floats; the reference's clamped
elements have zero logvar gradient.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pit.quantization.gaussian import GaussianQuantRegularizer as RefGQ1  # noqa: E402
from pit.quantization.gaussian import GaussianQuantRegularizer2 as RefGQ2  # noqa: E402

import train_step_ref as R  # noqa: E402


def make_z(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    shape = list(cfg["shape"])
    axis = (1 if cfg["format"] == "bchw" else 2) if cfg["kind"] == "gq1" else cfg["dim_idx"] % len(shape)
    shape[axis] //= 2
    scale = cfg["mu_scale"] * (0.9 + 0.1 * torch.rand(shape, generator=g))
    mu = scale * torch.randn(shape, generator=g)
    lv = cfg["lv_mean"] + cfg["lv_std"] * torch.randn(shape, generator=g)
    w = torch.randn(shape, generator=g)
    w_std = torch.randn(shape, generator=g)
    return torch.cat([mu, lv], axis), w, w_std


def noise_in_zhat_layout(rec, cfg, zhat_shape):
    """What randn_like returned inside the reference ([b, l, c] for GQ1, [-1, c] for GQ2) -> the layout of zhat."""
    if cfg["kind"] == "gq1":
        if cfg["format"] == "bchw":
            b, c, h, w = zhat_shape
            return rec.reshape(b, h * w, c).permute(0, 2, 1).reshape(zhat_shape).contiguous()
        return rec.reshape(zhat_shape).contiguous()
    axis = cfg["dim_idx"] % len(zhat_shape)
    lead = list(zhat_shape)
    lead.append(lead.pop(axis))
    return torch.movedim(rec.reshape(lead), -1, axis).contiguous()


def run_case(tag, cfg, seed):
    if cfg["kind"] == "gq1":
        ref = RefGQ1(cfg["format"], cfg["n"], group=cfg["group"], logvar_range=list(cfg["lv_range"]), backend="torch")
    else:
        ref = RefGQ2(cfg["dim"], cfg["n"], dim_idx=cfg["dim_idx"], logvar_range=list(cfg["lv_range"]), backend="torch")
    ref.train()
    ref.lam, ref.lam_min, ref.lam_max = R.LAMS0
    out, fracs = {}, []
    for it in range(R.STEPS):
        z, w, w_std = make_z(cfg, seed + 1000 * it)
        g_kl = (0.37, 1.3)[it]
        lams_before = (ref.lam, ref.lam_min, ref.lam_max)
        zt = z.clone().requires_grad_(True)
        recorded = []
        orig = torch.randn_like

        def recording_randn_like(t, *a, **k):
            r = orig(t, *a, **k)
            recorded.append(r.detach().clone())
            return r

        torch.manual_seed(seed + it)
        torch.randn_like = recording_randn_like
        try:
            zhat, info = ref(zt)
        finally:
            torch.randn_like = orig
        assert len(recorded) == 1
        loss = (zhat * w).sum() + g_kl * info["kl_loss"]
        if cfg["kind"] == "gq2":
            loss = loss + (info["std"] * w_std).sum()
        loss.backward()
        noise = noise_in_zhat_layout(recorded[0], cfg, tuple(w.shape))
        s = R.step(z.numpy(), noise.numpy(), lams_before, cfg, w.numpy(), g_kl, w_std.numpy() if cfg["kind"] == "gq2" else None)
        if s["margin"] < 16.0:
            return None, None
        lams_after = (ref.lam, ref.lam_min, ref.lam_max)
        assert s["lams_after"] == lams_after, (tag, it, s["lams_after"], lams_after)
        zh_ref = zhat.detach().numpy() if cfg["kind"] == "gq1" else info["zhat_noquant"].detach().numpy()
        assert np.abs(zh_ref - s["zhat"]).max() <= 4 * R.U * np.abs(s["zhat"]).max() + 1e-6
        scal = [float(info[k]) for k in ("kl_loss", "bits-mean", "bits-min", "bits-max")]
        for got, want in zip(scal, (s["kl_loss"],) + tuple(s["bits"])):
            assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (tag, it, got, want)
        gz = zt.grad.numpy()
        ref_err = R.err_units(gz, s["grad"], s["grad_abs"])          # (asserts exact zeros on clamped elements)
        n_clamped = int((~s["inside"]).sum())
        fr = [float((s["cls"] == c).mean()) for c in (1, 0, -1)]
        fracs.append(fr)
        print(f"{tag} step {it}: rows {s['cls'].size} above/inside/below {fr[0]:.2f}/{fr[1]:.2f}/{fr[2]:.2f} margin {s['margin']:.0f} "
              f"clamped {n_clamped} ref_err {ref_err:.2f} lams {lams_after}")
        p = f"{tag}_{it}_"
        out[p + "z"], out[p + "noise"], out[p + "w"] = z.numpy(), noise.numpy(), w.numpy()
        if cfg["kind"] == "gq2":
            out[p + "w_std"] = w_std.numpy()
        out[p + "g_kl"] = np.float64(g_kl)
        out[p + "lams_before"], out[p + "lams_after"] = np.array(lams_before, np.float64), np.array(lams_after, np.float64)
        out[p + "zhat"] = zhat.detach().numpy()
        out[p + "scalars"] = np.array(scal, np.float64)
        out[p + "grad_z"] = gz
        out[p + "grad64"], out[p + "grad_abs"] = s["grad"], s["grad_abs"].astype(np.float32)
        out[p + "ref_err"] = np.float64(ref_err)
        out[p + "clamped"] = np.int64(n_clamped)
    return out, fracs


if __name__ == "__main__":
    out, three = {}, False
    for i, (tag, cfg) in enumerate(R.CASES.items()):
        for seed in range(220 + 10 * i, 220 + 10 * i + 10):
            got, fracs = run_case(tag, cfg, seed)
            if got is not None:
                break
            print(f"{tag}: seed {seed} has a row within 16 units of a threshold, next seed")
        assert got is not None, tag
        out.update(got)
        out[f"{tag}_seed"] = np.int64(seed)
        three = three or any(min(fr) >= 0.02 for fr in fracs)
    assert three, "no case has all three classes at >= 2 % of its rows"
    assert out["gq1_clamp_0_clamped"] > 0
    path = os.path.join(HERE, "g22_gq_train_step.npz")
    np.savez_compressed(path, **out)
    print("max ref_err", max(float(v) for k, v in out.items() if k.endswith("ref_err")), "bytes", os.path.getsize(path))
