"""fp64 restatement of one train-mode step of the Gaussian regularizers (reference pit/quantization/gaussian.py:77-119 GQ1,
:211-271 + :333-345 GQ2) and of its gradient -- the checker of tests/test_gpu_train_step.py, proven on the CPU by
tests/test_train_step_host.py and used by tests/golden/make_golden_train.py to fill g22_gq_train_step.npz.  numpy only.

The scalar loss that is differentiated:
    loss = sum(zhat * w_zhat) + sum(std * w_std) + g_kl * kl_loss
    zhat = mu + noise * sd,  sd = exp(lv / 2),  var = exp(lv),  lv = clamp(logvar, lv_min, lv_max)
    kl2[row] = sum_g C (mu^2 + var - 1 - lv),  C = float32(0.7213)  (1.4426 * 0.5 is formed in Python, then cast to the tensor's dtype)
    kl_loss  = sum_rows w(row) kl2[row] / divisor * float32(lam)
    w(row)   = float32(lam_max) if kl2 > float32(log2n + tol), float32(lam_min) if kl2 < float32(log2n - tol), else 1
with the lambdas as they are BEFORE the step's update (the weights are constants of the graph: comparisons have no gradient);
divisor = B for GQ1 (sum over [1, 2], then sum / B), = rows for GQ2 (a mean).  Its gradient:
    coef        = float32(g_kl) * float32(lam) * w(row) / divisor      (a Python scalar times an fp32 tensor is an fp32 product)
    grad_mu     = w_zhat + coef * 2 C mu
    grad_logvar = inside * (w_zhat noise sd / 2 + w_std sd / 2 + coef C var - coef C),  inside = lv_min <= logvar <= lv_max
Every function returns, next to a value, the SUM OF THE ABSOLUTE VALUES of the terms it was added up from: errors are stated in
units of 2^-24 of that sum (an fp32 evaluation of a sum of t terms, each a product of a few correctly rounded factors, is off by a
small multiple of it whatever the cancellation between the terms).  `coef C (var - 1)` counts as two terms, coef C var and coef C:
var itself is an fp32 number with a rounding error of 2^-24 var, which the difference does not shrink.
"""
import math

import numpy as np

C = float(np.float32(0.7213))
U = 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def to_rows(t, cfg):
    """A [mu- or zhat-shaped] array -> [rows, dim] with row = (b L + l) K + k, and the function that undoes it."""
    t = np.asarray(t)
    if cfg["kind"] == "gq1":
        g = cfg["group"]
        if cfg["format"] == "bchw":
            b, c, h, w = t.shape
            x = t.reshape(b, c, h * w).transpose(0, 2, 1)          # b l c
        else:
            b, _, c = t.shape
            x = t
        lead = x.shape
        K = c // g
        rows = x.reshape(lead[0], lead[1], g, K).transpose(0, 1, 3, 2).reshape(-1, g)      # channel g K + k -> (k, g)

        def back(r):
            y = r.reshape(lead[0], lead[1], K, g).transpose(0, 1, 3, 2).reshape(lead)
            return y.transpose(0, 2, 1).reshape(t.shape) if cfg["format"] == "bchw" else y
        return rows, back
    d, axis = cfg["dim"], cfg["dim_idx"]
    x = np.moveaxis(t, axis, -1)
    lead = x.shape
    rows = x.reshape(-1, d)                                        # channel k dim + g

    def back(r):
        return np.moveaxis(r.reshape(lead), -1, axis)
    return rows, back


def split(z, cfg):
    """z -> (mu, logvar) halves along the channel axis, each in the shape of zhat."""
    axis = (1 if cfg["format"] == "bchw" else 2) if cfg["kind"] == "gq1" else cfg["dim_idx"]
    return np.split(np.asarray(z), 2, axis=axis), axis


def step(z, noise, lams, cfg, w_zhat=None, g_kl=0.0, w_std=None):
    """One step in fp64 from fp32 inputs.  lams = (lam, lam_min, lam_max) before the step.  Returns a dict: zhat, std, kl2 [rows] and
    kl2_abs (sum of |terms| per row), cls [rows] (+1 above, -1 below, 0 inside), kl_loss, bits (mean, min, max), lams_after, grad
    (shape of z) and grad_abs (sum of |terms| per element), margin (min over rows of |kl2 - nearest threshold| / (2^-24 kl2_abs))."""
    (mu, lvr), axis = split(np.asarray(z, np.float64), cfg)
    noise = np.asarray(noise, np.float64)
    lo, hi = f32(cfg["lv_range"][0]), f32(cfg["lv_range"][1])
    inside = (lvr >= lo) & (lvr <= hi)
    lv = np.clip(lvr, lo, hi)
    sd, var = np.exp(0.5 * lv), np.exp(lv)
    zhat = mu + noise * sd
    el = C * (mu * mu + var - 1.0 - lv)
    el_abs = C * (mu * mu + var + 1.0 + np.abs(lv))
    r_el, back = to_rows(el, cfg)
    kl2 = r_el.sum(1)
    kl2_abs = to_rows(el_abs, cfg)[0].sum(1)
    n2 = int(math.log(cfg["n"], 2))
    thr_hi, thr_lo = f32(n2 + cfg["tol"]), f32(n2 - cfg["tol"])
    cls = np.where(kl2 > thr_hi, 1, np.where(kl2 < thr_lo, -1, 0))
    lam, lam_min, lam_max = (f32(v) for v in lams)
    wrow = np.where(cls > 0, lam_max, np.where(cls < 0, lam_min, 1.0))
    rows = kl2.shape[0]
    divisor = float(np.asarray(z).shape[0]) if cfg["kind"] == "gq1" else float(rows)
    kl_loss = (wrow * kl2).sum() / divisor * lam
    margin = (np.minimum(np.abs(kl2 - thr_hi), np.abs(kl2 - thr_lo)) / (U * kl2_abs)).min()
    # the lambda state machine in Python floats, exactly as the reference writes it (GQ2's lam_max decrease is a no-op expression)
    f = cfg["lam_factor"]
    l0, l1, l2 = (float(v) for v in lams)
    mean, mn, mx = f32(kl2.mean()), f32(kl2.min()), f32(kl2.max())
    l0 = l0 * f if mean > n2 else l0 / f
    if mx > n2 + cfg["tol"]:
        l2 = l2 * f
    elif cfg["kind"] == "gq1":
        l2 = l2 / f
    l2 = max(min(l2, cfg["lam_range"][1]), 1.0)
    l1 = l1 / f if mn < n2 - cfg["tol"] else l1 * f
    l1 = max(min(l1, 1.0), cfg["lam_range"][0])
    # gradient
    wz = np.zeros_like(mu) if w_zhat is None else np.asarray(w_zhat, np.float64)
    ws = np.zeros_like(mu) if w_std is None else np.asarray(w_std, np.float64)
    coef = back(np.repeat((f32(g_kl) * lam * wrow / divisor)[:, None], r_el.shape[1], 1))
    t_mu = [wz, coef * 2.0 * C * mu]
    t_lv = [wz * noise * 0.5 * sd, ws * 0.5 * sd, coef * C * var, -coef * C * np.ones_like(var)]
    g_mu, a_mu = sum(t_mu), sum(np.abs(t) for t in t_mu)
    g_lv, a_lv = inside * sum(t_lv), inside * sum(np.abs(t) for t in t_lv)
    return {"zhat": zhat, "std": sd, "kl2": kl2, "kl2_abs": kl2_abs, "cls": cls, "kl_loss": kl_loss,
            "bits": (kl2.mean(), kl2.min(), kl2.max()), "lams_after": (l0, l1, l2), "inside": inside,
            "grad": np.concatenate([g_mu, g_lv], axis), "grad_abs": np.concatenate([a_mu, a_lv], axis), "margin": margin}


def loss64(z, noise, lams, cfg, w_zhat, g_kl, w_std=None, cls=None):
    """The scalar loss above in fp64 (for central differences); `cls` freezes the rows' classes -- the weights are constants."""
    (mu, lvr), _ = split(np.asarray(z, np.float64), cfg)
    lo, hi = f32(cfg["lv_range"][0]), f32(cfg["lv_range"][1])
    lv = np.clip(lvr, lo, hi)
    sd, var = np.exp(0.5 * lv), np.exp(lv)
    zhat = mu + np.asarray(noise, np.float64) * sd
    kl2 = to_rows(C * (mu * mu + var - 1.0 - lv), cfg)[0].sum(1)
    lam, lam_min, lam_max = (f32(v) for v in lams)
    wrow = np.where(cls > 0, lam_max, np.where(cls < 0, lam_min, 1.0))
    divisor = float(np.asarray(z).shape[0]) if cfg["kind"] == "gq1" else float(kl2.shape[0])
    out = (zhat * np.asarray(w_zhat, np.float64)).sum() + f32(g_kl) * (wrow * kl2).sum() / divisor * lam
    if w_std is not None:
        out = out + (sd * np.asarray(w_std, np.float64)).sum()
    return out


def err_units(got, want, want_abs):
    """max |got - want| / (2^-24 sum |terms|) over the elements with a non-zero sum; elements without terms must be exact zeros."""
    got, want, want_abs = (np.asarray(a, np.float64) for a in (got, want, want_abs))
    live = want_abs > 0
    assert np.all(got[~live] == 0.0), "an element without terms is not exactly zero"
    return float((np.abs(got - want)[live] / (U * want_abs[live])).max()) if live.any() else 0.0


# the fixture's cases (tests/golden/make_golden_train.py); "z" shapes are the module's input shapes
CASES = {
    "gq1_bchw_g16": dict(kind="gq1", format="bchw", group=16, n=1024, shape=(2, 32, 8, 8), mu_scale=0.74, lv_mean=-0.9, lv_std=0.5),
    "gq1_blc_g8": dict(kind="gq1", format="blc", group=8, n=4096, shape=(2, 16, 32), mu_scale=1.1, lv_mean=-0.9, lv_std=0.5),
    "gq1_bchw_g4": dict(kind="gq1", format="bchw", group=4, n=64, shape=(2, 16, 4, 4), mu_scale=1.3, lv_mean=-0.9, lv_std=0.5),
    "gq2_d4_i1": dict(kind="gq2", dim=4, dim_idx=1, n=1024, shape=(2, 32, 4, 4), mu_scale=1.9, lv_mean=-1.5, lv_std=0.3),
    "gq2_d16_im1": dict(kind="gq2", dim=16, dim_idx=-1, n=4096, shape=(1, 32, 64), mu_scale=0.8, lv_mean=-1.5, lv_std=0.3),
    "gq1_clamp": dict(kind="gq1", format="bchw", group=8, n=256, shape=(2, 16, 4, 4), mu_scale=0.6, lv_mean=-2.0, lv_std=4.0,
                      lv_range=(-8.0, 4.0)),
}
for _c in CASES.values():
    _c.setdefault("lv_range", (-30.0, 20.0))
    _c.update(tol=0.5, lam_factor=1.01, lam_range=(1e-3, 1e3) if _c["kind"] == "gq1" else (1e-7, 1e7))
LAMS0 = (1.3, 0.7, 1.9)
STEPS = 2
