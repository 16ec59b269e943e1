"""CPU: the host half of the fused train-mode step of the Gaussian regularizers -- the two entry points exist and validate their
arguments before any HIP call, the fixture g22 loads, and the fp64 checker the GPU tests rely on (tests/train_step_ref.py) is proven
here: it reproduces the reference's autograd gradient within the reference's own fp32 error, and it agrees with a central
difference of the fp64 loss."""
import ctypes
import os

import numpy as np
import pytest
import torch

import train_step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INVALID = 1          # GQHIP_ERR_INVALID_ARG


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


def _fixture():
    return np.load(os.path.join(G, "g22_gq_train_step.npz"))


def test_train_step_symbols_are_exported_and_bound():
    L = _lib()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("gq_gauss_train_f32", "gq_gauss_backward_f32"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(dll, name) and hasattr(L.lib(), name)
    assert L.lib().gqhip_abi_version() == 8         # additive: the version does not move


def _train(L, z=64, noise=64, zhat=64, kl=64, sc=64, lam=64, B=2, Lp=4, c=16, dim=8, layout=0, grouping=0, div=2.0):
    return L.gq_gauss_train_f32(z, noise, zhat, None, kl, sc, lam, B, Lp, c, dim, layout, grouping, -30.0, 20.0, 10.0, 0.5, 1.01,
                                1e-3, 1e3, 1, div, None)


def _back(L, z=64, noise=64, gk=None, lam=64, gz=64, B=2, Lp=4, c=16, dim=8, layout=0, grouping=0, div=2.0):
    return L.gq_gauss_backward_f32(z, noise, None, None, gk, lam, gz, B, Lp, c, dim, layout, grouping, -30.0, 20.0, 10.0, 0.5, div,
                                   None)


def test_train_step_entry_points_validate_before_any_hip_call():
    """Pointers here are small fake addresses: every call must be rejected (or, with rows == 0, accepted) on its arguments alone."""
    L = _lib().lib()
    for kw in (dict(z=None), dict(noise=None), dict(zhat=None), dict(kl=None), dict(sc=None), dict(lam=None),
               dict(sc=68), dict(lam=68),                     # 8-byte alignment of scalars_out / lam_state
               dict(c=16, dim=5), dict(dim=0), dict(dim=65, c=65), dict(layout=2), dict(grouping=-1), dict(Lp=0), dict(B=-1),
               dict(div=0.0), dict(div=float("nan"))):
        assert _train(L, **kw) == INVALID, kw
    for kw in (dict(z=None), dict(noise=None), dict(lam=None), dict(gz=None), dict(lam=68), dict(gk=66),
               dict(c=16, dim=5), dict(dim=0), dict(layout=7), dict(grouping=2), dict(Lp=0), dict(B=-1), dict(div=-1.0)):
        assert _back(L, **kw) == INVALID, kw


def test_train_step_with_no_rows_is_ok_and_launches_nothing():
    L = _lib().lib()
    assert _train(L, B=0) == 0 and _back(L, B=0) == 0
    assert _train(L, B=0, div=0.0) == 0             # GQ1's divisor IS B


def test_fixture_loads_and_is_complete():
    d = _fixture()
    for tag, cfg in R.CASES.items():
        for it in range(R.STEPS):
            p = f"{tag}_{it}_"
            keys = ["z", "noise", "w", "g_kl", "lams_before", "lams_after", "zhat", "scalars", "grad_z", "grad64", "grad_abs", "ref_err"]
            for k in keys + (["w_std"] if cfg["kind"] == "gq2" else []):
                assert p + k in d.files, p + k
            assert d[p + "z"].shape == cfg["shape"] and d[p + "grad_z"].shape == cfg["shape"] and d[p + "z"].dtype == np.float32
            assert d[p + "noise"].shape == d[p + "zhat"].shape == d[p + "w"].shape
        assert tuple(d[f"{tag}_0_lams_before"]) == R.LAMS0
        assert tuple(d[f"{tag}_1_lams_before"]) == tuple(d[f"{tag}_0_lams_after"])       # two CONSECUTIVE steps
    assert d["gq1_clamp_0_clamped"] > 0
    assert os.path.getsize(os.path.join(G, "g22_gq_train_step.npz")) < (1 << 20)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_formula_helper_reproduces_the_fixture(tag):
    """The fp64 helper, run on the fixture's inputs, gives the fixture's fp64 gradient (it made it) and lies within ref_err of the
    reference's fp32 autograd gradient; statistics, lambdas and zhat are the reference's; no row is near a threshold; some case has
    all three classes."""
    d, cfg = _fixture(), R.CASES[tag]
    for it in range(R.STEPS):
        p = f"{tag}_{it}_"
        s = R.step(d[p + "z"], d[p + "noise"], tuple(d[p + "lams_before"]), cfg, d[p + "w"], float(d[p + "g_kl"]),
                   d[p + "w_std"] if cfg["kind"] == "gq2" else None)
        assert np.allclose(s["grad"], d[p + "grad64"], rtol=1e-12, atol=1e-300)
        err = R.err_units(d[p + "grad_z"], s["grad"], s["grad_abs"])
        assert err <= float(d[p + "ref_err"]) * (1 + 1e-9), (it, err)
        assert s["lams_after"] == tuple(d[p + "lams_after"])
        assert s["margin"] >= 16.0
        for got, want in zip((s["kl_loss"],) + s["bits"], d[p + "scalars"]):
            assert abs(got - want) <= 2e-5 * max(1.0, abs(want))
        lv = np.split(d[p + "z"], 2, axis=R.split(d[p + "z"], cfg)[1])[1]
        glv = np.split(d[p + "grad_z"], 2, axis=R.split(d[p + "z"], cfg)[1])[1]
        out = (lv < cfg["lv_range"][0]) | (lv > cfg["lv_range"][1])
        assert int(out.sum()) == int(d[p + "clamped"]) and np.all(glv[out] == 0.0)
    if tag == "gq1_clamp":
        lv = np.split(d[f"{tag}_0_z"], 2, axis=1)[1]
        assert (lv < -8.0).any() and (lv > 4.0).any()           # clamps on both sides


def test_some_fixture_case_has_all_three_row_classes():
    d, best = _fixture(), 0.0
    for tag, cfg in R.CASES.items():
        s = R.step(d[f"{tag}_0_z"], d[f"{tag}_0_noise"], R.LAMS0, cfg)
        best = max(best, min(float((s["cls"] == c).mean()) for c in (1, 0, -1)))
    assert best >= 0.02


@pytest.mark.parametrize("tag", ["gq1_bchw_g4", "gq2_d4_i1", "gq1_clamp"])
def test_formula_helper_against_a_central_difference(tag):
    """64 random elements of a small z, step 1e-6 in fp64: agreement within 1e-5 of the sum of |terms| -- coarse on purpose (the
    difference quotient is good to ~1e-9; a wrong formula is off by order 1).  Classes are frozen: the weights are constants."""
    d, cfg = _fixture(), R.CASES[tag]
    p = f"{tag}_0_"
    z = d[p + "z"].astype(np.float64)
    lams, w, gk = tuple(d[p + "lams_before"]), d[p + "w"], float(d[p + "g_kl"])
    ws = d[p + "w_std"] if cfg["kind"] == "gq2" else None
    s = R.step(z, d[p + "noise"], lams, cfg, w, gk, ws)
    rng = np.random.default_rng(7)
    h, checked = 1e-6, 0
    lo, hi = cfg["lv_range"]
    for flat in rng.choice(z.size, 64, replace=False):
        i = np.unravel_index(flat, z.shape)
        if min(abs(z[i] - lo), abs(z[i] - hi)) < 1e-3:       # (the clamp's kink: no derivative there)
            continue
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        num = (R.loss64(zp, d[p + "noise"], lams, cfg, w, gk, ws, s["cls"]) - R.loss64(zm, d[p + "noise"], lams, cfg, w, gk, ws, s["cls"])) / (2 * h)
        scale = max(s["grad_abs"][i], 1e-3)
        assert abs(num - s["grad"][i]) <= 1e-5 * scale + 1e-7 * abs(num), (i, num, s["grad"][i])
        checked += 1
    assert checked >= 60


def test_cpu_tensor_in_train_mode_still_takes_the_torch_branch():
    """No device, no library call: a CPU z through train() runs the op-by-op branch (bit identity with the reference's CPU golden is
    test_host.py's), its outputs carry the torch graph, and the host copy of the lambdas moves."""
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    m = GaussianQuantRegularizer("bchw", 1024, group=16).train()
    z = torch.from_numpy(_fixture()["gq1_bchw_g16_0_z"]).requires_grad_(True)
    zhat, info = m(z)
    assert set(info) == {"kl_loss", "bits-mean", "bits-min", "bits-max", "lam"}
    assert zhat.grad_fn is not None and "GaussTrainFn" not in type(zhat.grad_fn).__name__
    assert m._lam_dev is None and m.lam != 1.0
    (zhat.sum() + info["kl_loss"]).backward()
    assert z.grad is not None and torch.isfinite(z.grad).all()
