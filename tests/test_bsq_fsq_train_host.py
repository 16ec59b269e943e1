"""CPU: the host half of the fused BSQ / FSQ train steps -- the new entry points exist, are bound and validate their arguments
before any HIP call, the opt-in switch is off by default, the fixtures g26 / g27 load, the fp64 checker the GPU tests rely on
(tests/bsq_fsq_train_ref.py) agrees with a central difference, and a CPU BSQQuantizer / FSQQuantizer step (the torch branch, which
CPU tensors keep) lands on the fixtures, g29 (the "blc" kernel pairs g26 leaves out) among them."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import bsq_fsq_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INVALID, WORKSPACE = 1, 2          # GQHIP_ERR_INVALID_ARG, GQHIP_ERR_WORKSPACE
NAMES = ("bsq_train_workspace_bytes", "bsq_train_f32", "bsq_backward_f32", "fsq_train_f32", "fsq_backward_f32")


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


def _bsq():
    return np.load(os.path.join(G, "g26_bsq_train_step.npz"))


def _fsq():
    return np.load(os.path.join(G, "g27_fsq_train_step.npz"))


def _inputs(d, tag, key="x"):
    return d[f"{tag}_{key}"].astype(np.float32), d[f"{tag}_w"].astype(np.float32)


# ---- these fail on the parent commit -----------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_in_the_header():
    L = _lib()
    dll = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gqhip.h")).read()
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS and hasattr(dll, name) and hasattr(L.lib(), name)
        assert name + "(" in header
    assert "bsq.py:14-37, 64-133" in header and "fsq.py:6-9, 29-68" in header          # the map of reference line ranges
    assert L.lib().gqhip_abi_version() == L.ABI_VERSION == 8                            # additive: the version does not move
    assert "#define GQHIP_ABI_VERSION 8" in " ".join(header.split())


def test_wrappers_exist_and_have_no_cpu_fallback():
    L = _lib()
    assert list(inspect.signature(L.bsq_train).parameters) == ["x", "dim", "layout", "w_s", "w_b", "ws"]
    assert list(inspect.signature(L.bsq_backward).parameters) == ["x", "avg", "dim", "layout", "w_s", "w_b", "g_q", "g_aux", "ws"]
    assert list(inspect.signature(L.fsq_train).parameters) == ["z", "levels", "layout"]
    assert list(inspect.signature(L.fsq_backward).parameters) == ["z", "g_zhat", "levels", "layout"]
    assert issubclass(L.BsqTrainWorkspace, L._Scratch) and callable(L.BsqTrainWorkspace().get)
    with pytest.raises(L.GqHipError):
        L.bsq_train(torch.zeros(1, 16, 2, 2), 1, "bchw")
    with pytest.raises(L.GqHipError):
        L.bsq_backward(torch.zeros(1, 16, 2, 2), torch.zeros(1, 2), 1, "bchw")
    with pytest.raises(L.GqHipError):
        L.fsq_train(torch.zeros(1, 3, 2, 2), [5, 5, 5], "bchw")
    with pytest.raises(L.GqHipError):
        L.fsq_backward(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2), [5, 5, 5], "bchw")


def test_bsq_workspace_query():
    q = _lib().lib().bsq_train_workspace_bytes
    assert q(0, 1) > 0
    for d in (1, 4, 16):
        sizes = [q(r, d) for r in (1, 15, 16, 17, 255, 4099, 16384, 1 << 20)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert q(1 << 20, 16) <= 1 << 20                                                 # per-block partials only, never per row
    for d in range(1, 17):
        assert q(1000, d) > 0
    for bad in ((10, 0), (10, 17), (-1, 8), (1 << 30, 8)):
        assert q(*bad) == -1, bad


def _btrain(L, x=64, qz=64, idx=64, avg=64, sc=64, B=2, Lp=4, C=32, d=2, layout=0, ws=64, wsb=1 << 30):
    return L.bsq_train_f32(x, qz, idx, avg, sc, B, Lp, C, d, layout, 1.0, 1.0, ws, wsb, None)


def _bback(L, x=64, avg=64, gq=None, ga=None, gx=64, B=2, Lp=4, C=32, d=2, layout=0, ws=64, wsb=1 << 30):
    return L.bsq_backward_f32(x, avg, gq, ga, gx, B, Lp, C, d, layout, 1.0, 1.0, ws, wsb, None)


BSQ_BAD_SHAPES = (dict(C=33), dict(C=16), dict(d=0, C=0), dict(d=17, C=272), dict(layout=2), dict(layout=-1), dict(B=-1), dict(Lp=-1))


def test_bsq_calls_validate_before_any_hip_call():
    """Pointers here are small fake addresses: every call must be rejected on its arguments alone."""
    L = _lib().lib()
    need = L.bsq_train_workspace_bytes(2 * 4, 2)
    for kw in (dict(x=None), dict(qz=None), dict(idx=None), dict(avg=None), dict(sc=None), dict(avg=66), dict(sc=66), dict(idx=68),
               dict(x=66), dict(qz=66), dict(x=72, layout=1), dict(qz=72, layout=1)) + BSQ_BAD_SHAPES:
        assert _btrain(L, **kw) == INVALID, kw
    for kw in (dict(x=None), dict(avg=None), dict(gx=None), dict(ga=66), dict(avg=66), dict(gq=66), dict(gx=72, layout=1),
               dict(gq=72, layout=1)) + BSQ_BAD_SHAPES:
        assert _bback(L, **kw) == INVALID, kw
    for call in (_btrain, _bback):
        for layout in (0, 1):
            assert call(L, ws=None, layout=layout) == WORKSPACE
            assert call(L, ws=72, layout=layout) == WORKSPACE                      # not 16-byte aligned
            assert call(L, wsb=need - 1, layout=layout) == WORKSPACE
            assert call(L, B=0, ws=None, wsb=0, layout=layout) == 0 and call(L, Lp=0, ws=None, wsb=0, layout=layout) == 0


def _levels(v):
    return (ctypes.c_int32 * len(v))(*v), len(v)


def test_fsq_calls_validate_before_any_hip_call():
    L = _lib().lib()
    lev, n = _levels([8, 5, 5])

    def train(z=64, zhat=64, idx=64, levels=lev, nlev=n, B=2, Lp=4, layout=0):
        return L.fsq_train_f32(z, levels, nlev, zhat, idx, B, Lp, layout, None)

    def back(z=64, g=64, gz=64, levels=lev, nlev=n, B=2, Lp=4, layout=0):
        return L.fsq_backward_f32(z, g, levels, nlev, gz, B, Lp, layout, None)

    many, _ = _levels([2] * 17)
    zero, _ = _levels([8, 0, 5])
    huge, _ = _levels([1000] * 4)                                                     # the packed index is an int32
    shapes = (dict(levels=None), dict(nlev=0), dict(nlev=17, levels=many), dict(levels=zero), dict(levels=huge, nlev=4),
              dict(layout=2), dict(layout=-1), dict(B=-1), dict(Lp=-1))
    for kw in (dict(z=None), dict(zhat=None), dict(idx=None), dict(z=66), dict(zhat=66), dict(idx=66)) + shapes:
        assert train(**kw) == INVALID, kw
    for kw in (dict(z=None), dict(g=None), dict(gz=None), dict(z=66), dict(g=66), dict(gz=66)) + shapes:
        assert back(**kw) == INVALID, kw
    for call in (train, back):
        assert call(B=0) == 0 and call(Lp=0) == 0                                     # empty input


def test_opt_in_is_off_by_default_and_under_the_main_switch(monkeypatch):
    from pit_hip.quantization import _fused

    for var in ("GQHIP_TRAIN_FUSED", "GQHIP_BSQ_TRAIN_FUSED", "GQHIP_FSQ_TRAIN_FUSED"):
        monkeypatch.delenv(var, raising=False)
    assert not _fused.train_fused_opt_in("bsq") and not _fused.train_fused_opt_in("fsq")
    monkeypatch.setenv("GQHIP_BSQ_TRAIN_FUSED", "1")                                  # read per call
    assert _fused.train_fused_opt_in("bsq") and not _fused.train_fused_opt_in("fsq")
    monkeypatch.setenv("GQHIP_FSQ_TRAIN_FUSED", "1")
    assert _fused.train_fused_opt_in("bsq") and _fused.train_fused_opt_in("fsq")
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "0")
    assert not _fused.train_fused_opt_in("bsq") and not _fused.train_fused_opt_in("fsq")
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "1")
    monkeypatch.setenv("GQHIP_BSQ_TRAIN_FUSED", "0")
    assert not _fused.train_fused_opt_in("bsq") and _fused.train_fused_opt_in("fsq")


# ---- these pass on the parent commit: they prove the checker -----------------------------------------------------------------------
def test_fixtures_load_and_are_complete():
    d = _bsq()
    for tag, cfg in R.BSQ_CASES.items():
        x, w = _inputs(d, tag)
        assert x.shape == cfg["shape"] == w.shape == d[f"{tag}_grad_x"].shape == d[f"{tag}_grad_x64"].shape == d[f"{tag}_quantized"].shape
        assert d[f"{tag}_x"].dtype == np.float16 and d[f"{tag}_indices"].dtype == np.int64 and np.isfinite(x).all()
        assert d[f"{tag}_indices"].size * 16 == x.size
        for name in R.SCALARS + ("grad_x",):
            assert float(d[f"{tag}_{name}_ref_err"]) >= 0.0
    x = _inputs(d, "blc_d3_special")[0]
    assert (x[0, 3] == 0).all() and (np.abs(x[1, 5]) == 50).sum() == 2 and ((np.abs(x[1, 5]) > 0) & (np.abs(x[1, 5]) < 2e-4)).sum() == 2
    assert np.isfinite(d["blc_d3_special_grad_x64"]).all() and np.abs(d["blc_d3_special_grad_x64"][0, 3]).max() > 1e9
    assert (_inputs(d, "bchw_d1_saturated")[0] >= 0.5).all()
    xu = d["underflow_x"]
    assert xu.dtype == np.float32 and xu.shape == R.BSQ_UNDERFLOW["shape"] and d["underflow_indices"][0, 1, 0] == 1 << 15
    assert sorted(xu[0, 1][xu[0, 1] != 0].tolist()) == sorted(np.float32([1e18, 1e-30, -1e-30]).tolist())
    f = _fsq()
    for tag, cfg in R.FSQ_CASES.items():
        z, w = _inputs(f, tag, "z")
        assert z.shape == cfg["shape"] == w.shape == f[f"{tag}_zhat"].shape == f[f"{tag}_grad_z"].shape == f[f"{tag}_grad_z64"].shape
        assert f[f"{tag}_indices"].dtype == np.int32 and f[f"{tag}_margin"].shape == f[f"{tag}_indices"].shape
        assert (z == 20).sum() >= 2 and (z == -20).sum() >= 2 and (z == 0).sum() >= 2
        assert float(f[f"{tag}_grad_z_ref_err"]) >= 0.0
    for name in ("g26_bsq_train_step.npz", "g27_fsq_train_step.npz"):
        assert os.path.getsize(os.path.join(G, name)) < (400 << 10)


@pytest.mark.parametrize("tag", list(R.BSQ_CASES))
def test_bsq_checker_reproduces_the_fixture(tag):
    """The checker equals the reference's fp64 run (scalars to 1e-12, grad_x to 1e-7 of its sum of |terms|) and lies within ref_err
    of its fp32 run."""
    d, cfg = _bsq(), R.BSQ_CASES[tag]
    x, w = _inputs(d, tag)
    s = R.bsq64(x, cfg, w, float(d[f"{tag}_g_aux"]))
    for name in R.SCALARS:
        v64 = float(d[f"{tag}_{name}64"])
        assert abs(s[name] - v64) <= 1e-12 * max(abs(v64), s[name + "_abs"])
        assert abs(s[name + "_abs"] - float(d[f"{tag}_{name}_abs"])) <= 1e-12 * s[name + "_abs"]
        assert R.err_units(d[f"{tag}_{name}"], s[name], s[name + "_abs"]) <= float(d[f"{tag}_{name}_ref_err"]) * (1 + 1e-6) + 1e-6
    assert np.all(np.abs(s["grad_x"] - d[f"{tag}_grad_x64"]) <= 1e-7 * s["grad_x_abs"])
    assert np.allclose(s["grad_x_abs"], d[f"{tag}_grad_x_abs"], rtol=1e-12)
    assert R.err_units(d[f"{tag}_grad_x"], s["grad_x"], s["grad_x_abs"]) <= float(d[f"{tag}_grad_x_ref_err"]) * (1 + 1e-3) + 1e-3
    assert np.array_equal(s["indices"], d[f"{tag}_indices"])
    qs = np.float32(1.0 / np.sqrt(16 * cfg["d"]))
    assert np.all(np.abs(np.abs(d[f"{tag}_quantized"]) - qs) <= 3 * R.U * qs)          # two roundings in u + (q - u), one for the scale


def test_bsq_checker_against_a_central_difference():
    """40 random elements, step 1e-6 in fp64 (the signs do not move: the detached branch is a constant): agreement within 1e-5 of the
    sum of |terms| -- coarse on purpose (a wrong formula is off by order 1)."""
    tag = "blc_d2_small"
    d, cfg = _bsq(), R.BSQ_CASES[tag]
    x, w = (a.astype(np.float64) for a in _inputs(d, tag))
    ga = float(d[f"{tag}_g_aux"])
    s = R.bsq64(x, cfg, w, ga)
    rng = np.random.default_rng(11)
    h = 1e-6
    for flat in rng.choice(x.size, 40, replace=False):
        i = np.unravel_index(flat, x.shape)
        xp, xm = x.copy(), x.copy()
        xp[i] += h * 0.02
        xm[i] -= h * 0.02
        num = (R.bsq_loss64(xp, cfg, w, ga) - R.bsq_loss64(xm, cfg, w, ga)) / (2 * h * 0.02)
        assert abs(num - s["grad_x"][i]) <= 1e-5 * max(s["grad_x_abs"][i], 1e-3), (i, num, s["grad_x"][i])


@pytest.mark.parametrize("tag", list(R.FSQ_CASES))
def test_fsq_checker_reproduces_the_fixture_and_a_central_difference(tag):
    f, cfg = _fsq(), R.FSQ_CASES[tag]
    z, w = _inputs(f, tag, "z")
    s = R.fsq64(z, cfg["levels"], cfg["format"], w)
    assert np.all(np.abs(s["grad_z"] - f[f"{tag}_grad_z64"]) <= 1e-7 * s["grad_z_abs"])
    assert np.allclose(s["grad_z_abs"], f[f"{tag}_grad_z_abs"], rtol=1e-12)
    assert R.err_units(f[f"{tag}_grad_z"], s["grad_z"], s["grad_z_abs"]) <= float(f[f"{tag}_grad_z_ref_err"]) * (1 + 1e-3) + 1e-3
    n = len(cfg["levels"])
    hw = R.to_pos(z, cfg["format"])[1](np.tile(s["half_width"], (z.size // n, 1)))               # half_width of every element
    assert np.all(np.abs(f[f"{tag}_zhat"] - s["zhat"]) <= 2.0 ** -23 * (np.abs(s["r"]) + 1) / hw)
    rng = np.random.default_rng(12)
    z64, h = z.astype(np.float64), 1e-6
    for flat in rng.choice(z.size, 20, replace=False):
        i = np.unravel_index(flat, z.shape)
        zp, zm = z64.copy(), z64.copy()
        zp[i] += h
        zm[i] -= h
        num = (R.fsq_loss64(zp, cfg["levels"], cfg["format"], w) - R.fsq_loss64(zm, cfg["levels"], cfg["format"], w)) / (2 * h)
        assert abs(num - s["grad_z"][i]) <= 1e-5 * max(s["grad_z_abs"][i], 1e-3), (i, num, s["grad_z"][i])


def _as_input(a, cfg):
    t = torch.from_numpy(a)
    if cfg.get("channels_last"):
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(True)


def _cpu_bsq_step(cfg, x, w, g_aux, monkeypatch):
    """One train step of the CPU module under autograd: (quantized, info, x.grad)."""
    from pit_hip import _lib as L
    from pit_hip.quantization.bsq import BSQQuantizer

    def cpu_pack(x):
        bits = x > 0
        idx = torch.zeros(x.shape[0], dtype=torch.int64)
        for i in range(x.shape[1]):
            idx = idx * 2 + bits[:, i]
        return idx, torch.where(bits, 1.0, -1.0)

    monkeypatch.setattr(L, "lfq_pack", cpu_pack)
    monkeypatch.setenv("GQHIP_BSQ_TRAIN_FUSED", "1")                                 # a CPU tensor does not take the fused route
    m = BSQQuantizer(cfg["format"], 1 << cfg["d"], 16, sample_minimization_weight=cfg.get("w_s", 1.0),
                     batch_maximization_weight=cfg.get("w_b", 1.0)).train()
    xt = _as_input(x, cfg)
    quantized, info = m(xt)
    assert set(info) == {"indices", "entropy_aux_loss", "per_sample_entropy", "codebook_entropy"}
    assert "BSQTrainFn" not in type(info["entropy_aux_loss"].grad_fn).__name__
    ((quantized * torch.from_numpy(w)).sum() + g_aux * info["entropy_aux_loss"]).backward()
    return quantized.detach().numpy(), info, xt.grad.numpy()


@pytest.mark.parametrize("tag", list(R.BSQ_CASES))
def test_cpu_bsq_train_step_lands_on_the_fixture(tag, monkeypatch):
    """A CPU tensor keeps the torch branch.  That branch asks the library for the sign pack, which has no CPU implementation: numpy
    answers in its place, so what is checked is the differentiable glue -- the indices bit for bit, quantized within its three
    roundings, the scalars and grad_x within twice the reference's own fp32 error."""
    d, cfg = _bsq(), R.BSQ_CASES[tag]
    x, w = _inputs(d, tag)
    quantized, info, grad = _cpu_bsq_step(cfg, x, w, float(d[f"{tag}_g_aux"]), monkeypatch)
    assert np.array_equal(info["indices"].numpy(), d[f"{tag}_indices"])
    qs = 1.0 / np.sqrt(16 * cfg["d"])
    assert np.all(np.abs(quantized - d[f"{tag}_quantized"]) <= 6 * R.U * qs)
    for name in R.SCALARS:
        got = R.err_units(float(info[name].detach()), float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        assert got <= 2.0 * float(d[f"{tag}_{name}_ref_err"]) + 2.0, (name, got)
    got = R.err_units(grad, d[f"{tag}_grad_x64"], d[f"{tag}_grad_x_abs"])
    assert got <= 2.0 * float(d[f"{tag}_grad_x_ref_err"]) + 2.0, got


# ---- g29: the "blc" kernel pairs the cases above never launch (R.BSQ_VARIANT_CASES) ------------------------------------------------
G29 = os.path.join(G, "g29_bsq_train_variants.npz")


def test_bsq_variant_fixture_loads_and_is_complete():
    d = np.load(G29)
    for tag, cfg in R.BSQ_VARIANT_CASES.items():
        x, w = _inputs(d, tag)
        assert x.shape == cfg["shape"] == w.shape and x.shape[1 if cfg["format"] == "bchw" else 2] == 16 * cfg["d"]
        assert d[f"{tag}_x"].dtype == np.float16 and d[f"{tag}_indices"].dtype == np.int64 and np.isfinite(x).all()
        assert d[f"{tag}_indices"].size * 16 == x.size and float(d[f"{tag}_g_aux"]) == R.G_AUX
        for name in R.SCALARS:
            assert float(d[f"{tag}_{name}_ref_err"]) >= 0.0 and float(d[f"{tag}_{name}_abs"]) > 0.0
            assert np.isfinite(float(d[f"{tag}_{name}64"])) and d[f"{tag}_{name}"].dtype == np.float32
        assert float(d[f"{tag}_grad_x_ref_err"]) > 0.0
    blc = {c["d"] for c in list(R.BSQ_VARIANT_CASES.values()) + list(R.BSQ_CASES.values()) if c["format"] == "blc" or c.get("channels_last")}
    assert set(range(5, 16)) - {7} <= blc                                             # (d = 7 and 16 run in the GPU test's MULTI)
    assert os.path.getsize(G29) < (400 << 10)


@pytest.mark.parametrize("tag", list(R.BSQ_VARIANT_CASES))
def test_bsq_checker_reproduces_the_variant_fixture(tag):
    """The checker equals the reference's fp64 scalars to 1e-12 and lies within ref_err of its fp32 run; g29 holds no grad_x64 (the
    generator asserted the checker's against the reference's fp64 autograd to 1e-12 of the sum of |terms|)."""
    d, cfg = np.load(G29), R.BSQ_VARIANT_CASES[tag]
    x, w = _inputs(d, tag)
    s = R.bsq64(x, cfg, w, float(d[f"{tag}_g_aux"]))
    for name in R.SCALARS:
        v64 = float(d[f"{tag}_{name}64"])
        assert abs(s[name] - v64) <= 1e-12 * max(abs(v64), s[name + "_abs"])
        assert abs(s[name + "_abs"] - float(d[f"{tag}_{name}_abs"])) <= 1e-12 * s[name + "_abs"]
        assert R.err_units(d[f"{tag}_{name}"], s[name], s[name + "_abs"]) <= float(d[f"{tag}_{name}_ref_err"]) * (1 + 1e-6) + 1e-6
    assert np.array_equal(s["indices"], d[f"{tag}_indices"])
    assert np.isfinite(s["grad_x"]).all() and (s["grad_x_abs"] > 0).all()


@pytest.mark.parametrize("tag", list(R.BSQ_VARIANT_CASES))
def test_cpu_bsq_train_step_lands_on_the_variant_fixture(tag, monkeypatch):
    """The three checks of test_cpu_bsq_train_step_lands_on_the_fixture at the new widths; quantized against +-q_scale."""
    d, cfg = np.load(G29), R.BSQ_VARIANT_CASES[tag]
    x, w = _inputs(d, tag)
    quantized, info, grad = _cpu_bsq_step(cfg, x, w, float(d[f"{tag}_g_aux"]), monkeypatch)
    s = R.bsq64(x, cfg, w, float(d[f"{tag}_g_aux"]))
    assert np.array_equal(info["indices"].numpy(), d[f"{tag}_indices"])
    qs = float(np.float32(1.0 / np.sqrt(16 * cfg["d"])))
    assert np.all(np.abs(quantized - np.where(s["u"] > 0, qs, -qs)) <= 3 * R.U * qs)
    for name in R.SCALARS:
        got = R.err_units(float(info[name].detach()), float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        assert got <= 2.0 * float(d[f"{tag}_{name}_ref_err"]) + 2.0, (name, got)
    got = R.err_units(grad, s["grad_x"], s["grad_x_abs"])
    assert got <= 2.0 * float(d[f"{tag}_grad_x_ref_err"]) + 2.0, got


@pytest.mark.parametrize("tag", list(R.FSQ_CASES))
def test_cpu_fsq_train_step_lands_on_the_fixture(tag, monkeypatch):
    """The torch branch of FSQQuantizer on the CPU, with the oracle answering for the library's quantise call: the straight-through
    value is the rounded branch and grad_z that of the soft branch, within twice the reference's own fp32 error."""
    from oracle import gq_oracle as O
    from pit_hip import _lib as L
    from pit_hip.quantization.fsq import FSQQuantizer

    f, cfg = _fsq(), R.FSQ_CASES[tag]

    def cpu_quantize(zf, levels):
        zh, ind = O.fsq_forward(zf.numpy()[None], levels, "blc")
        return torch.from_numpy(zh[0]), torch.from_numpy(ind.reshape(-1))

    monkeypatch.setattr(L, "fsq_quantize", cpu_quantize)
    monkeypatch.setenv("GQHIP_FSQ_TRAIN_FUSED", "1")
    z, w = _inputs(f, tag, "z")
    zt = _as_input(z, cfg)
    zhat, info = FSQQuantizer(cfg["levels"], cfg["format"]).train()(zt)
    assert set(info) == {"indices", "bits"} and "FSQTrainFn" not in type(zhat.grad_fn).__name__
    (zhat * torch.from_numpy(w)).sum().backward()
    assert np.array_equal(info["indices"].numpy(), f[f"{tag}_indices"]) and info["indices"].dtype == torch.int32
    assert np.allclose(zhat.detach().numpy(), f[f"{tag}_zhat"], rtol=0, atol=2.0 ** -21)
    got = R.err_units(zt.grad.numpy(), f[f"{tag}_grad_z64"], f[f"{tag}_grad_z_abs"])
    assert got <= 2.0 * float(f[f"{tag}_grad_z_ref_err"]) + 2.0, got
