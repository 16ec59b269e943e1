"""CPU: the host half of LFQQuantizer's fused train step -- the three entry points exist, are bound and validate their arguments
before any HIP call, the fixture g25 loads, the fp64 checker the GPU tests rely on (tests/lfq_train_ref.py) agrees with the dense
[R, N] formula, with the reference's fp64 autograd and with a central difference, and a CPU LFQQuantizer step (the torch branch,
which CPU tensors keep) equals the fixture.  The same for g28, the fixture of the kernel variants g25 leaves out."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import lfq_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INVALID, WORKSPACE = 1, 2          # GQHIP_ERR_INVALID_ARG, GQHIP_ERR_WORKSPACE
NAMES = ("lfq_train_workspace_bytes", "lfq_train_f32", "lfq_backward_f32")


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


def _fixture():
    return np.load(os.path.join(G, "g25_lfq_train_step.npz"))


def _inputs(d, tag):
    return d[f"{tag}_x"].astype(np.float32), d[f"{tag}_w"].astype(np.float32)


# ---- these fail on the parent commit -----------------------------------------------------------------------------------------------
def test_lfq_train_symbols_are_exported_bound_and_in_the_header():
    L = _lib()
    dll = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gqhip.h")).read()
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS and hasattr(dll, name) and hasattr(L.lib(), name)
        assert name + "(" in header
    assert L.lib().gqhip_abi_version() == L.ABI_VERSION == 8         # additive: the version does not move
    assert "#define GQHIP_ABI_VERSION 8" in " ".join(header.split())


def test_lfq_train_wrappers_exist_and_have_no_cpu_fallback():
    L = _lib()
    assert list(inspect.signature(L.lfq_train).parameters) == ["x", "num_codebooks", "dim", "layout", "w_s", "w_b", "ws"]
    assert list(inspect.signature(L.lfq_backward).parameters) == ["x", "avg", "num_codebooks", "dim", "layout", "w_s", "w_b", "g_q",
                                                                  "g_aux", "g_commit", "ws"]
    assert callable(L.LfqTrainWorkspace().get)
    with pytest.raises(L.GqHipError):
        L.lfq_train(torch.zeros(1, 8, 2, 2), 2, 4, "bchw")
    with pytest.raises(L.GqHipError):
        L.lfq_backward(torch.zeros(1, 8, 2, 2), torch.zeros(16), 2, 4, "bchw")


def test_lfq_workspace_query():
    q = _lib().lib().lfq_train_workspace_bytes
    assert q(0, 8) > 0
    sizes = [q(r, 16) for r in (1, 255, 256, 257, 4099, 16384)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert q(16384, 16) < 16384 * 65536 * 4 // 16                      # the [R, N] matrix never exists, not even a sixteenth of it
    for d in range(1, 17):
        assert q(1000, d) > 0
    for bad in ((10, 0), (10, 17), (-1, 8), (1 << 30, 8)):
        assert q(*bad) == -1, bad


def _train(L, x=64, qz=64, idx=64, avg=64, sc=64, B=2, Lp=4, C=16, nc=2, d=8, layout=0, ws=64, wsb=1 << 30):
    return L.lfq_train_f32(x, qz, idx, avg, sc, B, Lp, C, nc, d, layout, 1.0, 1.0, ws, wsb, None)


def _back(L, x=64, avg=64, gq=None, ga=None, gc=None, gx=64, B=2, Lp=4, C=16, nc=2, d=8, layout=0, ws=64, wsb=1 << 30):
    return L.lfq_backward_f32(x, avg, gq, ga, gc, gx, B, Lp, C, nc, d, layout, 1.0, 1.0, ws, wsb, None)


BAD_SHAPES = (dict(C=17), dict(d=0, C=0), dict(d=17, nc=1, C=17), dict(nc=0, C=0), dict(nc=8, d=8, C=64), dict(layout=2),
              dict(layout=-1), dict(B=-1), dict(Lp=-1))


def test_lfq_calls_validate_before_any_hip_call():
    """Pointers here are small fake addresses: every call must be rejected on its arguments alone."""
    L = _lib().lib()
    need = L.lfq_train_workspace_bytes(2 * 4 * 2, 8)
    for kw in (dict(x=None), dict(qz=None), dict(idx=None), dict(avg=None), dict(sc=None), dict(avg=66), dict(sc=66)) + BAD_SHAPES:
        assert _train(L, **kw) == INVALID, kw
    for kw in (dict(x=None), dict(avg=None), dict(gx=None), dict(ga=66), dict(gc=66), dict(avg=66)) + BAD_SHAPES:
        assert _back(L, **kw) == INVALID, kw
    for call in (_train, _back):
        assert call(L, ws=None) == WORKSPACE
        assert call(L, ws=72) == WORKSPACE                              # not 16-byte aligned
        assert call(L, wsb=need - 1) == WORKSPACE
        assert call(L, B=0, ws=None, wsb=0) == 0 and call(L, Lp=0, ws=None, wsb=0) == 0       # empty input


# ---- these pass on the parent commit: they prove the checker -----------------------------------------------------------------------
def test_fixture_loads_and_is_complete():
    d = _fixture()
    for tag, cfg in R.CASES.items():
        x, w = _inputs(d, tag)
        assert x.shape == cfg["shape"] == w.shape == d[f"{tag}_grad_x"].shape == d[f"{tag}_grad_x64"].shape == d[f"{tag}_quantized"].shape
        assert d[f"{tag}_x"].dtype == np.float16 and d[f"{tag}_indices"].dtype == np.int64 and np.isfinite(x).all()
        assert d[f"{tag}_indices"].size * cfg["d"] * cfg["nc"] == x.size
        for name in R.SCALARS + ("grad_x",):
            assert float(d[f"{tag}_{name}_ref_err"]) >= 0.0
    x = _inputs(d, "blc_32x3_odd")[0]
    assert (x == 0).sum() >= 2 and (np.abs(x) == 50).sum() == 2 and ((np.abs(x) > 0) & (np.abs(x) < 2e-4)).sum() >= 2
    assert os.path.getsize(os.path.join(G, "g25_lfq_train_step.npz")) < (400 << 10)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_factorised_equals_dense(tag):
    d, cfg = _fixture(), R.CASES[tag]
    x, _ = _inputs(d, tag)
    f, dn = R.factorised64(x, cfg), R.dense64(x, cfg)
    for name in R.SCALARS:
        assert abs(f[name] - dn[name]) <= 1e-12 * max(abs(dn[name]), dn[name + "_abs"]), name
        assert abs(f[name + "_abs"] - dn[name + "_abs"]) <= 1e-12 * dn[name + "_abs"]


@pytest.mark.parametrize("tag", list(R.CASES))
def test_checker_reproduces_the_fixture(tag):
    """The checker equals the reference's fp64 run (scalars to 1e-12; grad_x to 1e-7 of its sum of |terms|: the reference's fp64
    softmax backward cancels among logits of magnitude 1e4 where x = +-50) and lies within ref_err of its fp32 run."""
    d, cfg = _fixture(), R.CASES[tag]
    x, w = _inputs(d, tag)
    s = R.factorised64(x, cfg, w, float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"]))
    for name in R.SCALARS:
        v64 = float(d[f"{tag}_{name}64"])
        assert abs(s[name] - v64) <= 1e-12 * max(abs(v64), s[name + "_abs"])
        assert abs(s[name + "_abs"] - float(d[f"{tag}_{name}_abs"])) <= 1e-12 * s[name + "_abs"]
        assert R.err_units(d[f"{tag}_{name}"], s[name], s[name + "_abs"]) <= float(d[f"{tag}_{name}_ref_err"]) * (1 + 1e-6) + 1e-6
    assert np.all(np.abs(s["grad_x"] - d[f"{tag}_grad_x64"]) <= 1e-7 * s["grad_x_abs"])
    assert np.allclose(s["grad_x_abs"], d[f"{tag}_grad_x_abs"], rtol=1e-6)
    assert R.err_units(d[f"{tag}_grad_x"], s["grad_x"], s["grad_x_abs"]) <= float(d[f"{tag}_grad_x_ref_err"]) * (1 + 1e-3) + 1e-3
    q = np.where(x > 0, 1.0, -1.0).astype(np.float32)
    assert np.array_equal(d[f"{tag}_quantized"], x + (q - x))            # two rounded fp32 operations, NOT always q
    bits = (R.to_rows(x, cfg)[0] > 0).reshape(-1, cfg["d"] * cfg["nc"])
    want = np.zeros(bits.shape[0], np.int64)
    for i in range(bits.shape[1]):
        want = want * 2 + bits[:, i]
    assert np.array_equal(d[f"{tag}_indices"].reshape(-1), want)


def test_checker_against_a_central_difference():
    """40 random elements (none of the special values), step 1e-7 in fp64 with the signs frozen: agreement within 1e-5 of the sum of
    |terms| -- coarse on purpose (a wrong formula is off by order 1)."""
    tag = "blc_32x3_odd"
    d, cfg = _fixture(), R.CASES[tag]
    x, w = (a.astype(np.float64) for a in _inputs(d, tag))
    ga, gc = float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"])
    s = R.factorised64(x, cfg, w, ga, gc)
    q = np.where(x > 0, 1.0, -1.0)
    rng = np.random.default_rng(11)
    h = 1e-7
    ok = np.flatnonzero((np.abs(x) > 1e-3).reshape(-1) & (np.abs(x) < 1).reshape(-1))
    for flat in rng.choice(ok, 40, replace=False):
        i = np.unravel_index(flat, x.shape)
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        num = (R.loss64(xp, cfg, w, ga, gc, q) - R.loss64(xm, cfg, w, ga, gc, q)) / (2 * h)
        assert abs(num - s["grad_x"][i]) <= 1e-5 * max(s["grad_x_abs"][i], 1e-3), (i, num, s["grad_x"][i])


def _cpu_module_step(cfg, x, w, g_aux, g_commit, monkeypatch):
    """One train step of the CPU module under autograd: (quantized, info, x.grad)."""
    from pit_hip import _lib as L
    from pit_hip.quantization.lfq import LFQQuantizer

    def cpu_pack(x):
        bits = x > 0
        idx = torch.zeros(x.shape[0], dtype=torch.int64)
        for i in range(x.shape[1]):
            idx = idx * 2 + bits[:, i]
        return idx, torch.where(bits, 1.0, -1.0)

    monkeypatch.setattr(L, "lfq_pack", cpu_pack)
    m = LFQQuantizer(cfg["format"], 1 << cfg["d"], cfg["nc"], sample_minimization_weight=cfg.get("w_s", 1.0),
                     batch_maximization_weight=cfg.get("w_b", 1.0)).train()
    xt = torch.from_numpy(x)
    if cfg.get("channels_last"):
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt.requires_grad_(True)
    quantized, info = m(xt)
    assert set(info) == {"indices", "entropy_aux_loss", "per_sample_entropy", "codebook_entropy", "commit_loss"}
    assert "LFQTrainFn" not in type(info["entropy_aux_loss"].grad_fn).__name__
    ((quantized * torch.from_numpy(w)).sum() + g_aux * info["entropy_aux_loss"] + g_commit * info["commit_loss"]).backward()
    return quantized.detach().numpy(), info, xt.grad.numpy()


@pytest.mark.parametrize("tag", list(R.CASES))
def test_cpu_module_train_step_equals_the_fixture(tag, monkeypatch):
    """A CPU tensor keeps the torch branch.  That branch asks the library for the sign pack, which has no CPU implementation: numpy
    answers in its place, so what is checked is the differentiable glue -- quantized and the indices bit for bit, the scalars and
    grad_x within twice the reference's own fp32 error (torch's CPU softmax is the reference's)."""
    d, cfg = _fixture(), R.CASES[tag]
    x, w = _inputs(d, tag)
    quantized, info, grad = _cpu_module_step(cfg, x, w, float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"]), monkeypatch)
    assert np.array_equal(info["indices"].numpy(), d[f"{tag}_indices"])
    assert np.array_equal(quantized, d[f"{tag}_quantized"])
    for name in R.SCALARS:
        got = R.err_units(float(info[name].detach()), float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        assert got <= 2.0 * float(d[f"{tag}_{name}_ref_err"]) + 2.0, (name, got)
    got = R.err_units(grad, d[f"{tag}_grad_x64"], d[f"{tag}_grad_x_abs"])
    assert got <= 2.0 * float(d[f"{tag}_grad_x_ref_err"]) + 2.0, got


# ---- g28: the kernel variants the cases above never launch (R.VARIANT_CASES) -------------------------------------------------------
G28 = os.path.join(G, "g28_lfq_train_variants.npz")


def _vinputs(d, tag):
    return R.variant(d, tag, "x").astype(np.float32), R.variant(d, tag, "w").astype(np.float32)


def _indices(x, cfg):
    """The big-endian pack of a position's nc d sign bits, in the module's shape."""
    bits = (R.to_rows(x, cfg)[0] > 0).reshape(-1, cfg["d"] * cfg["nc"])
    want = np.zeros(bits.shape[0], np.int64)
    for i in range(bits.shape[1]):
        want = want * 2 + bits[:, i]
    return want


def test_variant_fixture_loads_and_is_complete():
    d = np.load(G28)
    widths = set()
    for tag, cfg in R.VARIANT_CASES.items():
        x, w = _vinputs(d, tag)
        assert x.shape == cfg["shape"] == w.shape == R.variant(d, tag, "grad_x64").shape
        assert R.variant(d, tag, "x").dtype == np.float16 and d[f"{tag}_indices"].dtype == np.int64 and np.isfinite(x).all()
        assert R.variant(d, tag, "grad_x64").dtype == np.float64
        assert d[f"{tag}_indices"].size * cfg["d"] * cfg["nc"] == x.size
        assert float(d[f"{tag}_g_aux"]) == R.G_AUX and float(d[f"{tag}_g_commit"]) == R.G_COMMIT
        for name in R.SCALARS:
            assert float(d[f"{tag}_{name}_ref_err"]) >= 0.0 and float(d[f"{tag}_{name}_abs"]) > 0.0
            assert np.isfinite(float(d[f"{tag}_{name}64"])) and d[f"{tag}_{name}"].dtype == np.float32
        assert float(d[f"{tag}_grad_x_ref_err"]) > 0.0
        widths.add(cfg["d"])
    assert widths | {c["d"] for c in R.CASES.values()} == set(range(1, 17))          # every code width has a fixture case
    assert np.array_equal(_vinputs(d, "blc_d13x4")[0].reshape(-1), _vinputs(d, "blc_d13")[0].reshape(-1))
    assert os.path.getsize(G28) < (400 << 10)


@pytest.mark.parametrize("tag", list(R.VARIANT_CASES))
def test_checker_reproduces_the_variant_fixture(tag):
    """As test_checker_reproduces_the_fixture; g28 stores neither quantized nor grad_x_abs, the rules state them."""
    d, cfg = np.load(G28), R.VARIANT_CASES[tag]
    x, w = _vinputs(d, tag)
    s = R.factorised64(x, cfg, w, float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"]))
    for name in R.SCALARS:
        v64 = float(d[f"{tag}_{name}64"])
        assert abs(s[name] - v64) <= 1e-12 * max(abs(v64), s[name + "_abs"])
        assert abs(s[name + "_abs"] - float(d[f"{tag}_{name}_abs"])) <= 1e-12 * s[name + "_abs"]
        assert R.err_units(d[f"{tag}_{name}"], s[name], s[name + "_abs"]) <= float(d[f"{tag}_{name}_ref_err"]) * (1 + 1e-6) + 1e-6
    assert np.all(np.abs(s["grad_x"] - R.variant(d, tag, "grad_x64")) <= 1e-7 * s["grad_x_abs"])
    if cfg["d"] <= 12:
        dn = R.dense64(x, cfg)
        for name in R.SCALARS:
            assert abs(s[name] - dn[name]) <= 1e-12 * max(abs(dn[name]), dn[name + "_abs"]), name
    assert np.array_equal(d[f"{tag}_indices"].reshape(-1), _indices(x, cfg))


@pytest.mark.parametrize("tag", list(R.VARIANT_CASES))
def test_cpu_module_train_step_equals_the_variant_fixture(tag, monkeypatch):
    """The three checks of test_cpu_module_train_step_equals_the_fixture at the new widths; quantized is x + (q - x) in fp32, which
    the generator asserted of the reference's."""
    d, cfg = np.load(G28), R.VARIANT_CASES[tag]
    x, w = _vinputs(d, tag)
    quantized, info, grad = _cpu_module_step(cfg, x, w, float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"]), monkeypatch)
    assert np.array_equal(info["indices"].numpy(), d[f"{tag}_indices"])
    assert np.array_equal(quantized, x + (np.where(x > 0, 1.0, -1.0).astype(np.float32) - x))
    for name in R.SCALARS:
        got = R.err_units(float(info[name].detach()), float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        assert got <= 2.0 * float(d[f"{tag}_{name}_ref_err"]) + 2.0, (name, got)
    s = R.factorised64(x, cfg, w, float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"]))
    got = R.err_units(grad, R.variant(d, tag, "grad_x64"), s["grad_x_abs"])
    assert got <= 2.0 * float(d[f"{tag}_grad_x_ref_err"]) + 2.0, got
