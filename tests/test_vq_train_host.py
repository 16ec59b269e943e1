"""CPU: the host half of VQQuantizer's fused train step -- the entry points exist, are bound and validate their arguments before any
HIP call, the fixture g24 loads, the fp64 checker the GPU tests rely on (tests/vq_train_ref.py) reproduces the reference's autograd
gradients within the reference's own fp32 error and agrees with a central difference, and a CPU VQQuantizer step (the op-by-op
branch, which CPU tensors keep) equals the fixture."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vq_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INVALID, WORKSPACE = 1, 2          # GQHIP_ERR_INVALID_ARG, GQHIP_ERR_WORKSPACE


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


def _fixture():
    return np.load(os.path.join(G, "g24_vq_train_step.npz"))


def _emb(d, tag, it):
    """The codebook before step `it`: stored (float16, exact) for step 0, one plain SGD update later for step 1."""
    emb = d[f"{tag}_emb"].astype(np.float32)
    return emb if it == 0 else (emb - np.float32(d[f"{tag}_lr"]) * d[f"{tag}_0_grad_emb"]).astype(np.float32)


def test_vq_backward_symbols_are_exported_and_bound():
    L = _lib()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("vq_backward_f32", "vq_backward_workspace_bytes"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(dll, name) and hasattr(L.lib(), name)
    assert L.lib().gqhip_abi_version() == L.ABI_VERSION == 8         # additive: the version does not move


def test_vq_backward_wrapper_exists():
    import inspect

    L = _lib()
    assert callable(getattr(L, "vq_backward", None))
    names = list(inspect.signature(L.vq_backward).parameters)
    assert names == ["z", "emb", "idx", "dim", "layout", "beta", "legacy", "g_zq", "g_loss", "want_grad_z", "want_grad_emb", "ws"]
    p = inspect.signature(L.vq_quantize_z).parameters
    assert p["use_cache"].default is True
    with pytest.raises(L.GqHipError):                                   # no CPU fallback
        L.vq_backward(torch.zeros(1, 4, 2, 2), torch.zeros(8, 4), torch.zeros(1, 1, 2, 2, dtype=torch.int64), 4, "bchw", 0.25, True)


def test_workspace_query():
    L = _lib().lib()
    q = L.vq_backward_workspace_bytes
    assert q(0, 64, 16) > 0 and q(5000, 64, 16) > q(100, 64, 16) > 0
    assert q(65536, 65536, 16) < (4 << 20)                              # the 512^2 step: a few MiB at the most
    for bad in ((-1, 64, 16), (10, 0, 16), (10, 64, 0), (10, 64, 65), (1 << 30, 64, 16)):
        assert q(*bad) == -1, bad


def _back(L, z=64, emb=64, idx=64, gl=None, gz=64, ge=None, B=2, Lp=4, c=16, dim=8, n=32, layout=0, ws=64, wsb=1 << 30):
    return L.vq_backward_f32(z, emb, idx, None, gl, gz, ge, B, Lp, c, dim, n, layout, 0.25, 1, ws, wsb, None)


def test_vq_backward_validates_before_any_hip_call():
    """Pointers here are small fake addresses: every call must be rejected on its arguments alone."""
    L = _lib().lib()
    for kw in (dict(z=None), dict(emb=None), dict(idx=None), dict(gl=66), dict(c=16, dim=5), dict(dim=0), dict(dim=65, c=65),
               dict(layout=2), dict(Lp=0), dict(B=-1), dict(n=0), dict(ws=72)):
        assert _back(L, **kw) == INVALID, kw
    assert _back(L, ws=None) == WORKSPACE
    assert _back(L, wsb=L.vq_backward_workspace_bytes(2 * 4 * 2, 32, 8) - 1) == WORKSPACE
    assert _back(L, B=0, ws=None, wsb=0) == 0                            # no items, no grad_emb: nothing to do


def test_fixture_loads_and_is_complete():
    d = _fixture()
    for tag, cfg in R.CASES.items():
        assert d[f"{tag}_emb"].shape == (cfg["n"], cfg["dim"])
        for it in range(R.STEPS):
            p = f"{tag}_{it}_"
            for k in ("z", "w", "g_loss", "zq", "indices", "codebook_loss", "grad_z", "grad_emb", "gz64", "gz_abs", "ge64", "ge_abs",
                      "gz_ref_err", "ge_ref_err"):
                assert p + k in d.files, p + k
            assert d[p + "z"].shape == cfg["shape"] == d[p + "grad_z"].shape == d[p + "zq"].shape and d[p + "z"].dtype == np.float32
            assert d[p + "grad_emb"].shape == (cfg["n"], cfg["dim"]) and d[p + "indices"].dtype == np.int64
            assert d[p + "indices"].size * cfg["dim"] == d[p + "z"].size
    assert d["bchw_d4_k4_odd_0_z"][0, 0].size % 4 != 0                 # the 4-byte access path
    counts = np.bincount(d["bchw_d16_crowded_0_indices"].reshape(-1), minlength=256)
    assert counts.max() >= 8 and (counts == 0).any()                   # several items on one code, and codes nobody chose
    assert os.path.getsize(os.path.join(G, "g24_vq_train_step.npz")) < (1 << 20)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_formula_helper_reproduces_the_fixture(tag):
    """The fp64 helper, run on the fixture's inputs, gives the fixture's fp64 gradients (it made them) and lies within ref_err of
    the reference's fp32 autograd gradients; loss and z_q are the reference's."""
    d, cfg = _fixture(), R.CASES[tag]
    for it in range(R.STEPS):
        p = f"{tag}_{it}_"
        s = R.step(d[p + "z"], _emb(d, tag, it), d[p + "indices"], cfg, d[p + "w"], float(d[p + "g_loss"]))
        assert np.allclose(s["grad_z"], d[p + "gz64"], rtol=1e-12, atol=1e-300)
        assert np.allclose(s["grad_emb"], d[p + "ge64"], rtol=1e-12, atol=1e-300)
        assert R.err_units(d[p + "grad_z"], s["grad_z"], s["grad_z_abs"]) <= float(d[p + "gz_ref_err"]) * (1 + 1e-9)
        assert R.err_units(d[p + "grad_emb"], s["grad_emb"], s["grad_emb_abs"]) <= float(d[p + "ge_ref_err"]) * (1 + 1e-9)
        assert abs(s["loss"] - float(d[p + "codebook_loss"])) <= 2e-5 * max(1.0, abs(s["loss"]))
        assert np.abs(d[p + "zq"] - s["e"]).max() <= 4 * R.U * np.abs(s["e"]).max() + 1e-7
        chosen = np.zeros(cfg["n"], bool)
        chosen[d[p + "indices"].reshape(-1)] = True
        assert np.all(d[p + "grad_emb"][~chosen] == 0.0) and np.all(s["grad_emb_abs"][chosen] > 0)


def test_formula_helper_against_a_central_difference():
    """48 random elements of z and of the chosen codebook rows, step 1e-6 in fp64 with the indices frozen: agreement within 1e-5 of
    the sum of |terms| -- coarse on purpose (a wrong formula is off by order 1)."""
    tag = "blc_d8_k2"
    d, cfg = _fixture(), R.CASES[tag]
    p = f"{tag}_0_"
    z, emb, idx, w, gl = d[p + "z"].astype(np.float64), _emb(d, tag, 0).astype(np.float64), d[p + "indices"], d[p + "w"], float(d[p + "g_loss"])
    s = R.step(z, emb, idx, cfg, w, gl)
    rng = np.random.default_rng(7)
    h = 1e-6
    for flat in rng.choice(z.size, 48, replace=False):
        i = np.unravel_index(flat, z.shape)
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        num = (R.loss64(zp, emb, idx, cfg, w, gl) - R.loss64(zm, emb, idx, cfg, w, gl)) / (2 * h)
        # z moves both MSE terms of loss64; only the first is differentiated with respect to z
        a, b = (1.0, cfg["beta"]) if cfg["legacy"] else (cfg["beta"], 1.0)
        want = w[i] + (s["grad_z"][i] - w[i]) * (a + b) / a
        assert abs(num - want) <= 1e-5 * max(s["grad_z_abs"][i] * (a + b) / a, 1e-3), (i, num, want)
    rows = rng.choice(np.unique(idx), 6, replace=False)
    for j in rows:
        for dcol in range(cfg["dim"]):
            ep, em = emb.copy(), emb.copy()
            ep[j, dcol] += h
            em[j, dcol] -= h
            num = (R.loss64(z, ep, idx, cfg, w, gl) - R.loss64(z, em, idx, cfg, w, gl)) / (2 * h)
            a, b = (1.0, cfg["beta"]) if cfg["legacy"] else (cfg["beta"], 1.0)
            want = s["grad_emb"][j, dcol] * (a + b) / b
            assert abs(num - want) <= 1e-5 * max(s["grad_emb_abs"][j, dcol] * (a + b) / b, 1e-3), (j, dcol, num, want)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_cpu_module_train_step_equals_the_fixture(tag, monkeypatch):
    """A CPU tensor keeps the op-by-op branch.  That branch asks the library for the arg-min, which has no CPU implementation: here
    the fp64 arbiter of the oracle answers in its place (the fixture's indices ARE the arbiter's), so what is checked is the
    differentiable glue -- z_q and the indices bit for bit, the loss and both gradients within the reference's own error."""
    from oracle import gq_oracle as O
    from pit_hip import _lib as L
    from pit_hip.quantization.vq import VQQuantizer

    def cpu_argmin(z, emb, ws=None, use_cache=True):
        idx = O.vq_argmin_rows(z.numpy(), emb.numpy())
        return torch.from_numpy(idx), None

    monkeypatch.setattr(L, "vq_argmin", cpu_argmin)
    d, cfg = _fixture(), R.CASES[tag]
    m = VQQuantizer(cfg["format"], cfg["n"], cfg["dim"], beta=cfg["beta"], codebook_num=cfg["K"], legacy=cfg["legacy"]).train()
    m.embedding.weight.data = torch.from_numpy(_emb(d, tag, 0))
    lr = torch.tensor(float(d[f"{tag}_lr"]), dtype=torch.float32)
    for it in range(R.STEPS):
        p = f"{tag}_{it}_"
        z = torch.from_numpy(d[p + "z"]).requires_grad_(True)
        m.embedding.weight.grad = None
        zq, info = m(z)
        assert set(info) == {"indices", "codebook_loss"} and "VQTrainFn" not in type(info["codebook_loss"].grad_fn).__name__
        ((zq * torch.from_numpy(d[p + "w"])).sum() + float(d[p + "g_loss"]) * info["codebook_loss"]).backward()
        assert np.array_equal(info["indices"].numpy(), d[p + "indices"])
        assert np.array_equal(zq.detach().numpy(), d[p + "zq"])
        assert abs(float(info["codebook_loss"].detach()) - float(d[p + "codebook_loss"])) <= 2e-5 * max(1.0, float(d[p + "codebook_loss"]))
        bound = 2.0 * max(float(d[k]) for k in d.files if k.endswith("_ref_err"))
        assert R.err_units(z.grad.numpy(), d[p + "gz64"], d[p + "gz_abs"]) <= bound
        assert R.err_units(m.embedding.weight.grad.numpy(), d[p + "ge64"], d[p + "ge_abs"]) <= bound
        m.embedding.weight.data = m.embedding.weight.data - lr * m.embedding.weight.grad
