"""-m gpu: VQQuantizer's fused train step -- vq_quantize_z_f32 without a cache (the forward), vq_backward_f32 (grad_z, and grad of
the codebook as a bit-reproducible scatter-reduce) and the autograd.Function that puts them behind VQQuantizer -- against the
fixture captured from the reference's CPU autograd (g24: tests/golden/make_golden_vq_train.py) and the fp64 restatement
tests/vq_train_ref.py (proven on the CPU by tests/test_vq_train_host.py).

Gradient bound against the fixture: 2 x the LARGEST error the reference's own fp32 autograd shows against the fp64 formulas
(*_ref_err, in units of 2^-24 x sum of |terms|), read from the fixture; the factor 2 is headroom for op-order differences only.
The fixture's rows all keep an fp64 top-2 distance gap above 1e-4 and its indices are the fp64 arbiter's, so every element is
compared.  grad_emb's own value contract (one fp32 rounding of an fp64 sum) is checked on synthetic indices against math.fsum."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import vq_train_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
WORKSPACE = 2          # GQHIP_ERR_WORKSPACE


def _fixture():
    return np.load(os.path.join(G, "g24_vq_train_step.npz"))


def _bound(d):
    return 2.0 * max(float(d[k]) for k in d.files if k.endswith("_ref_err"))


def _emb(d, tag, it):
    emb = d[f"{tag}_emb"].astype(np.float32)
    return emb if it == 0 else (emb - np.float32(d[f"{tag}_lr"]) * d[f"{tag}_0_grad_emb"]).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------ 1. library level vs the fixture
@pytest.mark.parametrize("tag", list(R.CASES))
def test_library_step_matches_the_reference_fixture(tag):
    from pit_hip import _lib

    d, cfg = _fixture(), R.CASES[tag]
    bound = _bound(d)
    ws, bws = _lib.Workspace(), _lib.VqBackwardWorkspace()
    for it in range(R.STEPS):
        p = f"{tag}_{it}_"
        z, emb = _dev(d[p + "z"]), _dev(_emb(d, tag, it))
        idx, zq, loss = _lib.vq_quantize_z(z, emb, cfg["dim"], cfg["format"], cfg["beta"], cfg["legacy"], ws, use_cache=False)
        gz, ge = _lib.vq_backward(z, emb, idx, cfg["dim"], cfg["format"], cfg["beta"], cfg["legacy"], g_zq=_dev(d[p + "w"]),
                                  g_loss=_scalar(d[p + "g_loss"]), ws=bws)
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), d[p + "indices"])
        assert np.array_equal(zq.cpu().numpy(), d[p + "zq"])
        got, want = float(loss[0]), float(d[p + "codebook_loss"])
        print(f"{tag} step {it}: loss {got!r} vs {want!r}")
        assert abs(got - want) <= 2e-5 * abs(want)
        ez = R.err_units(gz.cpu().numpy(), d[p + "gz64"], d[p + "gz_abs"])
        ee = R.err_units(ge.cpu().numpy(), d[p + "ge64"], d[p + "ge_abs"])
        print(f"{tag} step {it}: grad_z {ez:.2f} units (reference {float(d[p + 'gz_ref_err']):.2f}), grad_emb {ee:.2f} units "
              f"(reference {float(d[p + 'ge_ref_err']):.2f}), bound {bound:.2f}")
        assert ez <= bound and ee <= bound, (it, ez, ee, bound)


# ------------------------------------------------------------------------------------------ 2. grad_emb's value contract
ITEMS, N, DIM = 5000, 64, 16
SHAPE = (2, DIM, 50, 50)                    # bchw, K = 1: 2 * 2500 items
BETA, G_LOSS = 0.25, 0.81


def _pattern(name):
    rng = np.random.default_rng(11)
    if name == "random":
        return rng.integers(0, N, ITEMS)
    if name == "one code":                  # a list that crosses every chunk boundary
        return np.full(ITEMS, 37)
    assert name == "codes 0 and 63"
    return np.where(rng.random(ITEMS) < 0.3, 0, N - 1)


_synthetic = {}


def _inputs():
    """z, emb, g_zq of the synthetic cases, drawn once."""
    if not _synthetic:
        g = torch.Generator().manual_seed(5)
        _synthetic.update(z=0.5 * torch.randn(SHAPE, generator=g), emb=0.5 * torch.randn(N, DIM, generator=g),
                          w=torch.randn(SHAPE, generator=g))
    return _synthetic["z"], _synthetic["emb"], _synthetic["w"]


def _exact_grad_emb(z, emb, items_idx, cfg, g_loss, n):
    """Per code and column: coef * S with S = math.fsum of the fp32 differences e - z (exact to 2^-53), and the contract's bound
    2^-24 |coef S| + items 2^-53 |coef| sum |terms|: one fp32 rounding plus an fp64 accumulation in any order."""
    zi, _ = R.to_items(z, cfg)
    ok = (items_idx >= 0) & (items_idx < n)
    safe = np.where(ok, items_idx, 0)
    terms = (emb[safe] - zi).astype(np.float32).astype(np.float64)          # fl32(e - z): numpy subtracts fp32 from fp32 in fp32
    b = cfg["beta"] if cfg["legacy"] else 1.0
    coef = float(np.float32(g_loss)) * (b * 2.0 / float(z.size))
    want, bound = np.zeros((n, emb.shape[1])), np.zeros((n, emb.shape[1]))
    for j in np.unique(safe[ok]):
        rows = terms[ok & (safe == j)]
        for dcol in range(emb.shape[1]):
            s = math.fsum(rows[:, dcol])
            want[j, dcol] = coef * s
            bound[j, dcol] = R.U * abs(coef * s) + items_idx.size * 2.0 ** -53 * abs(coef) * math.fsum(np.abs(rows[:, dcol]))
    chosen = np.zeros(n, bool)
    chosen[safe[ok]] = True
    return want, bound, chosen


def _check_grad_emb(ge, want, bound, chosen):
    ge = ge.cpu().numpy()
    assert np.all(np.abs(ge.astype(np.float64) - want) <= bound), float((np.abs(ge - want) - bound).max())
    assert np.all(ge[~chosen] == 0.0) and not np.signbit(ge[~chosen]).any(), "an unchosen code is not exactly +0.0"


@pytest.mark.parametrize("name", ["random", "one code", "codes 0 and 63"])
def test_grad_emb_value_contract_and_run_to_run_identity(name):
    from pit_hip import _lib

    cfg = dict(format="bchw", dim=DIM, K=1, beta=BETA, legacy=True)
    z, emb, w = _inputs()
    items_idx = _pattern(name)
    idx = torch.from_numpy(items_idx.reshape(2, 2500).reshape(2, 1, 50, 50)).to(DEV)
    zd, ed, wd, gl = z.to(DEV), emb.to(DEV), w.to(DEV), _scalar(G_LOSS)
    want, bound, chosen = _exact_grad_emb(z.numpy(), emb.numpy(), items_idx, cfg, G_LOSS, N)
    bws = _lib.VqBackwardWorkspace()
    gz, ge = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=gl, ws=bws)
    _check_grad_emb(ge, want, bound, chosen)
    assert int(chosen.sum()) == {"random": N, "one code": 1, "codes 0 and 63": 2}[name]
    s = R.step(z.numpy(), emb.numpy(), idx.cpu().numpy(), cfg, w.numpy(), G_LOSS)
    # grad_z: fl32(z - e) exact to 2^-24 of the term, everything else fp64, one rounding of the sum: 2 units at the very worst
    assert R.err_units(gz.cpu().numpy(), s["grad_z"], s["grad_z_abs"]) <= 2.0
    # the same bits from a workspace full of 0xFF, and from a side stream
    bws.buf.fill_(0xFF)
    gz2, ge2 = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=gl, ws=bws)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gz3, ge3 = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=gl, ws=_lib.VqBackwardWorkspace())
    side.synchronize()
    for a, b in ((ge, ge2), (ge, ge3), (gz, gz2), (gz, gz3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,shape,dim,K,n", [
    # n = 1000: two 8-bit passes, not a power of two; 5000 items of two sub-codebooks in "blc": ten sort tiles per pass
    ("two passes, ten tiles", (4, 625, 16), 8, 2, 1000),
    # 70 000 items = 137 sort tiles: the digit table (256 x 137 entries) takes the scan kernel two rounds, with a carry between them
    ("137 tiles, two scan rounds", (1, 70000, 4), 4, 1, 300),
])
def test_grad_emb_larger_sorts(name, shape, dim, K, n):
    from pit_hip import _lib

    cfg = dict(format="blc", dim=dim, K=K, beta=BETA, legacy=False)
    items = shape[0] * shape[1] * K
    g = torch.Generator().manual_seed(6)
    z, emb, w = 0.5 * torch.randn(shape, generator=g), 0.5 * torch.randn(n, dim, generator=g), torch.randn(shape, generator=g)
    rng = np.random.default_rng(12)
    items_idx = np.where(rng.random(items) < 0.2, n - 1, rng.integers(0, n, items))       # one long list among short ones
    idx = torch.from_numpy(items_idx.reshape(shape[0], shape[1], K)).to(DEV)
    want, bound, chosen = _exact_grad_emb(z.numpy(), emb.numpy(), items_idx, cfg, G_LOSS, n)
    gz, ge = _lib.vq_backward(z.to(DEV), emb.to(DEV), idx, dim, "blc", BETA, False, g_zq=w.to(DEV), g_loss=_scalar(G_LOSS))
    _check_grad_emb(ge, want, bound, chosen)
    s = R.step(z.numpy(), emb.numpy(), idx.cpu().numpy(), cfg, w.numpy(), G_LOSS)
    assert R.err_units(gz.cpu().numpy(), s["grad_z"], s["grad_z_abs"]) <= 2.0, name


def test_out_of_range_indices_contribute_nothing():
    from pit_hip import _lib

    cfg = dict(format="bchw", dim=DIM, K=1, beta=BETA, legacy=True)
    z, emb, w = _inputs()
    items_idx = _pattern("random").copy()
    items_idx[123], items_idx[4321] = -1, N
    idx = torch.from_numpy(items_idx.reshape(2, 1, 50, 50)).to(DEV)
    want, bound, chosen = _exact_grad_emb(z.numpy(), emb.numpy(), items_idx, cfg, G_LOSS, N)
    gz, ge = _lib.vq_backward(z.to(DEV), emb.to(DEV), idx, DIM, "bchw", BETA, True, g_zq=w.to(DEV), g_loss=_scalar(G_LOSS))
    torch.cuda.synchronize()
    _check_grad_emb(ge, want, bound, chosen)
    gzi, _ = R.to_items(gz.cpu().numpy(), cfg)
    wi, _ = R.to_items(w.numpy(), cfg)
    for p in (123, 4321):                                               # no loss term: g_zq alone, bit for bit
        assert np.array_equal(gzi[p], wi[p])
    assert not np.array_equal(gzi[124], wi[124])


def test_null_gradients_skipped_outputs_and_short_workspace():
    from pit_hip import _lib

    cfg = dict(format="bchw", dim=DIM, K=1, beta=BETA, legacy=True)
    z, emb, w = _inputs()
    items_idx = _pattern("random")
    idx = torch.from_numpy(items_idx.reshape(2, 1, 50, 50)).to(DEV)
    zd, ed, wd, gl = z.to(DEV), emb.to(DEV), w.to(DEV), _scalar(G_LOSS)
    full_z, full_e = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=gl)
    # no gradient at z_q: the loss term alone
    gz, ge = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=None, g_loss=gl)
    s = R.step(z.numpy(), emb.numpy(), idx.cpu().numpy(), cfg, None, G_LOSS)
    assert R.err_units(gz.cpu().numpy(), s["grad_z"], s["grad_z_abs"]) <= 2.0
    assert torch.equal(ge, full_e)
    # no gradient at the loss: g_zq passes through, the codebook gets exact zeros
    gz, ge = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=None)
    assert torch.equal(gz, wd)
    assert torch.equal(ge.view(torch.int32), torch.zeros_like(ge).view(torch.int32))
    # neither
    gz, ge = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True)
    assert not gz.any() and not ge.any()
    # skipped outputs
    gz, ge = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=gl, want_grad_emb=False)
    assert ge is None and torch.equal(gz, full_z)
    gz, ge = _lib.vq_backward(zd, ed, idx, DIM, "bchw", BETA, True, g_zq=wd, g_loss=gl, want_grad_z=False)
    assert gz is None and torch.equal(ge, full_e)
    # a short workspace is refused, a missing one too
    L = _lib.lib()
    need = L.vq_backward_workspace_bytes(ITEMS, N, DIM)
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    out_z, out_e = torch.empty_like(zd), torch.empty_like(ed)
    args = (zd.data_ptr(), ed.data_ptr(), idx.data_ptr(), wd.data_ptr(), gl.data_ptr(), out_z.data_ptr(), out_e.data_ptr(), 2, 2500, DIM,
            DIM, N, 0, BETA, 1)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.vq_backward_f32(*args, buf.data_ptr(), need - 1, stream) == WORKSPACE
    assert L.vq_backward_f32(*args, None, need, stream) == WORKSPACE
    assert L.vq_backward_f32(*args, buf.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_z, full_z) and torch.equal(out_e, full_e)
    # no items: nothing but the zeroing of grad_emb
    out_e.fill_(1.0)
    assert L.vq_backward_f32(*args[:7], 0, 2500, DIM, DIM, N, 0, BETA, 1, None, 0, stream) == 0
    torch.cuda.synchronize()
    assert not out_e.any()


# ------------------------------------------------------------------------------------------ 3. module level
def _module(cfg, emb):
    from pit_hip.quantization.vq import VQQuantizer

    m = VQQuantizer(cfg["format"], cfg["n"], cfg["dim"], beta=cfg["beta"], codebook_num=cfg["K"], legacy=cfg["legacy"])
    m.embedding.weight.data = torch.from_numpy(emb)
    return m.to(DEV).train()


def _count_calls(monkeypatch):
    from pit_hip import _lib

    calls = {"vq_quantize_z": [], "vq_backward": [], "vq_argmin": []}
    for name in calls:
        def wrapped(*a, _f=getattr(_lib, name), _n=name, **k):
            calls[_n].append(k)
            return _f(*a, **k)
        monkeypatch.setattr(_lib, name, wrapped)
    return calls


def _step(m, z, w, g_loss):
    zi = z.clone().requires_grad_(True)
    m.embedding.weight.grad = None
    zq, info = m(zi)
    ((zq * w).sum() + g_loss * info["codebook_loss"]).backward()
    return zq, info, zi.grad, m.embedding.weight.grad


@pytest.mark.parametrize("tag", list(R.CASES))
def test_module_train_steps_fixture_and_torch_path_twin(tag, monkeypatch):
    from pit_hip import _lib

    d, cfg = _fixture(), R.CASES[tag]
    bound = _bound(d)
    m = _module(cfg, _emb(d, tag, 0))
    twin = copy.deepcopy(m)
    calls = _count_calls(monkeypatch)
    lr = float(np.float32(d[f"{tag}_lr"]))
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    for it in range(R.STEPS):
        p = f"{tag}_{it}_"
        z, w, g_loss = _dev(d[p + "z"]), _dev(d[p + "w"]), float(d[p + "g_loss"])
        emb_now = m.embedding.weight.detach().cpu().numpy().copy()
        monkeypatch.delenv("GQHIP_TRAIN_FUSED", raising=False)
        before = {k: len(v) for k, v in calls.items()}
        zq, info, gz, ge = _step(m, z, w, g_loss)
        torch.cuda.synchronize()
        assert {k: len(v) - before[k] for k, v in calls.items()} == {"vq_quantize_z": 1, "vq_backward": 1, "vq_argmin": 0}
        assert calls["vq_quantize_z"][-1]["use_cache"] is False          # training: the codebook moves every step
        assert set(info) == {"indices", "codebook_loss"} and "VQTrainFn" in type(info["codebook_loss"].grad_fn).__name__
        assert not info["indices"].requires_grad and info["codebook_loss"].dim() == 0
        assert np.array_equal(info["indices"].cpu().numpy(), d[p + "indices"])      # step 1: from the UPDATED codebook
        if it == 0:
            assert np.array_equal(zq.detach().cpu().numpy(), d[p + "zq"])
            assert R.err_units(gz.cpu().numpy(), d[p + "gz64"], d[p + "gz_abs"]) <= bound
            assert R.err_units(ge.cpu().numpy(), d[p + "ge64"], d[p + "ge_abs"]) <= bound
        else:
            stale, _, _ = _lib.vq_quantize_z(z, _dev(_emb(d, tag, 0)), cfg["dim"], cfg["format"], cfg["beta"], cfg["legacy"])
            assert not torch.equal(stale, info["indices"]), "the fixture's second step does not tell a stale codebook apart"
            np.testing.assert_allclose(zq.detach().cpu().numpy(), d[p + "zq"], rtol=0, atol=1e-5)
        # the codebook this step really started from (after step 0: this module's own update, a rounding away from the fixture's)
        s = R.step(d[p + "z"], emb_now, d[p + "indices"], cfg, d[p + "w"], g_loss)
        ez, ee = R.err_units(gz.cpu().numpy(), s["grad_z"], s["grad_z_abs"]), R.err_units(ge.cpu().numpy(), s["grad_emb"], s["grad_emb_abs"])
        print(f"{tag} step {it}: module grad_z {ez:.2f} grad_emb {ee:.2f} units (bound {bound:.2f})")
        assert ez <= bound and ee <= bound
        assert abs(float(info["codebook_loss"].detach()) - s["loss"]) <= 2e-5 * abs(s["loss"])
        # the op-by-op path of a twin, from the same codebook
        monkeypatch.setenv("GQHIP_TRAIN_FUSED", "0")
        twin.embedding.weight.data.copy_(m.embedding.weight.data)
        before = {k: len(v) for k, v in calls.items()}
        zq_t, info_t, gz_t, ge_t = _step(twin, z, w, g_loss)
        assert len(calls["vq_backward"]) == before["vq_backward"] and len(calls["vq_argmin"]) == before["vq_argmin"] + cfg["K"]
        assert "VQTrainFn" not in type(info_t["codebook_loss"].grad_fn).__name__ and set(info_t) == set(info)
        assert torch.equal(info_t["indices"], info["indices"]) and torch.equal(zq_t, zq)
        assert abs(float(info_t["codebook_loss"].detach()) - float(info["codebook_loss"].detach())) <= 2e-5 * abs(float(info["codebook_loss"].detach()))
        assert R.err_units(gz_t.cpu().numpy(), s["grad_z"], s["grad_z_abs"]) <= bound
        assert R.err_units(ge_t.cpu().numpy(), s["grad_emb"], s["grad_emb_abs"]) <= bound
        opt.step()
    monkeypatch.delenv("GQHIP_TRAIN_FUSED", raising=False)


def test_module_channels_last_frozen_codebook_and_eval_with_autograd(monkeypatch):
    tag = "bchw_d16_crowded"
    d, cfg = _fixture(), R.CASES[tag]
    p = f"{tag}_0_"
    m = _module(cfg, _emb(d, tag, 0))
    z, w, g_loss = _dev(d[p + "z"]), _dev(d[p + "w"]), float(d[p + "g_loss"])
    zq, info, gz, ge = _step(m, z, w, g_loss)
    ge = ge.clone()
    # channels_last: the same values, and -- every sum keeps its order -- the same bits
    zq_c, info_c, gz_c, ge_c = _step(m, z.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last), g_loss)
    assert zq_c.shape == zq.shape and torch.equal(zq_c, zq) and torch.equal(info_c["indices"], info["indices"])
    assert torch.equal(info_c["codebook_loss"], info["codebook_loss"])
    assert torch.equal(gz_c, gz) and torch.equal(ge_c, ge)
    # a frozen codebook: no weight.grad, the same z.grad
    m.embedding.weight.requires_grad_(False)
    _, _, gz_f, ge_f = _step(m, z, w, g_loss)
    assert ge_f is None and m.embedding.weight.grad is None and torch.equal(gz_f, gz)
    m.embedding.weight.requires_grad_(True)
    # eval() with z.requires_grad: still the fused route, now with the codebook cache
    calls = _count_calls(monkeypatch)
    m.eval()
    zq_e, info_e, gz_e, ge_e = _step(m, z, w, g_loss)
    assert [len(calls[k]) for k in ("vq_quantize_z", "vq_backward", "vq_argmin")] == [1, 1, 0]
    assert calls["vq_quantize_z"][-1]["use_cache"] is True
    assert torch.equal(zq_e, zq) and torch.equal(info_e["indices"], info["indices"]) and torch.equal(gz_e, gz) and torch.equal(ge_e, ge)
    # and without autograd nothing changes: the one-call eval forward
    with torch.no_grad():
        zq_n, info_n = m(z)
    assert torch.equal(zq_n, zq) and torch.equal(info_n["indices"], info["indices"]) and not zq_n.requires_grad
    assert len(calls["vq_backward"]) == 1
