"""-m gpu: LFQQuantizer's fused train step -- lfq_train_f32 (the forward: quantized, indices, the batch-average distribution as a
GEMM of per-row probability tables, the four scalars), lfq_backward_f32 and the autograd.Function that puts them behind
LFQQuantizer -- against the fixture captured from the reference's CPU autograd in fp32 and fp64 (g25:
tests/golden/make_golden_lfq_train.py) and the fp64 restatement tests/lfq_train_ref.py (proven on the CPU by
tests/test_lfq_train_host.py).

Bounds: per case and per output, 2 x the error the reference's own fp32 run shows against its fp64 run ({name}_ref_err in the
fixture, in units of 2^-24 x sum of |terms|); the factor 2 covers the different summation order over rows.  One allowance on top, an
absolute 2^-100 per element of grad_x: exp(-|400 x|) below fp32's normal range (|x| > 0.218) is flushed, and what it would have
contributed -- at most 2^-126 times 400 |s| |G| / R < 2^26 -- exists in the fp64 run (down to |x| = 1.77) but not in fp32.  It matters
only where no other term reaches the element (an absent upstream gradient of ``quantized`` on saturated inputs).
Every case prints its figures before asserting."""
import itertools
import os

import numpy as np
import pytest
import torch

import lfq_train_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
FLUSH = 2.0 ** -100


def _fixture():
    return np.load(os.path.join(G, "g25_lfq_train_step.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def _units(got, want, want_abs):
    """R.err_units with the flush allowance of the module docstring."""
    got, want, want_abs = (np.asarray(a, np.float64) for a in (got, want, want_abs))
    live = want_abs > 0
    assert np.all(got[~live] == 0.0), "an element without terms is not exactly zero"
    err = np.maximum(np.abs(got - want) - FLUSH, 0.0)
    unit = R.U * want_abs                                                 # (zero where the sum of |terms| itself is subnormal)
    ratio = np.divide(err, unit, out=np.where(err > 0, np.inf, 0.0), where=unit > 0)
    return float(ratio[live].max()) if live.any() else 0.0


def _module(cfg, cls=None):
    from pit_hip.quantization.lfq import LFQQuantizer

    return (cls or LFQQuantizer)(cfg["format"], 1 << cfg["d"], cfg["nc"], sample_minimization_weight=cfg.get("w_s", 1.0),
                                 batch_maximization_weight=cfg.get("w_b", 1.0)).to(DEV)


def _x(d, tag, cfg):
    x = _dev(d[f"{tag}_x"].astype(np.float32))
    return x.contiguous(memory_format=torch.channels_last) if cfg.get("channels_last") else x


def _lib_view(x, cfg):
    """(x as the library takes it, layout): a channels_last [B, C, h, w] is the "blc" view of the same memory."""
    if cfg["format"] == "bchw" and not x.is_contiguous():
        b, c, h, w = x.shape
        return x.permute(0, 2, 3, 1).reshape(b, h * w, c), "blc"
    return x, cfg["format"]


def _home(t, x, cfg):
    """A library-layout tensor back in the shape of the module's x, as numpy."""
    if cfg["format"] == "bchw" and not x.is_contiguous():
        b, c, h, w = x.shape
        t = t.view(b, h, w, c).permute(0, 3, 1, 2)
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. bit-exact outputs
@pytest.mark.parametrize("tag", list(R.CASES))
def test_quantized_and_indices_are_bit_exact(tag, monkeypatch):
    d, cfg = _fixture(), R.CASES[tag]
    m, x = _module(cfg).train(), _x(d, tag, cfg)
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "1")
    qf, inf = m(x)
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "0")
    qt, int_ = m(x)
    torch.cuda.synchronize()
    print(f"{tag}: quantized {tuple(qf.shape)} indices {tuple(inf['indices'].shape)}")
    assert set(inf) == set(int_) and all(inf[k].shape == int_[k].shape and inf[k].dtype == int_[k].dtype for k in inf)
    assert qf.shape == qt.shape == x.shape
    assert np.array_equal(qf.cpu().numpy(), d[f"{tag}_quantized"]) and torch.equal(qf, qt)
    assert np.array_equal(inf["indices"].cpu().numpy(), d[f"{tag}_indices"]) and torch.equal(inf["indices"], int_["indices"])


# ------------------------------------------------------------------------------------------ 2. accuracy against fp64
@pytest.mark.parametrize("tag", list(R.CASES))
def test_scalars_and_grad_x_against_fp64(tag):
    from pit_hip import _lib

    d, cfg = _fixture(), R.CASES[tag]
    x = _x(d, tag, cfg)
    xv, layout = _lib_view(x, cfg)
    w = _dev(d[f"{tag}_w"].astype(np.float32))
    wv = _lib_view(w.contiguous(memory_format=torch.channels_last) if cfg.get("channels_last") else w, cfg)[0]
    ws_, wb_ = cfg.get("w_s", 1.0), cfg.get("w_b", 1.0)
    ws = _lib.LfqTrainWorkspace()
    _, _, avg, scal = _lib.lfq_train(xv, cfg["nc"], cfg["d"], layout, ws_, wb_, ws)
    scal = scal.cpu().numpy()
    for k, name in enumerate(R.SCALARS):
        ref = float(d[f"{tag}_{name}_ref_err"])
        got = R.err_units(scal[k], float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        print(f"{tag}: {name} {scal[k]!r} vs fp64 {float(d[f'{tag}_{name}64'])!r}: {got:.2f} units (reference {ref:.2f})")
    bound = 2.0 * float(d[f"{tag}_grad_x_ref_err"])
    ga, gc = float(d[f"{tag}_g_aux"]), float(d[f"{tag}_g_commit"])
    xn, wn = d[f"{tag}_x"].astype(np.float32), d[f"{tag}_w"].astype(np.float32)
    errs = {}
    for has_q, has_a, has_c in itertools.product((True, False), repeat=3):
        gx = _lib.lfq_backward(xv, avg, cfg["nc"], cfg["d"], layout, ws_, wb_, g_q=wv if has_q else None,
                               g_aux=_scalar(ga) if has_a else None, g_commit=_scalar(gc) if has_c else None, ws=ws)
        got = _home(gx, x, cfg)
        if has_q and has_a and has_c:
            want, want_abs = d[f"{tag}_grad_x64"], d[f"{tag}_grad_x_abs"]
        else:
            s = R.factorised64(xn, cfg, wn if has_q else None, ga if has_a else 0.0, gc if has_c else 0.0)
            want, want_abs = s["grad_x"], s["grad_x_abs"]
        errs[(has_q, has_a, has_c)] = _units(got, want, want_abs)
        print(f"{tag}: grad_x with (g_q, g_aux, g_commit) = {(has_q, has_a, has_c)}: {errs[(has_q, has_a, has_c)]:.2f} units "
              f"(reference with all three {float(d[f'{tag}_grad_x_ref_err']):.2f}, bound {bound:.2f})")
        if not (has_q or has_a or has_c):
            assert not got.any()                                          # absent gradients contribute exact zeros
    for k, name in enumerate(R.SCALARS):
        got = R.err_units(scal[k], float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        assert got <= 2.0 * float(d[f"{tag}_{name}_ref_err"]), (name, got)
    assert max(errs.values()) <= bound, errs


# ------------------------------------------------------------------------------------------ 3. several reduction blocks with a tail
ROWS = 4099
_big = {}


def _multi(dbits):
    """x [1, 4099, d] ~ 0.02 N(0, 1) (float16-exact), w, and the fp64 step, computed once per d."""
    if dbits not in _big:
        g = torch.Generator().manual_seed(40 + dbits)
        cfg = dict(format="blc", d=dbits, nc=1)
        x = (0.02 * torch.randn(1, ROWS, dbits, generator=g)).half().float()
        w = torch.randn(1, ROWS, dbits, generator=g)
        s = R.factorised64(x.numpy(), cfg, w.numpy(), R.G_AUX, R.G_COMMIT)
        _big[dbits] = (cfg, x, w, s, R.dense64(x.numpy(), cfg) if dbits == 8 else s)
    return _big[dbits]


@pytest.mark.parametrize("dbits,like", [(8, "bchw_256x2"), (16, "blc_65536x1")])
def test_rows_across_several_reduction_blocks(dbits, like):
    """R = 4099 = 16 chunks of 256 rows and a tail of 3.  d = 8: scalars against the dense [R, N] formula; d = 16: against the
    factorised one.  No reference run exists at this size, so the bounds are the fixture's: for a scalar 2 x the largest error the
    reference's fp32 run shows on any fixture case, for grad_x 2 x its error on the fixture case with the same d."""
    from pit_hip import _lib

    d = _fixture()
    cfg, x, w, s, sc = _multi(dbits)
    ws = _lib.LfqTrainWorkspace()
    xd = x.to(DEV)
    _, _, avg, scal = _lib.lfq_train(xd, 1, dbits, "blc", 1.0, 1.0, ws)
    gx = _lib.lfq_backward(xd, avg, 1, dbits, "blc", 1.0, 1.0, g_q=w.to(DEV), g_aux=_scalar(R.G_AUX), g_commit=_scalar(R.G_COMMIT),
                           ws=ws)
    scal, avg = scal.cpu().numpy(), avg.cpu().numpy().astype(np.float64)
    print(f"d {dbits}: sum(avg) - 1 = {avg.sum() - 1.0:.3e}, max |avg - fp64| = {np.abs(avg - s['avg'].reshape(-1)).max():.3e}")
    errs = {name: R.err_units(scal[k], sc[name], sc[name + "_abs"]) for k, name in enumerate(R.SCALARS)}
    errs["grad_x"] = _units(gx.cpu().numpy(), s["grad_x"], s["grad_x_abs"])
    bounds = {name: 2.0 * max(float(d[f"{tag}_{name}_ref_err"]) for tag in R.CASES) for name in R.SCALARS}
    bounds["grad_x"] = 2.0 * float(d[f"{like}_grad_x_ref_err"])
    for name, e in errs.items():
        print(f"d {dbits}: {name} {e:.2f} units (bound {bounds[name]:.2f})")
    assert abs(avg.sum() - 1.0) <= 1e-5
    for name, e in errs.items():
        assert e <= bounds[name], (name, e)


def test_runs_are_bitwise_equal_whatever_the_workspace_holds():
    from pit_hip import _lib

    cfg, x, w, _, _ = _multi(16)
    xd, wd = x.to(DEV), w.to(DEV)
    runs = []
    for fill in (None, 0xFF, 0):                                          # the workspace's contents are don't-care on entry
        ws = _lib.LfqTrainWorkspace()
        if fill is not None:
            ws.get(ROWS, 16, torch.device(DEV))
            ws.buf.fill_(fill)
        _, _, avg, scal = _lib.lfq_train(xd, 1, 16, "blc", 1.0, 1.0, ws)
        gx = _lib.lfq_backward(xd, avg, 1, 16, "blc", 1.0, 1.0, g_q=wd, g_aux=_scalar(R.G_AUX), g_commit=_scalar(R.G_COMMIT), ws=ws)
        runs.append((avg.clone(), scal.clone(), gx.clone()))
    print("scalars", runs[0][1].tolist())
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(*runs))


# ------------------------------------------------------------------------------------------ 4. the matrix never exists
def test_flagship_step_stays_far_below_the_logits_matrix():
    """LFQQuantizer("bchw", 65536, 1) at z = [16, 16, 32, 32]: one copy of the [16 384, 65 536] fp32 logits is 4.29 GB; forward +
    backward may raise the peak by less than a sixteenth of that."""
    from pit_hip.quantization.lfq import LFQQuantizer

    m = LFQQuantizer("bchw", 65536, 1).to(DEV).train()
    g = torch.Generator().manual_seed(3)
    x = (0.02 * torch.randn(16, 16, 32, 32, generator=g)).to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    q, info = m(x)
    (q.sum() + info["entropy_aux_loss"] + info["commit_loss"]).backward()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    limit = 16384 * 65536 * 4 // 16
    print(f"peak grew by {grew / 1e6:.1f} MB (limit {limit / 1e6:.1f} MB); codebook_entropy {float(info['codebook_entropy']):.4f} "
          f"of {16 * np.log(2):.4f}")
    assert 0 < grew < limit
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


# ------------------------------------------------------------------------------------------ 5. no host synchronisation
def test_the_step_never_synchronises_with_the_host():
    d, tag = _fixture(), "bchw_256x2"
    cfg = R.CASES[tag]
    m = _module(cfg).train()
    x, w = _x(d, tag, cfg), _dev(d[f"{tag}_w"].astype(np.float32))
    for strict in (False, True):                                          # the first step sizes the workspace
        xl = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error" if strict else "default")
        try:
            q, info = m(xl)
            ((q * w).sum() + info["entropy_aux_loss"] + info["commit_loss"]).backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    print("step under sync debug mode 'error': ok, grad_fn", type(info["entropy_aux_loss"].grad_fn).__name__)
    assert "LFQTrainFn" in type(info["entropy_aux_loss"].grad_fn).__name__
    assert not info["per_sample_entropy"].requires_grad and not info["codebook_entropy"].requires_grad
    assert not info["indices"].requires_grad and xl.grad is not None


# ------------------------------------------------------------------------------------------ 6. routing
def test_eval_and_bsq_keep_their_routes(monkeypatch):
    from pit_hip.quantization.bsq import BSQQuantizer

    d, tag = _fixture(), "bchw_256x2"
    cfg = R.CASES[tag]
    x = _x(d, tag, cfg)
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("GQHIP_TRAIN_FUSED", flag)
        m = _module(cfg).eval()
        q, info = m(x)
        assert all(float(info[k]) == 0.0 for k in R.SCALARS)
        xb = x.clone().requires_grad_(True)
        b = _module(dict(format="bchw", d=1, nc=16), BSQQuantizer).train()
        qb, ib = b(xb)
        (qb.sum() + ib["entropy_aux_loss"]).backward()
        assert "LFQTrainFn" not in type(ib["entropy_aux_loss"].grad_fn).__name__
        outs[flag] = (q, info["indices"], qb.detach(), ib["indices"], ib["entropy_aux_loss"].detach(), ib["per_sample_entropy"],
                      ib["codebook_entropy"], xb.grad)
    print("eval and BSQ train outputs equal under GQHIP_TRAIN_FUSED=1 and 0:", [torch.equal(a, b) for a, b in zip(outs["1"], outs["0"])])
    assert all(torch.equal(a, b) for a, b in zip(outs["1"], outs["0"]))


# ------------------------------------------------------------------------------------------ 7. the module's backward
@pytest.mark.parametrize("tag", ["bchw_256x2", "blc_65536x1", "bchw_4096x1_cl"])
def test_module_backward_reaches_x_in_its_own_layout(tag):
    from pit_hip import _lib

    d, cfg = _fixture(), R.CASES[tag]
    m = _module(cfg).train()
    x = _x(d, tag, cfg).requires_grad_(True)
    w = _dev(d[f"{tag}_w"].astype(np.float32))
    q, info = m(x)
    ((q * w).sum() + info["entropy_aux_loss"] + info["commit_loss"]).backward()
    xv, layout = _lib_view(x.detach(), cfg)
    wv = _lib_view(w.contiguous(memory_format=torch.channels_last) if cfg.get("channels_last") else w, cfg)[0]
    ws = _lib.LfqTrainWorkspace()
    ql, il, avg, scal = _lib.lfq_train(xv, cfg["nc"], cfg["d"], layout, 1.0, 1.0, ws)
    gl = _lib.lfq_backward(xv, avg, cfg["nc"], cfg["d"], layout, 1.0, 1.0, g_q=wv, g_aux=_scalar(1.0), g_commit=_scalar(1.0), ws=ws)
    print(f"{tag}: x strides {x.stride()} grad strides {x.grad.stride()} max |grad| {float(x.grad.abs().max()):.4f}")
    assert x.grad.shape == x.shape and x.grad.stride() == x.stride()
    assert np.array_equal(x.grad.cpu().numpy(), _home(gl, x.detach(), cfg))
    assert np.array_equal(q.detach().cpu().numpy(), _home(ql, x.detach(), cfg))
    assert [float(info[k].detach()) for k in R.SCALARS] == scal.tolist()
