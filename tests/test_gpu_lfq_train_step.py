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
Every case prints its figures before asserting.

Sections 8 and 9 launch the kernel variants g25's widths (1, 5, 8, 12, 16) leave out, from g28 (R.VARIANT_CASES: every other width,
nc > 1 above d = 8, non-square forward grids; tests/golden/make_golden_train_variants.py).  Bounds of section 8:
  a scalar   2 x max(the case's own ref_err, the largest ref_err of that scalar over g25's cases): at these widths the reference's
             fp32 error on a scalar is often far below one unit (commit_loss 0.00 at d = 15), which no kernel that rounds its
             result once can meet -- the rule of test_rows_across_several_reduction_blocks.
  grad_x     2 x the case's own grad_x_ref_err, with all three gradients (against the reference's fp64 autograd) and with g_aux alone
             (against the checker; the sum of |terms| then holds only the entropy terms, so a wrong batch term cannot hide behind
             |w|).  The gate is loose: the reference's dense fp32 route is off by 30 .. 21 000 units.  It catches a wrong mapping
             (10^5 .. 10^7 units), not a loss of digits; section 9 checks the same variants without a tolerance.
  avg        per entry 2^-24 avg (d (max |s| + 7) + 35) + 2^-120, s = 400 x: a factor sigma(+-s) carries |s| + 6 units (the rounding
             of s through exp; expf, 1 + e, the division), each of a row's d factors one more for its product, the 32-row fp32 sum
             32, the partial tile, the division by R and the cast 3; 2^-120 for products below fp32's normal range.
Measured (profiles/r27/gpu_new_tests.txt): scalars 0.00 .. 0.83 units, grad_x 1.4 .. 5.0, with g_aux alone 2.1 .. 7.4, avg at most
0.023 of its bound; section 9 without a differing bit."""
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


# ------------------------------------------------------------------------------------------ 8. every kernel variant (g28)
@pytest.fixture(scope="module")
def g28():
    return dict(np.load(os.path.join(G, "g28_lfq_train_variants.npz")))


def _vx(fix, tag, cfg, key="x"):
    """(the float32 numbers, the device tensor in the case's memory format)"""
    a = R.variant(fix, tag, key).astype(np.float32)
    t = _dev(a)
    return a, t.contiguous(memory_format=torch.channels_last) if cfg.get("channels_last") else t


def _avg_bound(x, cfg, a64):
    """|avg - fp64| per entry (module docstring): 2^-24 avg (d (max |s| + 7) + 35) + 2^-120."""
    return R.U * a64 * (cfg["d"] * (400.0 * float(np.abs(x).max()) + 7.0) + 35.0) + 2.0 ** -120


@pytest.mark.parametrize("tag", list(R.VARIANT_CASES))
def test_variant_scalars_avg_and_grad_x_against_fp64(tag, g28):
    from pit_hip import _lib

    cfg = R.VARIANT_CASES[tag]
    (xn, x), (wn, w) = _vx(g28, tag, cfg), _vx(g28, tag, cfg, "w")
    xv, layout = _lib_view(x, cfg)
    wv = _lib_view(w, cfg)[0]
    ga, gc = float(g28[f"{tag}_g_aux"]), float(g28[f"{tag}_g_commit"])
    full, aux = R.factorised64(xn, cfg, wn, ga, gc), R.factorised64(xn, cfg, None, ga, 0.0)
    ws = _lib.LfqTrainWorkspace()
    q, ind, avg, scal = _lib.lfq_train(xv, cfg["nc"], cfg["d"], layout, 1.0, 1.0, ws)
    g_full = _lib.lfq_backward(xv, avg, cfg["nc"], cfg["d"], layout, 1.0, 1.0, g_q=wv, g_aux=_scalar(ga), g_commit=_scalar(gc), ws=ws)
    g_aux = _lib.lfq_backward(xv, avg, cfg["nc"], cfg["d"], layout, 1.0, 1.0, g_aux=_scalar(ga), ws=ws)
    scal, avg = scal.cpu().numpy(), avg.cpu().numpy().astype(np.float64)
    g25 = _fixture()
    errs, bounds = {}, {}
    for k, name in enumerate(R.SCALARS):
        errs[name] = R.err_units(scal[k], float(g28[f"{tag}_{name}64"]), float(g28[f"{tag}_{name}_abs"]))
        bounds[name] = 2.0 * max(float(g28[f"{tag}_{name}_ref_err"]), max(float(g25[f"{t}_{name}_ref_err"]) for t in R.CASES))
    errs["grad_x"] = _units(_home(g_full, x, cfg), R.variant(g28, tag, "grad_x64"), full["grad_x_abs"])
    errs["grad_x_aux_only"] = _units(_home(g_aux, x, cfg), aux["grad_x"], aux["grad_x_abs"])
    bounds["grad_x"] = bounds["grad_x_aux_only"] = 2.0 * float(g28[f"{tag}_grad_x_ref_err"])
    a64 = full["avg"].reshape(-1)
    avg_rel = float((np.abs(avg - a64) / _avg_bound(xn, cfg, a64)).max())
    for name, e in errs.items():
        print(f"{tag}: {name} {e:.2f} units (bound {bounds[name]:.2f})")
    print(f"{tag}: avg {avg_rel:.4f} of its bound, sum(avg) - 1 = {avg.sum() - 1.0:.3e}")
    assert np.array_equal(ind.cpu().numpy().reshape(-1), g28[f"{tag}_indices"].reshape(-1))
    assert np.array_equal(_home(q, x, cfg), xn + (np.where(xn > 0, 1.0, -1.0).astype(np.float32) - xn))
    assert avg_rel <= 1.0 and abs(avg.sum() - 1.0) <= 1e-5
    for name, e in errs.items():
        assert e <= bounds[name], (name, e)


# ------------------------------------------------------------------------------------------ 9. the same variants, exactly
def _one_hot(cfg):
    """x in {+1, -1}: row r spells code[r] (bit i = channel i of the row).  The codes 0, 2^d - 1, every 2^i, every complement of
    one, then seeded random ones.  Returns (codes, x in the case's shape, w)."""
    d, rows = cfg["d"], int(np.prod(cfg["shape"])) // cfg["d"]
    last = (1 << d) - 1
    rng = np.random.default_rng(900 + d)
    codes = [0, last] + [1 << i for i in range(d)] + [last ^ (1 << i) for i in range(d)]
    codes = np.array(codes + rng.integers(0, 1 << d, rows - len(codes)).tolist(), np.int64)
    x = np.where((codes[:, None] >> np.arange(d)[None, :]) & 1, 1.0, -1.0).astype(np.float32).reshape(cfg["shape"])
    return codes, x, rng.standard_normal(cfg["shape"]).astype(np.float32)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("tag", [t for t, c in R.VARIANT_CASES.items() if c["format"] == "blc"])
def test_one_hot_rows_give_exact_counts_and_pass_the_gradient_through(tag):
    """exp(-400) is 0 in fp32: every probability is exactly 0 or 1 and every table one-hot, so avg[j] = fl32(count_j / R) and, with
    g_q = w, grad_x = w, bit for bit: x - q = 0, p q = 0 and every factor (bit ? q_i : -p_i) of the batch term is an exact zero.
    Anything read from an unwritten LDS slab or a padded table entry shows as a non-zero or a NaN."""
    from pit_hip import _lib

    cfg = R.VARIANT_CASES[tag]
    codes, x, w = _one_hot(cfg)
    rows = codes.size
    want = (np.bincount(codes, minlength=1 << cfg["d"]).astype(np.float64) / rows).astype(np.float32)
    xd, wd = _dev(x), _dev(w)
    ws = _lib.LfqTrainWorkspace()
    q, _, avg, scal = _lib.lfq_train(xd, cfg["nc"], cfg["d"], "blc", 1.0, 1.0, ws)
    gx = _lib.lfq_backward(xd, avg, cfg["nc"], cfg["d"], "blc", 1.0, 1.0, g_q=wd, g_aux=_scalar(R.G_AUX), g_commit=_scalar(R.G_COMMIT),
                           ws=ws)
    scal = scal.cpu().numpy()
    bad_avg, bad_g = int((_bits(avg) != want.view(np.int32)).sum()), int((_bits(gx) != w.view(np.int32)).sum())
    print(f"{tag}: {rows} rows on {int((want > 0).sum())} codes: avg differs at {bad_avg} of {want.size}, grad_x at {bad_g} of {w.size}; "
          f"per_sample_entropy {scal[1]!r}, commit_loss {scal[3]!r}")
    assert bad_avg == 0 and bad_g == 0
    assert np.array_equal(q.cpu().numpy(), x) and scal[1] == 0.0 and scal[3] == 0.0


def test_regrouping_the_same_memory_changes_no_bit(g28):
    """d = 13: [1, 75, 52] with nc = 4 and [1, 300, 13] with nc = 1 are the same rows in the same order with the same R and P C, so
    avg and grad_x are bit-equal and the 52-bit indices are the 13-bit ones of the four rows in a row."""
    from pit_hip import _lib

    outs = {}
    for tag in ("blc_d13", "blc_d13x4"):
        cfg = R.VARIANT_CASES[tag]
        (_, x), (_, w) = _vx(g28, tag, cfg), _vx(g28, tag, cfg, "w")
        ws = _lib.LfqTrainWorkspace()
        _, ind, avg, _ = _lib.lfq_train(x, cfg["nc"], 13, "blc", 1.0, 1.0, ws)
        gx = _lib.lfq_backward(x, avg, cfg["nc"], 13, "blc", 1.0, 1.0, g_q=w, g_aux=_scalar(R.G_AUX), g_commit=_scalar(R.G_COMMIT), ws=ws)
        outs[tag] = (avg, gx.reshape(-1), ind.cpu().numpy().reshape(-1))
    (a1, g1, i1), (a4, g4, i4) = outs["blc_d13"], outs["blc_d13x4"]
    i1 = i1.reshape(75, 4)
    print(f"avg differs at {int((_bits(a1) != _bits(a4)).sum())}, grad_x at {int((_bits(g1) != _bits(g4)).sum())} of {g1.numel()}")
    assert np.array_equal(_bits(a1), _bits(a4)) and np.array_equal(_bits(g1), _bits(g4))
    assert np.array_equal(i4, (i1[:, 0] << 39) | (i1[:, 1] << 26) | (i1[:, 2] << 13) | i1[:, 3])


@pytest.mark.parametrize("tag", ["blc_d11x2", "blc_d13", "blc_d15"])
def test_variant_runs_are_bitwise_equal_whatever_the_workspace_holds(tag, g28):
    from pit_hip import _lib

    cfg = R.VARIANT_CASES[tag]
    (xn, x), (_, w) = _vx(g28, tag, cfg), _vx(g28, tag, cfg, "w")
    runs = []
    for fill in (None, 0xFF, 0):                                          # the workspace's contents are don't-care on entry
        ws = _lib.LfqTrainWorkspace()
        if fill is not None:
            ws.get(xn.size // cfg["d"], cfg["d"], torch.device(DEV))
            ws.buf.fill_(fill)
        _, _, avg, scal = _lib.lfq_train(x, cfg["nc"], cfg["d"], "blc", 1.0, 1.0, ws)
        gx = _lib.lfq_backward(x, avg, cfg["nc"], cfg["d"], "blc", 1.0, 1.0, g_q=w, g_aux=_scalar(R.G_AUX), g_commit=_scalar(R.G_COMMIT),
                               ws=ws)
        runs.append((avg.clone(), scal.clone(), gx.clone()))
    print(tag, "scalars", runs[0][1].tolist())
    assert all(np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)) for a, b, c in zip(*runs))


def test_module_route_at_d13_nc4_channels_last(g28):
    """LFQQuantizer("bchw", 2^13, 4) on an NHWC tensor: through the autograd function, x.grad in x's strides and equal to the direct
    library call bit for bit."""
    from pit_hip import _lib

    tag = "bchw_d13x4_cl"
    cfg = R.VARIANT_CASES[tag]
    m = _module(cfg).train()
    x = _vx(g28, tag, cfg)[1].requires_grad_(True)
    w = _vx(g28, tag, cfg, "w")[1]
    q, info = m(x)
    assert "LFQTrainFn" in type(info["entropy_aux_loss"].grad_fn).__name__
    ((q * w).sum() + R.G_AUX * info["entropy_aux_loss"] + R.G_COMMIT * info["commit_loss"]).backward()
    xv, layout = _lib_view(x.detach(), cfg)
    ws = _lib.LfqTrainWorkspace()
    ql, il, avg, scal = _lib.lfq_train(xv, 4, 13, layout, 1.0, 1.0, ws)
    gl = _lib.lfq_backward(xv, avg, 4, 13, layout, 1.0, 1.0, g_q=_lib_view(w, cfg)[0], g_aux=_scalar(R.G_AUX), g_commit=_scalar(R.G_COMMIT),
                           ws=ws)
    print(f"{tag}: x strides {x.stride()} grad strides {x.grad.stride()} max |grad| {float(x.grad.abs().max()):.4f}")
    assert layout == "blc" and not x.is_contiguous() and x.grad.shape == x.shape and x.grad.stride() == x.stride()
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), _home(gl, x.detach(), cfg).view(np.int32))
    assert np.array_equal(q.detach().cpu().numpy(), _home(ql, x.detach(), cfg))
    assert np.array_equal(info["indices"].cpu().numpy().reshape(-1), il.cpu().numpy().reshape(-1))
    assert [float(info[k].detach()) for k in R.SCALARS] == scal.tolist()
