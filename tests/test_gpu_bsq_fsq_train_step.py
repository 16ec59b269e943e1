"""-m gpu: the fused train steps of BSQQuantizer (bsq_train_f32, bsq_backward_f32, _BSQTrainFn) and FSQQuantizer (fsq_train_f32,
fsq_backward_f32, _FSQTrainFn), opted into with GQHIP_BSQ_TRAIN_FUSED=1 / GQHIP_FSQ_TRAIN_FUSED=1 -- against the fixtures captured
from the reference's CPU autograd in fp32 and fp64 (g26, g27: tests/golden/make_golden_bsq_fsq_train.py) and the fp64 restatement
tests/bsq_fsq_train_ref.py (proven on the CPU by tests/test_bsq_fsq_train_host.py).

Bounds: per case and per output, 2 x max(the error the reference's own fp32 run shows against its fp64 run -- {name}_ref_err in the
fixture, in units of 2^-24 x sum of |terms| --, 1 unit); the factor 2 covers a different summation order over rows, the 1-unit floor
the one rounding of u to fp32 that the fp64 run does not have.  Every case prints its figures before asserting.

Section 12 launches the "blc" kernel pairs g26's widths leave out (<16, 3> at d = 9 .. 12, the partly idle last chunk of <16, 2> and
<16, 4>) and "bchw" at d = 9 and 15, from g29 (R.BSQ_VARIANT_CASES; tests/golden/make_golden_train_variants.py), under the same rule
``_bound``: the reference's own error there is 2.2 .. 5.7 units on grad_x and 0.03 .. 3.6 on the scalars, a gate of 4.4 .. 11.5 and
2 .. 7.1 units.  Measured (profiles/r27/gpu_new_tests.txt): grad_x 0.60 .. 0.84 units, with g_aux alone 0.37 .. 0.77, scalars 0.00 ..
0.78."""
import itertools
import os

import numpy as np
import pytest
import torch

import bsq_fsq_train_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def bsq():
    return dict(np.load(os.path.join(G, "g26_bsq_train_step.npz")))


@pytest.fixture(scope="module")
def fsq():
    return dict(np.load(os.path.join(G, "g27_fsq_train_step.npz")))


@pytest.fixture
def opt_in(monkeypatch):
    monkeypatch.delenv("GQHIP_TRAIN_FUSED", raising=False)
    monkeypatch.setenv("GQHIP_BSQ_TRAIN_FUSED", "1")
    monkeypatch.setenv("GQHIP_FSQ_TRAIN_FUSED", "1")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def _bound(ref_err):
    return 2.0 * max(float(ref_err), 1.0)


def _made_by(t, name):
    """True when ``name`` is the autograd node of t, or stands behind the views (a channels_last output is a permuted view) of it."""
    fn = t.grad_fn
    while fn is not None and name not in type(fn).__name__ and len(fn.next_functions) == 1:
        fn = fn.next_functions[0][0]
    return fn is not None and name in type(fn).__name__


def _bsq_module(cfg):
    from pit_hip.quantization.bsq import BSQQuantizer

    return BSQQuantizer(cfg["format"], 1 << cfg["d"], 16, sample_minimization_weight=cfg.get("w_s", 1.0),
                        batch_maximization_weight=cfg.get("w_b", 1.0)).to(DEV)


def _fsq_module(cfg):
    from pit_hip.quantization.fsq import FSQQuantizer

    return FSQQuantizer(cfg["levels"], cfg["format"]).to(DEV)


def _in(a, cfg):
    x = _dev(np.asarray(a, np.float32))
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
        t = t.view(b, h, w, -1).permute(0, 3, 1, 2)
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1, 2. indices and quantized
@pytest.mark.parametrize("tag", list(R.BSQ_CASES) + ["underflow"])
def test_bsq_indices_and_quantized(tag, bsq, opt_in):
    cfg = R.BSQ_UNDERFLOW if tag == "underflow" else R.BSQ_CASES[tag]
    m = _bsq_module(cfg).train()
    x = _in(bsq[f"{tag}_x"], cfg)
    with torch.no_grad():
        q, info = m(x)
    q, want = q.cpu().numpy(), bsq[f"{tag}_quantized"]
    qs = float(np.float32(1.0 / np.sqrt(16 * cfg["d"])))
    e_fix, e_one = np.abs(q - want).max() / (R.U * qs), np.abs(np.abs(q) - qs).max() / (R.U * qs)
    print(f"{tag}: indices equal {np.array_equal(info['indices'].cpu().numpy(), bsq[f'{tag}_indices'])}; quantized: "
          f"{e_fix:.2f} units of 2^-24 q_scale from the fixture (bound 6), {e_one:.2f} from +-q_scale (bound 3)")
    assert info["indices"].dtype == torch.int64 and info["indices"].shape == bsq[f"{tag}_indices"].shape
    assert np.array_equal(info["indices"].cpu().numpy(), bsq[f"{tag}_indices"])
    assert q.shape == want.shape and e_fix <= 6.0 and e_one <= 3.0
    assert np.all(np.abs(np.abs(want) - qs) <= 3.0 * R.U * qs)
    if tag == "underflow":
        assert int(info["indices"][0, 1, 0]) == 1 << 15                  # the positive element whose fp32 quotient is 0 gets bit 0


# ------------------------------------------------------------------------------------------ 3, 4. scalars and grad_x
@pytest.mark.parametrize("tag", list(R.BSQ_CASES))
def test_bsq_scalars_and_grad_x_within_the_references_own_error(tag, bsq):
    from pit_hip import _lib

    d, cfg = bsq, R.BSQ_CASES[tag]
    x, w = _in(d[f"{tag}_x"], cfg), _in(d[f"{tag}_w"], cfg)
    xv, layout = _lib_view(x, cfg)
    wv = _lib_view(w, cfg)[0]
    ws_, wb_ = cfg.get("w_s", 1.0), cfg.get("w_b", 1.0)
    ws = _lib.BsqTrainWorkspace()
    _, _, avg, scal = _lib.bsq_train(xv, cfg["d"], layout, ws_, wb_, ws)
    scal = scal.cpu().numpy()
    for i, name in enumerate(R.SCALARS):
        e = R.err_units(scal[i], float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        print(f"{tag}: {name} {e:.2f} units (reference fp32 {float(d[f'{tag}_{name}_ref_err']):.2f}, bound "
              f"{_bound(d[f'{tag}_{name}_ref_err']):.2f})")
    x_np, w_np = d[f"{tag}_x"].astype(np.float32), d[f"{tag}_w"].astype(np.float32)
    errs = {}
    for has_q, has_aux in itertools.product((True, False), repeat=2):
        gx = _lib.bsq_backward(xv, avg, cfg["d"], layout, ws_, wb_, g_q=wv if has_q else None,
                               g_aux=_scalar(R.G_AUX) if has_aux else None, ws=ws)
        got = _home(gx, x, cfg)
        if has_q and has_aux:
            want, want_abs = d[f"{tag}_grad_x64"], d[f"{tag}_grad_x_abs"]
        else:
            s = R.bsq64(x_np, cfg, w_np if has_q else None, R.G_AUX if has_aux else 0.0)
            want, want_abs = s["grad_x"], s["grad_x_abs"]
        if not has_q and not has_aux:
            assert np.all(got == 0.0)
        errs[(has_q, has_aux)] = R.err_units(got, want, want_abs)
        print(f"{tag}: grad_x g_q {has_q} g_aux {has_aux}: {errs[(has_q, has_aux)]:.2f} units (reference fp32 "
              f"{float(d[f'{tag}_grad_x_ref_err']):.2f}, bound {_bound(d[f'{tag}_grad_x_ref_err']):.2f})")
    a64 = R.bsq64(x_np, cfg)["avg"]
    assert np.all(np.abs(avg.cpu().numpy() - a64) <= R.U * a64 + 1e-45)                     # each entry rounded once
    for i, name in enumerate(R.SCALARS):
        e = R.err_units(scal[i], float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"]))
        assert e <= _bound(d[f"{tag}_{name}_ref_err"]), (name, e)
    for k, e in errs.items():
        assert e <= _bound(d[f"{tag}_grad_x_ref_err"]), (k, e)


# ------------------------------------------------------------------------------------------ 5. several reduction blocks
MULTI = {"blc_d1_4099": dict(format="blc", d=1, shape=(1, 4099, 16)), "bchw_d4_4099": dict(format="bchw", d=4, shape=(1, 64, 4099)),
         "bchw_d16_67": dict(format="bchw", d=16, shape=(1, 256, 67)), "blc_d16_67": dict(format="blc", d=16, shape=(1, 67, 256)),
         "blc_d7_300": dict(format="blc", d=7, shape=(2, 150, 112)),
         # more tiles than partial records (1024): a block walks two of them
         "blc_d3_16500": dict(format="blc", d=3, shape=(1, 16500, 48)), "bchw_d1_262500": dict(format="bchw", d=1, shape=(1, 16, 262500))}


@pytest.mark.parametrize("tag", list(MULTI))
def test_bsq_several_reduction_blocks_against_the_checker(tag, bsq):
    """No reference run at these sizes: the check is against the fp64 checker, each output's bound the largest of its fixture
    bounds.  (bchw always makes a second pass over x; blc keeps a row's C / 4 chunks in the registers of its 16 lanes, d = 16 too.)"""
    from pit_hip import _lib

    cfg = MULTI[tag]
    g = torch.Generator().manual_seed(55)
    x = torch.randn(cfg["shape"], generator=g).half().float()
    w = torch.randn(cfg["shape"], generator=g).half().float()
    s = R.bsq64(x.numpy(), cfg, w.numpy(), R.G_AUX)
    bounds = {n: max(_bound(bsq[f"{t}_{n}_ref_err"]) for t in R.BSQ_CASES) for n in R.SCALARS + ("grad_x",)}
    ws = _lib.BsqTrainWorkspace()
    xd = x.to(DEV)
    q, ind, avg, scal = _lib.bsq_train(xd, cfg["d"], cfg["format"], 1.0, 1.0, ws)
    gx = _lib.bsq_backward(xd, avg, cfg["d"], cfg["format"], 1.0, 1.0, g_q=w.to(DEV), g_aux=_scalar(R.G_AUX), ws=ws)
    scal = scal.cpu().numpy()
    errs = {name: R.err_units(scal[i], s[name], s[name + "_abs"]) for i, name in enumerate(R.SCALARS)}
    errs["grad_x"] = R.err_units(gx.cpu().numpy(), s["grad_x"], s["grad_x_abs"])
    for name, e in errs.items():
        print(f"{tag}: {name} {e:.2f} units (bound {bounds[name]:.2f})")
    assert np.array_equal(ind.cpu().numpy(), s["indices"])
    qs = float(np.float32(1.0 / np.sqrt(16 * cfg["d"])))
    assert np.all(np.abs(q.cpu().numpy() - np.where(s["u"] > 0, qs, -qs)) <= 3.0 * R.U * qs)
    assert np.all(np.abs(avg.cpu().numpy() - s["avg"]) <= R.U * s["avg"] + 1e-45)
    for name, e in errs.items():
        assert e <= bounds[name], (name, e)


# ------------------------------------------------------------------------------------------ 6, 7. FSQ
@pytest.mark.parametrize("tag", list(R.FSQ_CASES))
def test_fsq_forward_and_backward(tag, fsq, opt_in):
    f, cfg = fsq, R.FSQ_CASES[tag]
    m = _fsq_module(cfg).train()
    z = _in(f[f"{tag}_z"], cfg).requires_grad_(True)
    w = _in(f[f"{tag}_w"], cfg)
    zhat, info = m(z)
    assert _made_by(zhat, "FSQTrainFn")
    (zhat * w).sum().backward()
    got, want = info["indices"].cpu().numpy(), f[f"{tag}_indices"]
    assert got.dtype == np.int32 and got.shape == want.shape and set(info) == {"indices", "bits"}
    diff = got != want
    n = len(cfg["levels"])
    s = R.fsq64(f[f"{tag}_z"].astype(np.float32), cfg["levels"], cfg["format"])
    hw = R.to_pos(s["r"], cfg["format"])[1](np.tile(s["half_width"], (s["r"].size // n, 1)))
    same = ~np.repeat(diff, n, axis=1 if cfg["format"] == "bchw" else 2)
    ez = (np.abs(zhat.detach().cpu().numpy() - f[f"{tag}_zhat"]) / (2.0 ** -23 * (np.abs(s["r"]) + 1) / hw))[same].max()
    e = R.err_units(z.grad.cpu().numpy(), f[f"{tag}_grad_z64"], f[f"{tag}_grad_z_abs"])
    print(f"{tag}: indices differ at {int(diff.sum())} of {diff.size}; zhat {ez:.2f} of its bound; grad_z {e:.2f} units (reference fp32 "
          f"{float(f[f'{tag}_grad_z_ref_err']):.2f}, bound {_bound(f[f'{tag}_grad_z_ref_err']):.2f})")
    assert np.all(f[f"{tag}_margin"][diff] < 1e-5) and diff.mean() < 0.01
    assert ez <= 1.0
    assert abs(float(info["bits"]) - float(np.sum(np.log2(cfg["levels"])) * z[0].numel())) < 1e-2
    assert z.grad.shape == z.shape and z.grad.stride() == z.stride()
    assert e <= _bound(f[f"{tag}_grad_z_ref_err"]), e


# ------------------------------------------------------------------------------------------ 8. bit-reproducibility
def test_bsq_runs_are_bitwise_equal_whatever_the_workspace_holds():
    from pit_hip import _lib

    g = torch.Generator().manual_seed(56)
    x = torch.randn(3, 700, 48, generator=g).to(DEV)
    w = torch.randn(3, 700, 48, generator=g).to(DEV)
    runs = []
    for fill in (None, 0xFF, 0):                                          # the workspace's contents are don't-care on entry
        ws = _lib.BsqTrainWorkspace()
        if fill is not None:
            ws.get(3 * 700, 3, torch.device(DEV))
            ws.buf.fill_(fill)
        q, _, avg, scal = _lib.bsq_train(x, 3, "blc", 1.0, 1.0, ws)
        gx = _lib.bsq_backward(x, avg, 3, "blc", 1.0, 1.0, g_q=w, g_aux=_scalar(R.G_AUX), ws=ws)
        runs.append((avg.clone(), scal.clone(), q.clone(), gx.clone()))
    print("scalars", runs[0][1].tolist())
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(*runs))


# ------------------------------------------------------------------------------------------ 9. no host synchronisation
@pytest.mark.parametrize("family", ["bsq", "fsq"])
def test_the_step_never_synchronises_with_the_host(family, bsq, fsq, opt_in):
    if family == "bsq":
        tag, cfg = "bchw_d1", R.BSQ_CASES["bchw_d1"]
        m, x, w = _bsq_module(cfg).train(), _in(bsq[f"{tag}_x"], cfg), _in(bsq[f"{tag}_w"], cfg)
    else:
        tag, cfg = "bchw_6", R.FSQ_CASES["bchw_6"]
        m, x, w = _fsq_module(cfg).train(), _in(fsq[f"{tag}_z"], cfg), _in(fsq[f"{tag}_w"], cfg)
    for strict in (False, True):                                          # the first step sizes the workspace
        xl = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error" if strict else "default")
        try:
            q, info = m(xl)
            loss = (q * w).sum()
            (loss + info["entropy_aux_loss"] if family == "bsq" else loss).backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    assert xl.grad is not None and not info["indices"].requires_grad
    if family == "bsq":
        assert not info["per_sample_entropy"].requires_grad and not info["codebook_entropy"].requires_grad


# ------------------------------------------------------------------------------------------ 10. routing
def _step(m, x, w, aux):
    xl = x.clone().requires_grad_(True)
    q, info = m(xl)
    ((q * w).sum() + info["entropy_aux_loss"] if aux else (q * w).sum()).backward()
    return q, info, xl.grad


def test_routing(bsq, fsq, monkeypatch):
    bc, fc = R.BSQ_CASES["bchw_d1"], R.FSQ_CASES["bchw_6"]
    bx, bw = _in(bsq["bchw_d1_x"], bc), _in(bsq["bchw_d1_w"], bc)
    fx, fw = _in(fsq["bchw_6_z"], fc), _in(fsq["bchw_6_w"], fc)
    outs = {}
    for name, env in (("unset", {}), ("opt_in", dict(GQHIP_BSQ_TRAIN_FUSED="1", GQHIP_FSQ_TRAIN_FUSED="1")),
                      ("main_off", dict(GQHIP_BSQ_TRAIN_FUSED="1", GQHIP_FSQ_TRAIN_FUSED="1", GQHIP_TRAIN_FUSED="0"))):
        for var in ("GQHIP_TRAIN_FUSED", "GQHIP_BSQ_TRAIN_FUSED", "GQHIP_FSQ_TRAIN_FUSED"):
            monkeypatch.delenv(var, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        q, info, gx = _step(_bsq_module(bc).train(), bx, bw, True)
        zh, finfo, gz = _step(_fsq_module(fc).train(), fx, fw, False)
        fused = name == "opt_in"
        assert ("BSQTrainFn" in type(info["entropy_aux_loss"].grad_fn).__name__) == fused
        assert ("FSQTrainFn" in type(zh.grad_fn).__name__) == fused
        with torch.no_grad():
            qe, ie = _bsq_module(bc).eval()(bx)
            ze, fe = _fsq_module(fc).eval()(fx)
        assert all(float(ie[k]) == 0.0 for k in R.SCALARS)
        outs[name] = (q.detach(), info["indices"], info["entropy_aux_loss"].detach(), info["per_sample_entropy"], info["codebook_entropy"],
                      gx, zh.detach(), finfo["indices"], gz, qe, ie["indices"], ze, fe["indices"])
    print("unset vs GQHIP_TRAIN_FUSED=0:", [torch.equal(a, b) for a, b in zip(outs["unset"], outs["main_off"])])
    assert all(torch.equal(a, b) for a, b in zip(outs["unset"], outs["main_off"]))
    assert all(torch.equal(a, b) for a, b in zip(outs["unset"][9:], outs["opt_in"][9:]))          # eval() is unchanged either way
    assert torch.equal(outs["unset"][1], outs["opt_in"][1]) and torch.equal(outs["unset"][7], outs["opt_in"][7])


# ------------------------------------------------------------------------------------------ 11. layout
@pytest.mark.parametrize("family", ["bsq", "fsq"])
def test_channels_last_input_gets_its_gradient_in_channels_last_memory(family, bsq, fsq, opt_in):
    if family == "bsq":
        cfg = R.BSQ_CASES["bchw_d1"]
        m, x, w = _bsq_module(cfg).train(), _in(bsq["bchw_d1_x"], cfg), _in(bsq["bchw_d1_w"], cfg)
    else:
        cfg = R.FSQ_CASES["bchw_6"]
        m, x, w = _fsq_module(cfg).train(), _in(fsq["bchw_6_z"], cfg), _in(fsq["bchw_6_w"], cfg)
    q0, i0, g0 = _step(m, x, w, family == "bsq")
    xc = x.contiguous(memory_format=torch.channels_last)
    ptr = xc.data_ptr()
    q1, i1, g1 = _step(m, xc, w.contiguous(memory_format=torch.channels_last), family == "bsq")
    print(f"{family}: NCHW grad strides {g0.stride()}, channels_last grad strides {g1.stride()}")
    assert g0.is_contiguous() and g1.is_contiguous(memory_format=torch.channels_last) and not g1.is_contiguous()
    assert q1.is_contiguous(memory_format=torch.channels_last) and xc.data_ptr() == ptr
    assert torch.equal(g0, g1) and torch.equal(q0, q1) and torch.equal(i0["indices"], i1["indices"])


# ------------------------------------------------------------------------------------------ 12. every "blc" kernel pair (g29)
@pytest.fixture(scope="module")
def g29():
    return dict(np.load(os.path.join(G, "g29_bsq_train_variants.npz")))


@pytest.mark.parametrize("tag", list(R.BSQ_VARIANT_CASES))
def test_bsq_variant_against_fp64(tag, g29):
    """indices bit for bit, quantized within its three roundings, avg rounded once, the scalars and grad_x (with both gradients,
    and with g_aux alone) within _bound of the case's own reference error.  g29 holds no grad_x64: it is the checker's, which its
    generator held against the reference's fp64 autograd."""
    from pit_hip import _lib

    d, cfg = g29, R.BSQ_VARIANT_CASES[tag]
    x, w = _in(d[f"{tag}_x"], cfg), _in(d[f"{tag}_w"], cfg)
    xv, layout = _lib_view(x, cfg)
    wv = _lib_view(w, cfg)[0]
    x_np, w_np = d[f"{tag}_x"].astype(np.float32), d[f"{tag}_w"].astype(np.float32)
    full, aux = R.bsq64(x_np, cfg, w_np, R.G_AUX), R.bsq64(x_np, cfg, None, R.G_AUX)
    ws = _lib.BsqTrainWorkspace()
    q, ind, avg, scal = _lib.bsq_train(xv, cfg["d"], layout, 1.0, 1.0, ws)
    g_full = _lib.bsq_backward(xv, avg, cfg["d"], layout, 1.0, 1.0, g_q=wv, g_aux=_scalar(R.G_AUX), ws=ws)
    g_aux = _lib.bsq_backward(xv, avg, cfg["d"], layout, 1.0, 1.0, g_aux=_scalar(R.G_AUX), ws=ws)
    scal = scal.cpu().numpy()
    errs = {name: R.err_units(scal[i], float(d[f"{tag}_{name}64"]), float(d[f"{tag}_{name}_abs"])) for i, name in enumerate(R.SCALARS)}
    bounds = {name: _bound(d[f"{tag}_{name}_ref_err"]) for name in R.SCALARS}
    errs["grad_x"] = R.err_units(_home(g_full, x, cfg), full["grad_x"], full["grad_x_abs"])
    errs["grad_x_aux_only"] = R.err_units(_home(g_aux, x, cfg), aux["grad_x"], aux["grad_x_abs"])
    bounds["grad_x"] = bounds["grad_x_aux_only"] = _bound(d[f"{tag}_grad_x_ref_err"])
    for name, e in errs.items():
        print(f"{tag}: {name} {e:.2f} units (bound {bounds[name]:.2f})")
    assert layout == ("bchw" if tag in ("bchw_d9", "bchw_d15") else "blc")
    assert np.array_equal(_home(ind, x, cfg), d[f"{tag}_indices"])
    qs = float(np.float32(1.0 / np.sqrt(16 * cfg["d"])))
    assert np.all(np.abs(_home(q, x, cfg) - np.where(full["u"] > 0, qs, -qs)) <= 3.0 * R.U * qs)
    assert np.all(np.abs(avg.cpu().numpy() - full["avg"]) <= R.U * full["avg"] + 1e-45)          # each entry rounded once
    for name, e in errs.items():
        assert e <= bounds[name], (name, e)


@pytest.mark.parametrize("tag", ["blc_d10", "blc_d14"])
def test_bsq_variant_runs_are_bitwise_equal_whatever_the_workspace_holds(tag, g29):
    from pit_hip import _lib

    cfg = R.BSQ_VARIANT_CASES[tag]
    x, w = _in(g29[f"{tag}_x"], cfg), _in(g29[f"{tag}_w"], cfg)
    runs = []
    for fill in (None, 0xFF, 0):                                          # the workspace's contents are don't-care on entry
        ws = _lib.BsqTrainWorkspace()
        if fill is not None:
            ws.get(x.shape[0] * x.shape[1], cfg["d"], torch.device(DEV))
            ws.buf.fill_(fill)
        q, _, avg, scal = _lib.bsq_train(x, cfg["d"], "blc", 1.0, 1.0, ws)
        gx = _lib.bsq_backward(x, avg, cfg["d"], "blc", 1.0, 1.0, g_q=w, g_aux=_scalar(R.G_AUX), ws=ws)
        runs.append((avg.clone(), scal.clone(), q.clone(), gx.clone()))
    print(tag, "scalars", runs[0][1].tolist())
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(*runs))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])


def test_bsq_module_route_at_d10_channels_last(g29, opt_in):
    """BSQQuantizer("bchw", 2^10, 16) on an NHWC tensor takes the <16, 3> "blc" pair through the autograd function; x.grad has x's
    strides and equals the direct library call bit for bit."""
    from pit_hip import _lib

    tag = "bchw_d10_cl"
    cfg = R.BSQ_VARIANT_CASES[tag]
    m = _bsq_module(cfg).train()
    x, w = _in(g29[f"{tag}_x"], cfg).requires_grad_(True), _in(g29[f"{tag}_w"], cfg)
    q, info = m(x)
    assert _made_by(q, "BSQTrainFn") and "BSQTrainFn" in type(info["entropy_aux_loss"].grad_fn).__name__
    ((q * w).sum() + R.G_AUX * info["entropy_aux_loss"]).backward()
    xv, layout = _lib_view(x.detach(), cfg)
    ws = _lib.BsqTrainWorkspace()
    ql, il, avg, scal = _lib.bsq_train(xv, 10, layout, 1.0, 1.0, ws)
    gl = _lib.bsq_backward(xv, avg, 10, layout, 1.0, 1.0, g_q=_lib_view(w, cfg)[0], g_aux=_scalar(R.G_AUX), ws=ws)
    print(f"{tag}: x strides {x.stride()} grad strides {x.grad.stride()} max |grad| {float(x.grad.abs().max()):.4f}")
    assert layout == "blc" and not x.is_contiguous() and x.grad.shape == x.shape and x.grad.stride() == x.stride()
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), _home(gl, x.detach(), cfg).view(np.int32))
    assert np.array_equal(q.detach().cpu().numpy(), _home(ql, x.detach(), cfg))
    assert np.array_equal(info["indices"].cpu().numpy(), _home(il, x.detach(), cfg))
    assert [float(info[k].detach()) for k in R.SCALARS] == scal.tolist()
