"""The fused LPIPS comparison head (csrc/lpips_head.h) on the GPU: accuracy against fp64 over the case table in both layouts,
edge cases, autograd behaviour, and the LPIPS / loss modules on the fused route against the reference's run (g31).

Bounds.  Head: 2 x max(the reference's own fp32-vs-fp64 error for that case and output (g30), 1 unit), unit = 2^-24 x sum |terms|
(tests/lpips_ref.py); shapes the fixture does not hold (kernel variants the table misses, the multi-block shape) are held to
2 units.  Modules: the fused route's error against g31's fp64 values is at most 2 x max(the op-by-op route's error on the same
device, one fp32 rounding of the largest magnitude).

Measured on an MI355X (profiles/r29/gpu_new_tests.txt): see MEASURED below."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu

MEASURED = """out 0.001-0.71 unit, grad_f1 (and grad_f0) 0.80-0.993 unit over the 90 head runs (the table in both layouts, 16-byte
aligned and not, the extra kernel variants, the zero pixels, the dropout masks); the reference's own fp32 run: out 0.02-4.1,
grad_f1 2.9-10913 (g30).  Modules against g31: the fused route's error is 0.14-1.2 x the op-by-op route's on the same device."""

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# kernel variants the table does not reach: "blc" with 4 and 8 lanes per pixel, "bchw" with 16-byte loads at C <= 128
EXTRA_SHAPES = [(2, 16, 3, 5), (2, 32, 5, 3), (2, 128, 4, 6), R.MULTI_BLOCK_SHAPE]


@pytest.fixture(scope="module")
def L():
    from pit_hip import _lib

    return _lib


@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(G, "g30_lpips_head.npz"))


@pytest.fixture(scope="module")
def g31():
    return np.load(os.path.join(G, "g31_lpips_loss.npz"))


def _dev(a, offset=0):
    """a numpy array on the device; ``offset`` floats off the allocation's 16-byte alignment"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if offset:
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
        buf[offset:].copy_(t.reshape(-1))
        t = buf[offset:].view(t.shape)
    return t


def _to_layout(a, layout):
    """logical [B, C, H, W] numpy -> the library's array"""
    if a is None:
        return None
    B, C = a.shape[:2]
    return a.reshape(B, C, -1) if layout == "bchw" else a.reshape(B, C, -1).transpose(0, 2, 1)


def _from_layout(t, shape, layout):
    B, C, H, W = shape
    t = t.cpu()
    return t.reshape(shape) if layout == "bchw" else t.reshape(B, H * W, C).permute(0, 2, 1).reshape(shape)


def _run(L, f0, f1, w, keep, g, layout, offset=0, scale=R.KEEP_SCALE):
    shape = f0.shape
    d0, d1, dk = (_dev(_to_layout(a, layout), offset) for a in (f0, f1, keep))
    dw, dg = _dev(w, offset), _dev(g)
    out = L.lpips_head(d0, d1, dw, layout, dk, scale)
    grad = L.lpips_head_backward(d0, d1, dw, dg, layout, dk, scale)
    torch.cuda.synchronize()
    return out.cpu(), _from_layout(grad, shape, layout)


def _check_case(L, shape, near, masked, bounds, offsets=(0,)):
    f0, f1, w, keep, g = R.case_inputs(shape, near, masked)
    want_o, want_g, uo, ug = R.head_ref(f0, f1, w, keep, R.KEEP_SCALE, g)
    worst = [0.0, 0.0]
    for layout in ("bchw", "blc"):
        for offset in offsets:
            out, grad = _run(L, f0, f1, w, keep, g, layout, offset)
            eo, eg = R.err_units(out, want_o, uo), R.err_units(grad, want_g, ug)
            print(f"{R.case_id(shape, near, masked)} {layout} +{offset}: out {eo:.3f} unit (bound {bounds[0]:.1f}), "
                  f"grad_f1 {eg:.3f} unit (bound {bounds[1]:.1f})")
            assert torch.isfinite(grad).all()
            assert eo <= bounds[0] and eg <= bounds[1], (shape, near, masked, layout, offset, eo, eg)
            worst = [max(worst[0], eo), max(worst[1], eg)]
    return worst


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_over_the_table(L, g30, shape):
    for near in (False, True):
        for masked in (False, True):
            cid = R.case_id(shape, near, masked).replace("/", ".")
            bounds = [2 * max(float(g30[cid + "." + k]), 1.0) for k in ("out_ref_err", "grad_ref_err")]
            # off the 16-byte alignment once per shape: the 4-byte kernels of either layout
            _check_case(L, shape, near, masked, bounds, offsets=(0, 1) if near and not masked else (0,))


@pytest.mark.parametrize("shape", EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_of_the_other_kernel_variants(L, shape):
    for masked in (False, True):
        _check_case(L, shape, True, masked, [2.0, 2.0])


def test_all_zero_pixels_give_the_limit(L):
    shape = (2, 64, 5, 7)
    f0, f1, w, _, g = R.case_inputs(shape, True, False)
    f1[0, :, 1, 2] = 0
    f0[0, :, 3, 3] = 0
    f0[1, :, 0, 0] = f1[1, :, 0, 0] = 0
    want_o, want_g, uo, ug = R.head_ref(f0, f1, w, None, 1.0, g)
    # at f1's zero pixel the gradient is the r1 t_j term alone: (g / HW) 1e10 (-2 w_j f0_j / n0)
    n0 = np.sqrt((f0[0, :, 1, 2].astype(np.float64) ** 2).sum())
    term = float(g[0]) / 35.0 * 1e10 * (-2.0 * w.astype(np.float64) * f0[0, :, 1, 2].astype(np.float64) / (n0 + 1e-10))
    assert np.allclose(want_g[0, :, 1, 2].numpy(), term, rtol=1e-12, atol=0)
    for layout in ("bchw", "blc"):
        out, grad = _run(L, f0, f1, w, None, g, layout, scale=1.0)
        eo, eg = R.err_units(out, want_o, uo), R.err_units(grad, want_g, ug)
        print(f"zero pixels {layout}: out {eo:.3f} unit, grad_f1 {eg:.3f} unit")
        assert torch.isfinite(grad).all() and eo <= 2 and eg <= 2
        assert float(grad[1, :, 0, 0].abs().max()) == 0.0          # both zero: u = 0


def test_equal_features_and_an_empty_mask_give_exact_zeros(L):
    for shape in ((2, 64, 5, 7), (2, 128, 4, 6), (2, 3, 4, 5)):
        f0, f1, w, _, g = R.case_inputs(shape, True, False)
        for layout in ("bchw", "blc"):
            out, grad = _run(L, f0, f0.copy(), w, None, g, layout, scale=1.0)
            assert float(out.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0
            out, grad = _run(L, f0, f1, w, np.zeros(shape, np.uint8), g, layout)
            assert float(out.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0


def test_empty_batch(L):
    f = torch.empty(0, 64, 9, device="cuda")
    assert L.lpips_head(f, f, torch.ones(64, device="cuda"), "bchw").shape == (0,)


def test_autograd_symmetry_and_reproducibility(L):
    from pit_hip.modules.lpips.loss.lpips import LpipsHeadFn

    shape = R.MULTI_BLOCK_SHAPE
    f0n, f1n, w, keep, g = R.case_inputs(shape, True, True)
    for layout in ("bchw", "blc"):
        f0, f1 = (_dev(_to_layout(a, layout)).requires_grad_() for a in (f0n, f1n))
        dk, dw, dg = _dev(_to_layout(keep, layout)), _dev(w), _dev(g)
        cfg = (layout, R.KEEP_SCALE, L.LpipsHeadWorkspace())
        out = LpipsHeadFn.apply(f0, f1, dw, dk, cfg)
        assert type(out.grad_fn).__name__ == "LpipsHeadFnBackward"
        a0, a1 = torch.autograd.grad(out, (f0, f1), dg, retain_graph=True)
        b0, b1 = torch.autograd.grad(out, (f0, f1), dg, retain_graph=True)
        assert torch.equal(a0, b0) and torch.equal(a1, b1)                      # re-entrant, same bits
        (only1,) = torch.autograd.grad(out, f1, dg, retain_graph=True)          # a gradient for one of the two alone
        assert torch.equal(only1, a1)
        assert torch.equal(a0, L.lpips_head_backward(f1.detach(), f0.detach(), dw, dg, layout, dk, R.KEEP_SCALE))   # the swapped call
        assert torch.equal(out.detach(), LpipsHeadFn.apply(f0, f1, dw, dk, cfg).detach())
        want_o, want_g, uo, ug = R.head_ref(f1n, f0n, w, keep, R.KEEP_SCALE, g)     # f0's gradient against fp64
        eg = R.err_units(_from_layout(a0, shape, layout), want_g, ug)
        print(f"grad_f0 {layout}: {eg:.3f} unit")
        assert eg <= 2


def _fused_node(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if type(n).__name__ == "LpipsHeadFnBackward":
            return n
        todo += [f for f, _ in n.next_functions]
    return None


def test_dropout_in_training_mode_reproduces_the_restatement(L):
    from pit_hip.modules.lpips.loss.lpips import LPIPS

    torch.manual_seed(5)
    m = LPIPS(pretrained=False).cuda().train()        # the quirk: train() switches the `lin` dropouts on
    shape = (2, 64, 9, 11)
    f0n, f1n, _, _, g = R.case_inputs(shape, True, False)
    for fmt in (torch.contiguous_format, torch.channels_last):
        f0 = _dev(f0n).contiguous(memory_format=fmt)
        f1 = _dev(f1n).contiguous(memory_format=fmt).requires_grad_()
        out = m._head(f0, f1, m.lin0)
        node = _fused_node(out)
        assert node is not None and out.shape == (2, 1, 1, 1)
        keep = node.saved_tensors[3]
        assert keep.dtype == torch.uint8 and 0.4 < float(keep.float().mean()) < 0.6
        keep_l = keep.reshape(shape) if fmt == torch.contiguous_format else keep.reshape(2, 9, 11, 64).permute(0, 3, 1, 2)
        (grad,) = torch.autograd.grad(out.reshape(-1), f1, _dev(g))
        want_o, want_g, uo, ug = R.head_ref(f0n, f1n, m.lin0.model[-1].weight.detach().reshape(-1).cpu().numpy(),
                                            keep_l.cpu().numpy(), 2.0, g)
        eo, eg = R.err_units(out.detach().reshape(-1).cpu(), want_o, uo), R.err_units(grad.cpu(), want_g, ug)
        print(f"dropout {fmt}: out {eo:.3f} unit, grad_f1 {eg:.3f} unit")
        assert eo <= 2 and eg <= 2
    out = m.eval()._head(f0, f1, m.lin0)                  # eval(): no mask is drawn
    assert _fused_node(out).saved_tensors[3] is None


def test_modules_on_the_fused_route_against_the_reference(g31, monkeypatch):
    """LPIPS alone, then GeneralLPIPSWithDiscriminator with optimizer_idx 0 and 1, on the op-by-op route (GQHIP_TRAIN_FUSED=0) and
    on the fused route, both on this device (the VGG convolutions are the vendor library's on both sides: only the head differs).
    The vendor library is held to its deterministic algorithms for both runs: left free it answers the same call with one of a few
    results from run to run (opt0.loss errors of 1.6e-5 .. 1.4e-4 on either route, the adaptive weight amplifies them), and a bound
    taken from one draw was then applied to another -- the parent's code failed its own test in about one run in three that way
    (profiles/r30/lpips_module_test_noise.txt).  With it both routes see the same convolutions, which is what the bound assumes."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    errs = {}

    def record(name, got, f32, f64):
        errs[name] = float(np.abs(np.asarray(got, np.float64) - np.asarray(f64, np.float64)).max())

    def against_op_by_op(name, got, f32, f64):
        f64 = np.asarray(f64, np.float64)
        err = float(np.abs(np.asarray(got, np.float64) - f64).max())
        floor = R.U24 * float(np.abs(f64).max())
        print(f"{name}: fused err {err:.3e}, op-by-op err {errs[name]:.3e}, floor {floor:.3e}")
        assert err <= 2 * max(errs[name], floor), name

    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "0")
    nodes = R.run_loss_against_fixture(g31, torch.device("cuda"), check=record)
    assert all(_fused_node(v) is None for v in nodes.values())
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "1")
    nodes = R.run_loss_against_fixture(g31, torch.device("cuda"), check=against_op_by_op)
    assert _fused_node(nodes["lpips"]) is not None and _fused_node(nodes["opt0.p_loss"]) is not None
