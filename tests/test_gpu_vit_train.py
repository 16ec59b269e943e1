"""-m gpu: training the BSQ-ViT on the kernel route on a real MI355X -- the forward with log-sum-exp and the fused attention
backward (csrc/gq_attn_bwd.h, _lib.mha_fwd_lse / _lib.mha_bwd) against fp64 autograd, their exact zeros, determinism, the module
under autograd against the reference's gradients (g23), which calls enter the kernels, and whole-block checkpointing.

The gate.  For each of dq, dk, dv and each head, err = max|g - g64| / max|g64| (g64: torch's fp64 autograd of the explicit
softmax(q k^T / sqrt(d)) v on the device, itself checked against tests/attn_bwd_ref.py here); where max|g64| is exactly 0 (one
key: dq = dk = 0) the denominator is 1.  The gate is err_hip <= MARGIN * err_torch32, err_torch32 the same quantity for torch's fp32
autograd through the same explicit formula, computed in the same test: both routes sum the same fp32 products over the same
lengths in different orders, so neither should be systematically worse; the margin is for order noise only.

MARGIN is 4, not 2: err is a maximum over a head's elements and the ratio of two such maxima scatters.  Measured on an MI355X
(profiles/r14/gpu_new_tests.txt), worst head ratio per case: 0.71 ... 1.78 on the nine shapes except dq at (2, 3, 31): 2.23
(err_hip 5.3e-7 against 2.9e-7 over the case); q = 0: 1.39; operand scaling 1.38; the peaked softmax 1.00 on dq and dk, 1.59 on dv;
the four parameter gradients of the module 0.66 ... 1.03."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_bwd_ref

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
MARGIN = 4.0      # the issue's 2, raised to its allowed ceiling: measured ratios in the module docstring
SHAPES = [(2, 3, 1), (2, 3, 31), (2, 3, 33), (2, 3, 63), (2, 3, 65), (1, 2, 128), (1, 2, 129), (1, 1, 333), (2, 2, 300)]
NAMES = ("transformer.resblocks.0.attn.in_proj_weight", "transformer.resblocks.0.attn.in_proj_bias",
         "transformer.resblocks.0.ln_1.weight", "positional_embedding")


def _randn(shape, seed):
    return torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _explicit(qkv, dout, H, dtype):
    """autograd of the explicit softmax(q k^T / sqrt(d)) v in `dtype` on the device: (out [B, L, E], lse [B, H, L], dqkv)"""
    t = qkv.detach().to(dtype).requires_grad_(True)
    B, L, E3 = t.shape
    E = E3 // 3
    q, k, v = (t[..., i * E:(i + 1) * E].reshape(B, L, H, E // H).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(E // H)
    out = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, E)
    out.backward(dout.to(dtype))
    return out.detach(), torch.logsumexp(s.detach(), dim=-1), t.grad


@functools.lru_cache(maxsize=None)
def _case(B, H, L):
    """the seeded operands of a shape and its references, computed once and shared (never modified)"""
    qkv, dout = _randn((B, L, 3 * H * 64), B * 1000 + H * 10 + L), _randn((B, L, H * 64), 77 + L)
    return (qkv, dout) + _refs(qkv, dout, H)


def _refs(qkv, dout, H):
    _, lse64, g64 = _explicit(qkv, dout, H, torch.float64)
    _, _, g32 = _explicit(qkv, dout, H, torch.float32)
    return lse64, g64, g32


def _errs(g, g64, H):
    """err per (block of dq | dk | dv, head): [3, H]"""
    B, L, E3 = g64.shape
    d = E3 // 3 // H
    diff = (g.double() - g64).abs().reshape(B, L, 3, H, d).amax(dim=(0, 1, 4))
    ref = g64.abs().reshape(B, L, 3, H, d).amax(dim=(0, 1, 4))
    return diff / torch.where(ref > 0, ref, torch.ones_like(ref))


def _gate(label, g, g64, g32, H):
    eh, et = _errs(g, g64, H), _errs(g32, g64, H)
    for i, n in enumerate(("dq", "dk", "dv")):
        ratio = float((eh[i] / et[i].clamp_min(1e-300)).max()) if float(eh[i].max()) > 0 else 0.0
        print(f"{label} {n}: err_hip {float(eh[i].max()):.3e}  err_torch32 {float(et[i].max()):.3e}  worst head ratio {ratio:.2f}")
    assert bool(torch.isfinite(g).all()), label
    assert bool((eh <= MARGIN * et).all()), label


def _run(qkv, dout, H):
    from pit_hip import _lib

    out, lse = _lib.mha_fwd_lse(qkv, H)
    return out, lse, _lib.mha_bwd(qkv, out, lse, dout, H)


def _heads(qkv, H):
    """views of q, k, v as [B, L, H, d]"""
    B, L, E3 = qkv.shape
    E = E3 // 3
    return [qkv[..., i * E:(i + 1) * E].view(B, L, H, E // H) for i in range(3)]


# ---- 1. forward with lse -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,L", SHAPES)
def test_forward_with_lse(B, H, L):
    from pit_hip import _lib

    qkv, dout, lse64, g64, g32 = _case(B, H, L)
    out, lse = _lib.mha_fwd_lse(qkv, H)
    assert out.shape == (B, L, H * 64) and lse.shape == (B, H, L)
    assert torch.equal(out, _lib.mha_fwd(qkv, H))
    err = float((lse.double() * math.log(2.0) - lse64).abs().max())
    print(f"B{B} H{H} L{L}: max|lse ln 2 - lse64| = {err:.3e}")
    assert err <= 1e-5


def test_fp64_reference_on_the_device_is_attn_bwd_ref():
    qkv, dout, lse64, g64, _ = _case(2, 3, 65)
    want = attn_bwd_ref.mha_bwd_from_qkv(qkv.cpu().numpy(), dout.cpu().numpy(), 3)
    assert np.abs(g64.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(lse64.cpu().numpy() - attn_bwd_ref.lse_from_qkv(qkv.cpu().numpy(), 3)).max() <= 1e-12 * float(lse64.abs().max())


# ---- 2. backward values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,L", SHAPES)
def test_backward_against_fp64(B, H, L):
    qkv, dout, _, g64, g32 = _case(B, H, L)
    _, _, g = _run(qkv, dout, H)
    assert g.shape == qkv.shape
    _gate(f"B{B} H{H} L{L}", g, g64, g32, H)


# ---- 3. operand ranges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [-12, 8])
def test_backward_operand_scaling(f):
    """q x 2^f, k x 2^-f: the logits are unchanged, dq and dk span 2^-+f."""
    B, H, L = 2, 2, 300
    qkv = _case(B, H, L)[0].clone()
    dout = _case(B, H, L)[1]
    q, k, v = _heads(qkv, H)
    q.mul_(2.0 ** f)
    k.mul_(2.0 ** -f)
    _, g64, g32 = _refs(qkv, dout, H)
    _gate(f"q x 2^{f}, k x 2^{-f}", _run(qkv, dout, H)[2], g64, g32, H)


def test_backward_peaked_softmax():
    """The input of test_gpu_vit.py's peaked case at L 300: every query is 7 x one key, P is near one-hot, dP - delta cancels.
    The true dq and dk are ~1e-6 of dv here (the softmax is saturated) and err is relative to THEM: what passes is a backward
    whose delta is sum_j P_j dP_j of the P and dP it multiplies with, and whose P is normalised by its own row sum (with
    delta = dout . out the kernel stood at 7.07 x torch's error on dq and dk, with P = exp2(s2 - lse2) alone at 24 x on dv)."""
    B, H, L = 2, 4, 300
    qkv = _randn((B, L, 3 * H * 64), 9)
    q, k, v = _heads(qkv, H)
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(1)).to(DEV)
    q.copy_(7.0 * k[:, perm])
    dout = _randn((B, L, H * 64), 99)
    _, g64, g32 = _refs(qkv, dout, H)
    _gate("peaked", _run(qkv, dout, H)[2], g64, g32, H)


def test_backward_zero_q_uniform_softmax():
    """q = 0: P = 1 / L, dS_ij = (dout_i . (v_j - mean v)) / L, dq_i = sum_j dS_ij k_j / 8 -- in fp64 from the operands.  The
    bound on |dq - analytic| is the worst-case rounding bound n u sum|terms| with u = 2^-24 and n = 64 (dP) + 64 (delta) + L (the
    sum over keys) + 8 (exp2, the products with P and 1 / 8) roundings on the path of a term."""
    B, H, L = 2, 3, 65
    qkv = _case(B, H, L)[0].clone()
    dout = _case(B, H, L)[1]
    q, k, v = _heads(qkv, H)
    q.zero_()
    _, g64, g32 = _refs(qkv, dout, H)
    g = _run(qkv, dout, H)[2]
    _gate("q = 0", g, g64, g32, H)
    do, k64, v64 = dout.double().view(B, L, H, 64), k.double(), v.double()
    vbar = v64.mean(dim=1, keepdim=True)
    ds = torch.einsum("bihd,bjhd->bhij", do, v64 - vbar) / L
    want = torch.einsum("bhij,bjhd->bihd", ds, k64) / 8
    ds_abs = torch.einsum("bihd,bjhd->bhij", do.abs(), v64.abs() + vbar.abs()) / L
    bound = (64 + 64 + L + 8) * 2.0 ** -24 * torch.einsum("bhij,bjhd->bihd", ds_abs, k64.abs()) / 8
    dq = g[..., :H * 64].double().view(B, L, H, 64)
    print(f"q = 0: max|dq - analytic| {float((dq - want).abs().max()):.3e}, smallest bound {float(bound.min()):.3e}, "
          f"max|dq| {float(want.abs().max()):.3e}")
    assert bool(((dq - want).abs() <= bound).all())


# ---- 4. exact zeros, no stray writes -------------------------------------------------------------------------------------------
def test_zero_dout_gives_exact_zeros():
    qkv, dout, *_ = _case(2, 2, 300)
    g = _run(qkv, torch.zeros_like(dout), 2)[2]
    assert int(torch.count_nonzero(g)) == 0 and not bool(torch.isnan(g).any())


@pytest.mark.parametrize("B,H,L", [(2, 3, 33), (1, 2, 129), (2, 2, 300)])
def test_every_element_is_written_and_nothing_beyond(B, H, L):
    from pit_hip import _lib

    qkv, dout, *_ = _case(B, H, L)
    E = H * 64
    out, lse = _lib.mha_fwd_lse(qkv, H)
    n, guard = B * L * 3 * E, 4096
    buf = torch.full((n + guard,), float("nan"), device=DEV)
    buf[n:] = 12345.0
    ws = torch.empty(max(_lib.lib().gq_mha_bwd_workspace_bytes(B, L, E, H), 8), dtype=torch.uint8, device=DEV)
    lse_guard = torch.full((B * H * L + 64,), 777.0, device=DEV)      # lse is an input: it must come back unchanged too
    lse_guard[:B * H * L] = lse.reshape(-1)
    rc = _lib.lib().gq_mha_bwd_f32(qkv.data_ptr(), out.data_ptr(), lse_guard.data_ptr(), dout.data_ptr(), buf.data_ptr(), B, L, E, H,
                                   ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert not bool(torch.isnan(buf[:n]).any())
    assert bool((buf[n:] == 12345.0).all()) and bool((lse_guard[B * H * L:] == 777.0).all())
    assert torch.equal(buf[:n].view(B, L, 3 * E), _lib.mha_bwd(qkv, out, lse, dout, H))


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------
def test_backward_is_deterministic_and_independent_of_the_address():
    from pit_hip import _lib

    qkv, dout, *_ = _case(2, 2, 300)
    out, lse, a = _run(qkv, dout, 2)
    b = _lib.mha_bwd(qkv, out, lse, dout, 2)
    assert torch.equal(a, b)
    big = torch.zeros(qkv.numel() + 8, device=DEV)
    moved = big[4:4 + qkv.numel()].view(qkv.shape)                  # 16 bytes further: still aligned, read in place
    moved.copy_(qkv)
    assert moved.data_ptr() % 16 == 0 and moved.data_ptr() != qkv.data_ptr()
    out2, lse2, c = _run(moved, dout, 2)
    assert torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(c, a)


# ---- 6.-8. the module ----------------------------------------------------------------------------------------------------------
def _encoder(tag="d64_tail", dtype=torch.float32, **override):
    from pit_hip.modules.vit import TransformerEncoder

    d = np.load(os.path.join(G, f"g21_vit_{tag}.npz"))
    params = dict(json.loads(str(d["params"]))["enc"], **override)
    enc = TransformerEncoder(**params)
    enc.load_state_dict({k[4:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("enc.")})
    return torch.from_numpy(d["x"]).to(DEV).to(dtype), enc.to(DEV).to(dtype).train()


def _grads(enc):
    named = dict(enc.named_parameters())
    return {n: named[n].grad.clone() for n in NAMES}


class _Count:
    def __init__(self, monkeypatch):
        from pit_hip import _lib

        self.n = dict(mha_fwd=0, mha_fwd_lse=0, mha_bwd=0)
        for name in self.n:
            monkeypatch.setattr(_lib, name, self._counted(name, getattr(_lib, name)))

    def _counted(self, name, real):
        def f(*a, **k):
            self.n[name] += 1
            return real(*a, **k)

        return f

    def take(self):
        got, self.n = self.n, dict.fromkeys(self.n, 0)
        return got


def test_module_under_autograd_against_the_reference_grads(monkeypatch):
    from pit_hip.modules import vit

    monkeypatch.setattr(vit, "HIP_ATTN_TRAIN", True)
    fx = np.load(os.path.join(G, "g23_vit_train_grads.npz"))
    x, enc = _encoder()
    with torch.no_grad():
        z0 = enc(x)
    z = enc(x)
    assert z.requires_grad and torch.equal(z.detach(), z0)
    (z * torch.from_numpy(fx["w"]).to(DEV)).sum().backward()
    got = _grads(enc)
    ok = True
    for n in NAMES:
        g64 = fx[f"g64.{n}"]
        eh = np.abs(got[n].cpu().numpy().astype(np.float64) - g64).max() / np.abs(g64).max()
        et = np.abs(fx[f"g32.{n}"].astype(np.float64) - g64).max() / np.abs(g64).max()
        print(f"{n}: err_hip {eh:.3e}  err_torch32 (fixture) {et:.3e}  ratio {eh / et:.2f}")
        ok = ok and eh <= MARGIN * et
    assert ok
    enc.zero_grad(set_to_none=True)
    enc(x).sum().backward()                                     # an expanded (stride 0) gradient reaches mha_bwd
    for n, g in _grads(enc).items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n


def test_routing_of_grad_enabled_calls(monkeypatch):
    from pit_hip.modules import vit

    cnt = _Count(monkeypatch)
    x, enc = _encoder()
    enc(x).sum().backward()                                     # flag off (the default): torch's route
    assert vit.HIP_ATTN_TRAIN is False and cnt.take() == dict(mha_fwd=0, mha_fwd_lse=0, mha_bwd=0)
    monkeypatch.setattr(vit, "HIP_ATTN_TRAIN", True)
    enc(x).sum().backward()                                     # one layer: one forward, one backward
    assert cnt.take() == dict(mha_fwd=0, mha_fwd_lse=1, mha_bwd=1)
    with torch.no_grad():
        enc(x)
    assert cnt.take() == dict(mha_fwd=1, mha_fwd_lse=0, mha_bwd=0)
    _, masked = _encoder("block_causal")
    masked(x).sum().backward()
    _, dropping = _encoder(attn_drop_rate=0.1)
    dropping(x).sum().backward()
    enc.set_grad_checkpointing(True, selective=True)
    enc(x).sum().backward()
    enc.set_grad_checkpointing(False)
    x64, enc64 = _encoder(dtype=torch.float64)
    enc64(x64).sum().backward()
    assert cnt.take() == dict(mha_fwd=0, mha_fwd_lse=0, mha_bwd=0)


def test_whole_block_checkpointing_gives_the_same_grads(monkeypatch):
    from pit_hip.modules import vit

    monkeypatch.setattr(vit, "HIP_ATTN_TRAIN", True)
    cnt = _Count(monkeypatch)
    fx = np.load(os.path.join(G, "g23_vit_train_grads.npz"))
    w = torch.from_numpy(fx["w"]).to(DEV)
    x, enc = _encoder()
    (enc(x) * w).sum().backward()
    plain = _grads(enc)
    assert cnt.take() == dict(mha_fwd=0, mha_fwd_lse=1, mha_bwd=1)
    enc.zero_grad(set_to_none=True)
    enc.set_grad_checkpointing(True)
    (enc(x) * w).sum().backward()
    assert cnt.take() == dict(mha_fwd=0, mha_fwd_lse=2, mha_bwd=1)     # the block's forward runs again in the backward
    for n, g in _grads(enc).items():
        assert torch.equal(g, plain[n]), n
