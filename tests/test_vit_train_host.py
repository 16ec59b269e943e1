"""CPU: the host half of the fused attention backward (csrc/gq_attn_bwd.h) -- the three entry points exist and validate their
arguments before any HIP call, the Python wrappers refuse what has no kernel, the training flag is off by default and never
sends a CPU module to the library, the fixture g23 loads and the torch route reproduces its fp32 gradients bit for bit, and the
fp64 checker the GPU tests rely on (tests/attn_bwd_ref.py) is proven against torch's fp64 autograd and a central difference."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import attn_bwd_ref
import attn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INVALID = 1          # GQHIP_ERR_INVALID_ARG
NAMES = ("transformer.resblocks.0.attn.in_proj_weight", "transformer.resblocks.0.attn.in_proj_bias",
         "transformer.resblocks.0.ln_1.weight", "positional_embedding")


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


def test_attention_training_symbols_are_exported_and_bound():
    L = _lib()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("gq_mha_fwd_lse_f32", "gq_mha_bwd_workspace_bytes", "gq_mha_bwd_f32"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(dll, name) and hasattr(L.lib(), name)
    assert L.lib().gqhip_abi_version() == 8         # additive: the version does not move
    assert L.lib().gq_mha_bwd_workspace_bytes(2, 37, 128, 2) >= 2 * 2 * 37 * 4      # delta, one float per (batch, head, row)
    assert L.lib().gq_mha_bwd_workspace_bytes(0, 37, 128, 2) == 0


def _fwd(L, qkv=64, out=128, lse=192, B=2, Lq=8, E=128, H=2):
    return L.gq_mha_fwd_lse_f32(qkv, out, lse, B, Lq, E, H, None, None)


def _bwd(L, qkv=64, out=128, lse=192, dout=256, dqkv=320, B=2, Lq=8, E=128, H=2, ws=384):
    return L.gq_mha_bwd_f32(qkv, out, lse, dout, dqkv, B, Lq, E, H, ws, None)


# E != 64 H, H = 0 (with and without a matching E), negative sizes, B H = 65536 > 65535
BAD_SHAPES = (dict(E=192), dict(H=0, E=0), dict(H=0), dict(B=-1), dict(Lq=-1), dict(B=32768))


def test_attention_training_entry_points_validate_before_any_hip_call():
    """Pointers here are small fake addresses: every call must be rejected on its arguments alone."""
    L = _lib().lib()
    for kw in (dict(qkv=None), dict(out=None), dict(lse=None), dict(qkv=72), dict(out=132), dict(lse=194)) + BAD_SHAPES:
        assert _fwd(L, **kw) == INVALID, kw
    for kw in (dict(qkv=None), dict(out=None), dict(lse=None), dict(dout=None), dict(dqkv=None), dict(ws=None),
               dict(qkv=72), dict(out=136), dict(dout=260), dict(dqkv=328), dict(lse=193), dict(ws=386)) + BAD_SHAPES:
        assert _bwd(L, **kw) == INVALID, kw


def test_attention_training_with_no_rows_is_ok_and_launches_nothing():
    L = _lib().lib()
    assert _fwd(L, B=0) == 0 and _bwd(L, B=0) == 0
    assert _fwd(L, Lq=0) == 0 and _bwd(L, Lq=0) == 0
    assert _fwd(L, B=0, qkv=None, out=None, lse=None) == 0 and _bwd(L, B=0, qkv=None, dqkv=None, ws=None) == 0


def test_wrappers_refuse_cpu_tensors_and_unbuilt_head_dims():
    L = _lib()
    with pytest.raises(L.GqHipError):
        L.mha_fwd_lse(torch.zeros(1, 4, 3 * 128), 2)                    # CPU tensor: no fallback
    with pytest.raises(L.GqHipError):
        L.mha_bwd(torch.zeros(1, 4, 3 * 128), torch.zeros(1, 4, 128), torch.zeros(1, 2, 4), torch.zeros(1, 4, 128), 2)
    with pytest.raises(L.GqHipError):
        L.mha_fwd_lse(torch.zeros(1, 4, 3 * 96), 3)                     # head dim 32 (and a CPU tensor)
    with pytest.raises(L.GqHipError):
        L.mha_bwd(torch.zeros(1, 4, 3 * 96), torch.zeros(1, 4, 96), torch.zeros(1, 3, 4), torch.zeros(1, 4, 96), 3)


@pytest.mark.parametrize("fn", ["mha_fwd_lse", "mha_bwd"])
def test_wrappers_check_the_head_dim_before_the_library(fn, monkeypatch):
    """Head dim 32 is refused by the wrapper's own check, whatever the device: with the device check stubbed out the error is
    the head-dim one and the library is never asked."""
    L = _lib()
    monkeypatch.setattr(L, "_dev", lambda t, dtype, name: t)
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    args = (torch.zeros(1, 4, 3 * 96), 3) if fn == "mha_fwd_lse" else \
        (torch.zeros(1, 4, 3 * 96), torch.zeros(1, 4, 96), torch.zeros(1, 3, 4), torch.zeros(1, 4, 96), 3)
    with pytest.raises(L.GqHipError, match="head dim 32"):
        getattr(L, fn)(*args)


def _load_enc(dtype=torch.float32):
    from pit_hip.modules.vit import TransformerEncoder

    d = np.load(os.path.join(G, "g21_vit_d64_tail.npz"))
    enc = TransformerEncoder(**json.loads(str(d["params"]))["enc"])
    enc.load_state_dict({k[4:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("enc.")}, strict=True)
    return d, enc.to(dtype).train()


def test_training_flag_is_off_by_default_and_cpu_never_enters_the_library(monkeypatch):
    from pit_hip import _lib as L
    from pit_hip.modules import vit

    assert vit.HIP_ATTN_TRAIN is False

    def boom(*a, **k):
        raise AssertionError("the HIP kernel was entered")

    for name in ("mha_fwd", "mha_fwd_lse", "mha_bwd"):
        monkeypatch.setattr(L, name, boom)
    monkeypatch.setattr(vit, "HIP_ATTN_TRAIN", True)
    d, enc = _load_enc()
    z = enc(torch.from_numpy(d["x"]))
    z.sum().backward()
    assert enc.transformer.resblocks[0].attn.in_proj_weight.grad is not None


def test_fixture_loads_and_is_complete():
    d, enc = _load_enc()
    g = np.load(os.path.join(G, "g23_vit_train_grads.npz"))
    named = dict(enc.named_parameters())
    assert g["w"].shape == d["z"].shape and g["w"].dtype == np.float32
    for n in NAMES:
        a, b = g[f"g32.{n}"], g[f"g64.{n}"]
        assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape == tuple(named[n].shape), n
        assert np.isfinite(b).all() and np.abs(b).max() > 0
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), n         # the fp32 run is the fp64 run, rounded along the way
    assert sorted(g.files) == sorted(["w"] + [f"{t}.{n}" for t in ("g32", "g64") for n in NAMES])
    assert os.path.getsize(os.path.join(G, "g23_vit_train_grads.npz")) < (1 << 20)


def test_torch_route_reproduces_the_reference_fp32_grads_bit_for_bit():
    d, enc = _load_enc()
    g = np.load(os.path.join(G, "g23_vit_train_grads.npz"))
    (enc(torch.from_numpy(d["x"])) * torch.from_numpy(g["w"])).sum().backward()
    named = dict(enc.named_parameters())
    for n in NAMES:
        assert np.array_equal(named[n].grad.numpy(), g[f"g32.{n}"]), n


def _torch64(qkv, dout, heads):
    """torch's fp64 autograd of softmax(q k^T / sqrt(d)) v: (out, lse, dqkv)"""
    t = torch.from_numpy(qkv).requires_grad_(True)
    B, L, E3 = t.shape
    E = E3 // 3
    q, k, v = (t[..., i * E:(i + 1) * E].reshape(B, L, heads, E // heads).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / (E // heads) ** 0.5
    out = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, E)
    out.backward(torch.from_numpy(dout))
    return out.detach().numpy(), torch.logsumexp(s, dim=-1).detach().numpy(), t.grad.numpy()


def test_attn_bwd_ref_matches_torch_fp64_autograd():
    B, H, L = 2, 2, 37
    rng = np.random.default_rng(37)
    qkv, dout = rng.standard_normal((B, L, 3 * H * 64)), rng.standard_normal((B, L, H * 64))
    out, lse, want = _torch64(qkv, dout, H)
    got = attn_bwd_ref.mha_bwd_from_qkv(qkv, dout, H)
    assert got.shape == want.shape
    E = H * 64
    for i in range(3):      # dq, dk, dv each at 1e-12 of its own scale
        a, b = got[..., i * E:(i + 1) * E], want[..., i * E:(i + 1) * E]
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), i
    assert np.abs(attn_bwd_ref.lse_from_qkv(qkv, H) - lse).max() <= 1e-12 * np.abs(lse).max()
    assert np.abs(attn_ref.mha_from_qkv(qkv, H) - out).max() <= 1e-12 * np.abs(out).max()


def test_attn_bwd_ref_against_a_central_difference():
    """loss = sum(dout o attention(qkv)) in fp64, step 1e-6 on 24 random entries (8 each in the q, k and v blocks): agreement to
    1e-7 of the block's largest gradient -- coarse on purpose (the quotient is good to ~1e-9; a wrong formula is off by order 1)."""
    B, H, L = 2, 2, 37
    E = H * 64
    rng = np.random.default_rng(38)
    qkv, dout = rng.standard_normal((B, L, 3 * E)), rng.standard_normal((B, L, E))
    g = attn_bwd_ref.mha_bwd_from_qkv(qkv, dout, H)

    def loss(x):
        return float((attn_ref.mha_from_qkv(x, H) * dout).sum())

    h = 1e-6
    for blk in range(3):
        scale = np.abs(g[..., blk * E:(blk + 1) * E]).max()
        for _ in range(8):
            i = (rng.integers(B), rng.integers(L), blk * E + rng.integers(E))
            xp, xm = qkv.copy(), qkv.copy()
            xp[i] += h
            xm[i] -= h
            num = (loss(xp) - loss(xm)) / (2 * h)
            assert abs(num - g[i]) <= 1e-7 * scale, (i, num, g[i])
