"""fp64 numpy restatement of the backward of unmasked multi-head self-attention, the yardstick of the fused HIP backward
(csrc/gq_attn_bwd.h), in the style of attn_ref.py.

``lse_from_qkv(qkv, heads)``: qkv [B, L, 3E] -> [B, heads, L], the natural log-sum-exp of the scaled logits s = q k^T / sqrt(d)
(the kernel stores it divided by ln 2).
``mha_bwd_from_qkv(qkv, dout, heads)``: the gradient of qkv [B, L, 3E] (dq | dk | dv in qkv's layout) for the gradient dout
[B, L, E] of ``attn_ref.mha_from_qkv(qkv, heads)``, by the five formulas the kernels use:
    P = exp(s - lse),  delta_i = sum_d dout[i, d] out[i, d],  dV = P^T dout,  dP = dout V^T,  dS = P o (dP - delta),
    dQ = dS K / sqrt(d),  dK = dS^T Q / sqrt(d)."""
import numpy as np


def _heads(x, heads):
    B, L, E = x.shape
    return x.reshape(B, L, heads, E // heads).transpose(0, 2, 1, 3)


def _split(qkv, heads):
    qkv = np.asarray(qkv, dtype=np.float64)
    E = qkv.shape[2] // 3
    return [_heads(qkv[..., i * E:(i + 1) * E], heads) for i in range(3)]


def lse_from_qkv(qkv, heads: int) -> np.ndarray:
    q, k, _ = _split(qkv, heads)
    s = np.einsum("bhld,bhmd->bhlm", q, k) / np.sqrt(q.shape[-1])
    m = s.max(axis=-1)
    return m + np.log(np.exp(s - m[..., None]).sum(axis=-1))


def mha_bwd_from_qkv(qkv, dout, heads: int) -> np.ndarray:
    q, k, v = _split(qkv, heads)
    B, H, L, d = q.shape
    do = _heads(np.asarray(dout, dtype=np.float64), heads)
    s = np.einsum("bhld,bhmd->bhlm", q, k) / np.sqrt(d)
    p = np.exp(s - lse_from_qkv(qkv, heads)[..., None])
    out = np.einsum("bhlm,bhmd->bhld", p, v)
    delta = (do * out).sum(axis=-1)
    dv = np.einsum("bhlm,bhld->bhmd", p, do)
    dp = np.einsum("bhld,bhmd->bhlm", do, v)
    ds = p * (dp - delta[..., None])
    dq = np.einsum("bhlm,bhmd->bhld", ds, k) / np.sqrt(d)
    dk = np.einsum("bhlm,bhld->bhmd", ds, q) / np.sqrt(d)
    return np.concatenate([g.transpose(0, 2, 1, 3).reshape(B, L, H * d) for g in (dq, dk, dv)], axis=2)
