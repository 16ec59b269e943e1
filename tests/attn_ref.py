"""fp64 numpy restatement of unmasked multi-head self-attention, the yardstick of the fused HIP kernel (csrc/gq_attn.h).

``mha_from_qkv(qkv, heads)``: qkv [B, L, 3E] (the in-projection output) -> [B, L, E], per (batch, head)
softmax(q k^T / sqrt(d)) v with the heads concatenated -- what nn.MultiheadAttention computes between in_proj and out_proj.
``mha(x, in_w, in_b, out_w, out_b, heads)``: the whole layer on batch-first x [B, L, E]."""
import numpy as np


def mha_from_qkv(qkv, heads: int) -> np.ndarray:
    qkv = np.asarray(qkv, dtype=np.float64)
    B, L, E3 = qkv.shape
    E = E3 // 3
    d = E // heads
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, L, heads, d).transpose(0, 2, 1, 3) for i in range(3))
    s = np.einsum("bhld,bhmd->bhlm", q, k) / np.sqrt(d)
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    o = np.einsum("bhlm,bhmd->bhld", p, v)
    return o.transpose(0, 2, 1, 3).reshape(B, L, E)


def mha(x, in_w, in_b, out_w, out_b, heads: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    qkv = x @ np.asarray(in_w, np.float64).T + np.asarray(in_b, np.float64)
    return mha_from_qkv(qkv, heads) @ np.asarray(out_w, np.float64).T + np.asarray(out_b, np.float64)
