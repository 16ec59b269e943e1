"""BSQQuantizer on the HIP sign/bit-pack kernels (reference pit/quantization/bsq.py:39-156).

Binary spherical quantisation: L2-normalise the channel vector, take signs, scale by
1/sqrt(embed_dim); the index packs the 16 sign bits big-endian (bsq.py:95-99 hard-codes 16).
Eval losses are zeros like the reference (bsq.py:113-118).  With GQHIP_BSQ_TRAIN_FUSED=1 in the environment (read per
call: ``_fused.train_fused_opt_in``) a HIP tensor in ``train()`` takes ONE forward library call (``bsq_train_f32``) and,
under autograd, ONE backward call (``bsq_backward_f32``); unset, or with GQHIP_TRAIN_FUSED=0, the torch route below runs."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _lib
from ._fused import format_view, train_fused_opt_in
from .lfq import LFQQuantizer


def bsq_entropy_loss(x, embed_dim, temperature=0.01, sample_minimization_weight=1.0,
                     batch_maximization_weight=1.0, eps=1e-5):
    """bsq.py:14-36."""
    probs = torch.sigmoid(-4 * x / (embed_dim ** 0.5) / temperature)
    probs = torch.stack([probs, 1 - probs], dim=-1)
    log_probs = torch.log(probs + eps)
    avg_probs = probs.reshape(-1, probs.shape[-2], probs.shape[-1]).mean(0)
    avg_entropy = -torch.sum(avg_probs * torch.log(avg_probs + eps))
    sample_entropy = torch.mean(-torch.sum(probs * log_probs, [-2, -1]))
    loss = sample_minimization_weight * sample_entropy - batch_maximization_weight * avg_entropy
    return sample_entropy, avg_entropy, loss


class _BSQTrainFn(torch.autograd.Function):
    """One forward library call and one backward library call for BSQQuantizer's train step under autograd.

    ``xv`` is x in a library layout; ``cfg`` = (codebook_dim, layout, w_s, w_b, workspace).  Differentiable outputs: quantized
    and entropy_aux_loss; the indices and the two entropies are not.  Saved: x and ``avg`` ([d, 2] floats) -- the backward
    rebuilds u, p and q from x."""

    @staticmethod
    def forward(ctx, xv, cfg):
        d, layout, w_s, w_b, ws = cfg
        quantized, ind, avg, scal = _lib.bsq_train(xv, d, layout, w_s, w_b, ws)
        aux, sample, batch = scal.unbind(0)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xv, avg)
        ctx.mark_non_differentiable(ind, sample, batch)
        return quantized, ind, aux, sample, batch

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_q, _g_ind, g_aux, _g_sample, _g_batch):
        xv, avg = ctx.saved_tensors
        d, layout, w_s, w_b, ws = ctx.cfg
        return _lib.bsq_backward(xv, avg, d, layout, w_s, w_b, g_q=g_q, g_aux=g_aux, ws=ws), None


class BSQQuantizer(LFQQuantizer):
    def __init__(self, format, codebook_size, num_codebooks=1, sample_minimization_weight=1.0,
                 batch_maximization_weight=1.0):
        super().__init__(format=format, codebook_size=codebook_size, num_codebooks=num_codebooks,
                         sample_minimization_weight=sample_minimization_weight,
                         batch_maximization_weight=batch_maximization_weight)
        self.embed_dim = self.codebook_dim * num_codebooks
        self._bws = _lib.BsqTrainWorkspace()

    def _forward_fused(self, x):
        """bsq.py:64-133 in train() as one call.  A channels_last x is read, and quantized / indices are written, in that memory
        (_fused.format_view); nothing is copied in either direction."""
        assert self.num_codebooks == 16, "the reference packs exactly 16 codebook bits (bsq.py:97)"
        xv, layout, as_module = format_view(x.float(), self.format)
        cfg = (self.codebook_dim, layout, self.sample_minimization_weight, self.batch_maximization_weight, self._bws)
        if torch.is_grad_enabled() and xv.requires_grad:
            quantized, ind, aux, sample, batch = _BSQTrainFn.apply(xv, cfg)
        else:
            quantized, ind, _, scal = _lib.bsq_train(xv, *cfg)
            aux, sample, batch = scal.unbind(0)
        info = {"indices": as_module(ind), "entropy_aux_loss": aux, "per_sample_entropy": sample.detach(),
                "codebook_entropy": batch.detach()}
        return as_module(quantized).to(x.dtype), info

    def forward(self, x):
        if x.is_cuda and self.training and train_fused_opt_in("bsq"):
            return self._forward_fused(x)
        if self.format == "bchw":
            b, c, h, w = x.shape
            xf = x.reshape(b, c, h * w).transpose(1, 2)
        else:
            b, _, c = x.shape
            xf = x
        l = xf.shape[1]
        xf = F.normalize(xf, dim=-1)
        q_scale = 1.0 / (self.embed_dim ** 0.5)
        d = self.codebook_dim
        assert self.num_codebooks == 16, "the reference packs exactly 16 codebook bits (bsq.py:97)"
        xs = xf.reshape(b, l, self.num_codebooks, d)
        # pack over the codebook axis for every d: rows = (b, l, d), bits = the 16 codebooks
        rows = xs.detach().float().permute(0, 1, 3, 2).reshape(-1, self.num_codebooks).contiguous()
        with torch.no_grad():
            idx, q = _lib.lfq_pack(rows)
        indices = idx.reshape(b, l, d)
        q = q.reshape(b, l, d, self.num_codebooks).permute(0, 1, 3, 2).to(x.dtype)
        quantized = (xs + (q - xs).detach()) * q_scale
        if self.training:
            per_sample_entropy, codebook_entropy, entropy_aux_loss = bsq_entropy_loss(
                x=xs, embed_dim=self.embed_dim, sample_minimization_weight=self.sample_minimization_weight,
                batch_maximization_weight=self.batch_maximization_weight)
        else:
            per_sample_entropy = codebook_entropy = entropy_aux_loss = self.zero
        quantized = quantized.reshape(b, l, c)
        if self.format == "bchw":
            quantized = quantized.transpose(1, 2).reshape(b, c, h, w)
            indices = indices.transpose(1, 2).reshape(b, d, h, w)
        info = {"indices": indices, "entropy_aux_loss": entropy_aux_loss,
                "per_sample_entropy": per_sample_entropy.detach(), "codebook_entropy": codebook_entropy.detach()}
        return quantized, info

    def dequant(self, indices):
        if self.format == "bchw":
            b, ng, h, w = indices.shape
            ind = indices.reshape(b, ng, h * w).transpose(1, 2)
        else:
            b, _, ng = indices.shape
            ind = indices
        l = ind.shape[1]
        q = _lib.lfq_unpack(ind.contiguous().reshape(-1), 16).reshape(b, l, ng, 16)
        q = q * (1.0 / (self.embed_dim ** 0.5))
        if self.format == "bchw":
            q = q.reshape(b, h, w, ng, 16).permute(0, 3, 4, 1, 2).reshape(b, ng * 16, h, w)
        return q
