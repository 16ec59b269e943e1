"""VQQuantizer on the HIP arg-min path (reference pit/quantization/vq.py:8-129).

Same constructor, same ``embedding.weight`` parameter (so checkpoints load), same
``forward -> (z_q, {"indices", "codebook_loss"})`` / ``dequant`` contracts.  The
``[rows, n]`` distance matrix of vq.py:58-69 is never built: the nearest code is
found by the MFMA filter (``-|e|^2 + 2 z.e``) + an fp64 re-rank of its candidates.
On a HIP tensor the whole forward -- permutes, per-sub-codebook slices, embedding
lookup, straight-through value, the two MSE means -- is ONE library call
(``vq_quantize_z_f32``).  When autograd records, that call sits behind a
``torch.autograd.Function`` whose backward is ONE library call as well
(``vq_backward_f32``: grad_z elementwise, grad of the codebook as a bit-reproducible
scatter-reduce, no float atomics); neither reads the host.  ``GQHIP_TRAIN_FUSED=0``
in the environment (read per call: ``_fused.train_fused``, the one switch of every
fused train step) selects the op-by-op path instead: the arg-min in the library
(``vq_argmin_f32``), the differentiable glue in torch.  CPU tensors always take that
path."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ._fused import format_view, train_fused


class _VQTrainFn(torch.autograd.Function):
    """One forward library call and one backward library call for VQQuantizer's step under autograd.

    ``zv`` is z in a library layout, ``weight`` the codebook; ``cfg`` = (dim, layout, beta, legacy, use_cache, forward workspace,
    backward workspace).  Differentiable outputs: z_q and codebook_loss; the indices are not.  Saved: z, the indices and the
    codebook -- the backward recomputes e = weight[indices], so no z_q is kept."""

    @staticmethod
    def forward(ctx, zv, weight, cfg):
        dim, layout, beta, legacy, use_cache, ws, _ = cfg
        ind, zq, loss = _lib.vq_quantize_z(zv, weight.detach(), dim, layout, beta, legacy, ws, use_cache=use_cache)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(zv, ind, weight)
        ctx.mark_non_differentiable(ind)
        return zq, ind, loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_zq, _g_ind, g_loss):
        zv, ind, weight = ctx.saved_tensors
        dim, layout, beta, legacy, _, _, bws = ctx.cfg
        grad_z, grad_emb = _lib.vq_backward(zv, weight.detach(), ind, dim, layout, beta, legacy, g_zq=g_zq, g_loss=g_loss,
                                            want_grad_z=ctx.needs_input_grad[0], want_grad_emb=ctx.needs_input_grad[1], ws=bws)
        return grad_z, grad_emb, None


class VQQuantizer(nn.Module):
    def __init__(self, format, n, dim, beta=0.25, codebook_num=1, legacy=True):
        super().__init__()
        self.format, self.n, self.dim = format, n, dim
        self.beta, self.legacy, self.codebook_num = beta, legacy, codebook_num
        self.embedding = nn.Embedding(self.n, self.dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n, 1.0 / self.n)
        self._ws = _lib.Workspace()
        self._bws = _lib.VqBackwardWorkspace()

    def get_trainable_parameters(self):
        return self.embedding.parameters()

    def _to_bhwc(self, t):
        if self.format == "bchw":
            return t.permute(0, 2, 3, 1).contiguous()
        b, l, c = t.shape
        h = int(np.sqrt(l))
        assert h * h == l, "Input length must be a perfect square for blc format"
        return t.reshape(b, h, h, c).contiguous()

    def _from_bhwc(self, t):
        if self.format == "bchw":
            return t.permute(0, 3, 1, 2).contiguous()
        b, h, w, c = t.shape
        return t.reshape(b, h * w, c).contiguous()

    def _forward_fused(self, z, recording=False):
        """vq.py:39-96 as one call.  A channels_last z (what the NHWC conv stack hands over) is read, and z_q / indices are written,
        in that memory layout (_fused.format_view).  ``recording``: autograd records, so the call goes through _VQTrainFn (the
        permuted views are autograd's own, they copy nothing in either direction)."""
        z = z.float()

        def run(zv, layout):
            if recording:
                # a learned codebook moves every optimizer step: no per-codebook cache while training (the dim-4 search index
                # would be rebuilt by one block per call); eval with autograd on keeps it
                return _VQTrainFn.apply(zv, self.embedding.weight.float(), (self.dim, layout, self.beta, self.legacy,
                                                                            not self.training, self._ws, self._bws))
            ind, zq, loss = _lib.vq_quantize_z(zv, self.embedding.weight.detach().float(), self.dim, layout, self.beta, self.legacy,
                                               self._ws)
            return zq, ind, loss[0]

        if self.format == "bchw":
            b, c, h, wd = z.shape
        else:
            b, l, c = z.shape
            h = int(np.sqrt(l))
            assert h * h == l, "Input length must be a perfect square for blc format"
        assert self.dim * self.codebook_num == c
        zv, layout, restore = format_view(z, self.format)
        zq, ind, loss = run(zv, layout)
        return restore(zq), {"indices": restore(ind), "codebook_loss": loss}

    def forward(self, z):
        recording = torch.is_grad_enabled() and (z.requires_grad or self.embedding.weight.requires_grad)
        if z.is_cuda and (not recording or train_fused()):
            return self._forward_fused(z, recording)
        z = self._to_bhwc(z)
        assert self.dim * self.codebook_num == z.shape[-1]
        zf = z.reshape(-1, self.dim, self.codebook_num)  # channel = d*K + k (vq.py:53)
        w = self.embedding.weight
        z_q, indices = [], []
        for k in range(self.codebook_num):
            with torch.no_grad():
                # a learned codebook moves every optimizer step: no per-codebook cache while training (the dim-4 search index would
                # be rebuilt by one block per call); eval with autograd on keeps it
                idx, _ = _lib.vq_argmin(zf[:, :, k].detach().float().contiguous(), w.detach().float(), ws=self._ws,
                                        use_cache=not self.training)
            z_q.append(self.embedding(idx)[:, :, None])
            indices.append(idx[:, None])
        z_q = torch.cat(z_q, dim=2).view(z.shape)
        indices = torch.cat(indices, dim=1).reshape(z.shape[0], z.shape[1], z.shape[2], self.codebook_num)
        if not self.legacy:
            loss = self.beta * torch.mean((z_q.detach() - z) ** 2) + torch.mean((z_q - z.detach()) ** 2)
        else:
            loss = torch.mean((z_q.detach() - z) ** 2) + self.beta * torch.mean((z_q - z.detach()) ** 2)
        z_q = z + (z_q - z).detach()
        return self._from_bhwc(z_q), {"indices": self._from_bhwc(indices), "codebook_loss": loss}

    def dequant(self, indices):
        ind = self._to_bhwc(indices)
        b, h, w, _ = ind.shape
        flat = ind.reshape(-1, self.codebook_num)
        z_q = torch.cat([self.embedding(flat[:, k])[:, :, None] for k in range(self.codebook_num)], dim=2)
        return self._from_bhwc(z_q.reshape(b, h, w, self.dim * self.codebook_num))
