"""Frechet distance between two feature sets (the reference's pit/evaluations/fid/fid_score.py and the mean / covariance it is fed
by eval.py:186-203, 241-259), with the statistics accumulated where the features are.

The reference keeps every [bs, 2048] feature block on the host and runs np.mean / np.cov over all of them at the end.  The raw
first and second moments are additive over images, so ``FrechetStats`` keeps (sum x x^T, sum x, n) in fp64 on the features' device
and folds each block in as it arrives:

    outer[i][j] <- fma(x[r][i], x[r][j], outer[i][j])    row by row, in ascending r, for j >= i
    sum[i]      <- sum[i] + x[r][i]

The product of two fp32 values is exact in fp64 (48 significant bits, exponent far inside the range), so each step rounds once
and the HIP kernel (csrc/gq_moments.h), the CPU loop below and any split of the rows over calls give the same bits.

Domain: the covariance comes from raw moments, cov = (outer - sum sum^T / n) / (n - 1).  For features whose (mean / std)^2 is
large that loses about n 2^-53 (1 + (mean / std)^2) relative accuracy in cov -- about 5e-10 for pooled Inception features at
n = 50 000 -- so no shift is applied.
"""
from __future__ import annotations

from typing import Iterable, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def state_words(D: int) -> int:
    """fp64 words of a state: [ outer: D D, row-major | sum: D | count: 1 ]."""
    return D * D + D + 1


class FrechetStats:
    """The raw moments of a stream of feature blocks, in fp64 on ``device``: ``state`` is one zeroed tensor
    [ outer: D D | sum: D | count: 1 ] that ``update`` adds to.  Only the upper triangle (j >= i) of ``outer`` is defined."""

    def __init__(self, D: int, device) -> None:
        if not 1 <= D <= 8192:
            raise ValueError(f"FrechetStats: 1 <= D <= 8192, got {D}")
        self.D = D
        self.state = torch.zeros(state_words(D), dtype=torch.float64, device=device)
        self.device = self.state.device       # "cuda" has become "cuda:<current>"

    @property
    def outer(self) -> torch.Tensor:
        return self.state[: self.D * self.D].view(self.D, self.D)

    @property
    def sum(self) -> torch.Tensor:
        return self.state[self.D * self.D: self.D * self.D + self.D]

    @property
    def count(self) -> torch.Tensor:
        return self.state[-1:]

    @torch.no_grad()
    def update(self, feats: torch.Tensor) -> "FrechetStats":
        """Fold in ``feats``: fp32 [B, D], or [B, D, h, w], which is pooled with adaptive_avg_pool2d(.., (1, 1)) first
        (eval.py:188-190).  On a HIP device one kernel launch; on the CPU the same rule as a sequential loop.  No host read."""
        if feats.dim() == 4:
            if feats.shape[2] != 1 or feats.shape[3] != 1:
                feats = F.adaptive_avg_pool2d(feats, (1, 1))
            feats = feats[:, :, 0, 0]
        if feats.dim() != 2 or feats.shape[1] != self.D:
            raise ValueError(f"FrechetStats.update: feats must be [B, {self.D}] or [B, {self.D}, h, w], got {tuple(feats.shape)}")
        if feats.dtype != torch.float32:
            raise ValueError(f"FrechetStats.update: feats must be float32 (the exactness of the fp64 sums rests on it), got {feats.dtype}")
        if feats.device != self.device:
            raise ValueError(f"FrechetStats.update: feats are on {feats.device}, the statistics on {self.device}")
        if feats.is_cuda:
            from ... import _lib

            if feats.shape[1] > 1 and feats.stride(1) != 1:
                feats = feats.contiguous()
            _lib.moments_update(feats, self.state)
            return self
        outer, total = self.outer, self.sum
        for row in feats.to(torch.float64):
            outer.addr_(row, row)         # outer + row row^T: the products are exact, one rounding per element
            total.add_(row)
        self.count.add_(feats.shape[0])
        return self

    @torch.no_grad()
    def merge_(self, states: Iterable[torch.Tensor]) -> "FrechetStats":
        """Add other ranks' states (each a [D D + D + 1] fp64 tensor), in the order given."""
        for s in states:
            if s.numel() != self.state.numel() or s.dtype != torch.float64:
                raise ValueError(f"FrechetStats.merge_: a state is float64 [{self.state.numel()}], got {s.dtype} {tuple(s.shape)}")
            self.state.add_(s.reshape(-1).to(self.device))
        return self

    @torch.no_grad()
    def moments(self) -> Tuple[int, torch.Tensor, torch.Tensor]:
        """(n, mean [D], cov [D, D]) in fp64 on the CPU: mean = sum / n, cov = (outer - sum sum^T / n) / (n - 1) -- np.mean and
        np.cov(rowvar=False) of all rows.  The symmetric matrix is built from the upper triangle alone, element by element in one
        order, so cov is bit-symmetric and the same bits whichever device accumulated the state.  n < 2 raises."""
        state = self.state.cpu()
        D = self.D
        n = int(state[-1])
        if n < 2:
            raise ValueError(f"FrechetStats.moments: a covariance needs at least 2 rows, got {n}")
        upper = torch.triu(state[: D * D].view(D, D))
        outer = upper + torch.triu(upper, 1).T
        total = state[D * D: D * D + D]
        upper_c = torch.triu((outer - torch.outer(total, total) / n) / (n - 1))
        cov = upper_c + torch.triu(upper_c, 1).T
        return n, total / n, cov


def _f64(a) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.detach().to("cpu", torch.float64)
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """d^2 = |mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrt(sigma1 sigma2), as the reference's function of this name; numpy or
    torch inputs, a Python float out.  Computed in torch fp64 on the CPU whatever device produced the statistics (it runs once
    per evaluation), so the value does not depend on that device.

    The reference takes scipy's Schur ``sqrtm`` of the non-symmetric product.  Here R = sigma1^(1/2) comes from eigh(sigma1) with
    the eigenvalues clamped at 0, M = R sigma2 R is symmetrised, and tr sqrt(sigma1 sigma2) = sum sqrt(max(eigvalsh(M), 0)): the
    two products have the same eigenvalues.  ``eps`` is accepted for signature compatibility and unused: this route is finite on
    singular covariances, where the reference adds ``eps`` to the diagonals only after ``sqrtm`` has failed, so the values may
    differ from the reference's there (n <= D)."""
    mu1, mu2 = _f64(mu1).reshape(-1), _f64(mu2).reshape(-1)
    sigma1, sigma2 = torch.atleast_2d(_f64(sigma1)), torch.atleast_2d(_f64(sigma2))
    if mu1.shape != mu2.shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise ValueError("Training and test covariances have different dimensions")
    diff = mu1 - mu2
    sigma1 = (sigma1 + sigma1.T) / 2
    lam, Q = torch.linalg.eigh(sigma1)
    R = (Q * lam.clamp(min=0).sqrt()) @ Q.T
    M = R @ sigma2 @ R
    M = (M + M.T) / 2
    tr_covmean = torch.linalg.eigvalsh(M).clamp(min=0).sqrt().sum()
    return float(diff.dot(diff) + torch.trace(sigma1) + torch.trace(sigma2) - 2 * tr_covmean)
