"""Gaussian-quantisation regularizers, MI355X path.

Drop-in mirrors of ``pit.quantization.gaussian`` (reference file
pit/quantization/gaussian.py): same constructor keywords, same ``forward(z) ->
(zhat, info)`` / ``dequant(indices) -> zhat`` contracts, same buffer names
(``prior_samples``, ``normal_log_prob``, both non-persistent).  The eval branch
(gaussian.py:120-160 and :273-331) runs as ONE call into libgqhip.so
(``gq_quantize_z_f32``): chunk / clamp / exp, the group permutes, the
rows x 65 536 score matrix, the arg-max and the codeword gather are all inside
the HIP kernels and the score matrix never exists in HBM.  For
``GaussianQuantRegularizer2`` the whole eval forward (gaussian.py:333-345: the
Gaussian branch's sample, KL statistics, re-weighted loss and lambda state
machine, quant_vq, the straight-through mix) is ONE call as well
(``gq_quantize_z_gauss_f32``) whenever autograd is not recording; the lambda
state then advances on the device and is read back only when somebody looks.

Training (``GaussianQuantRegularizer`` in ``train()``, ``GaussianQuantRegularizer2``
whenever autograd records) on a HIP tensor is one forward library call
(``gq_gauss_train_f32`` / ``gq_quantize_z_gauss_f32``) and one backward library call
(``gq_gauss_backward_f32``) behind a single ``torch.autograd.Function``; neither
reads the host: lambdas, thresholds and the loss stay on the device.  The noise is
drawn once per forward with ``torch.randn`` in the shape and memory layout of
``zhat`` (as the eval paths do), so a test can re-draw it from the seed.
``GQHIP_TRAIN_FUSED=0`` in the environment (read per call) selects the op-by-op
torch path instead, for A/B runs and as an escape hatch.

backend:
  "hip"   fused path (default here).
  "cuda"  what every shipped GQ YAML says (configs/sd3unet_gq_0.25.yaml:33): in
          the reference that selects its fast path, and it selects the fast path
          here too -- the fused kernels, indices bit-identical to the reference's
          torch backend, no score matrix (``self.perturbed`` stays ``None``).
  "cuda-compat" (or backend "cuda" with GQHIP_COMPAT=1 in the environment)
          the reference's own call sequence -- ``gq_cuda.ops.gq_cuda`` into a
          persistent ``perturbed`` buffer, then ``torch.argmax`` and
          ``index_select`` (gaussian.py:124-133) -- served by our HIP build of
          the ``extension_cpp::gq`` op: for users who want the rows x n score
          matrix.  HBM-bound by construction (4.29 GB written and re-read at
          bs 16), and its arg-max is the op's own rounding of 2 s + const(r):
          equal to the bit-exact indices except at rounding-level ties.
  "torch" accepted for config compatibility; runs the fused HIP path (the
          indices are those of the reference's torch backend, bit for bit).
There is no CPU implementation in this package: tensors must live on a HIP
device (``pit_hip._lib`` raises otherwise).
"""
from __future__ import annotations

import math
import os
from typing import Sequence

import torch
import torch.nn as nn
from torch.distributions import Normal

from .. import _lib
from ._fused import axis_view, format_view, mu_shape, positions_view, train_fused


def prior_samples(n_samples: int, n_variable: int, seed_rec: int) -> torch.Tensor:
    """Scrambled-Sobol points mapped through the normal quantile (gaussian.py:15-19).

    Third-party arithmetic (torch SobolEngine + scipy ``norm.ppf``), called the
    same way as the reference so the codebook is identical (sha256 pinned in
    tests/golden)."""
    from scipy.stats import norm
    from torch.quasirandom import SobolEngine

    sobol = SobolEngine(n_variable, scramble=True, seed=seed_rec)
    return torch.from_numpy(norm.ppf(sobol.draw(n_samples)))


def _kl_bits(mu: torch.Tensor, var: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
    return 1.4426 * 0.5 * (torch.pow(mu, 2) + var - 1.0 - logvar)


class _GaussTrainFn(torch.autograd.Function):
    """One forward library call and one backward library call for the train-mode step of both regularizers.

    ``run(zv, noise, lam_state) -> (zhat, zhat_noquant or None, std or None, scalars, extra tensors)`` is the class's forward call
    (it advances ``lam_state`` on the device); ``bw`` holds what gq_gauss_backward_f32 needs besides the tensors.  Differentiable
    outputs: zhat (unless bw["zhat_diff"] is False: then it holds codewords), zhat_noquant, std, kl_loss; ``scalars`` (64 bytes:
    the statistics and the lambdas after the update) and ``extra`` are not.  Saved: z, the noise and a device copy of the lambdas
    taken BEFORE the call -- the backward recomputes each row's KL bits and with them its weight, nothing per row is kept."""

    @staticmethod
    def forward(ctx, zv, noise, lam_state, run, bw):
        lam_before = lam_state.clone()                      # a device copy, not a read
        zhat, noquant, std, scalars, extra = run(zv, noise, lam_state)
        kl_loss = scalars[:16].view(torch.float32)[0].clone()
        ctx.bw = bw
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(zv, noise, lam_before)
        ctx.mark_non_differentiable(scalars, *extra, *(() if bw["zhat_diff"] else (zhat,)))
        return (zhat, noquant, std, kl_loss, scalars) + tuple(extra)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_zhat, g_noquant, g_std, g_kl, *_):
        zv, noise, lam_before = ctx.saved_tensors
        bw = ctx.bw
        grad_z = _lib.gq_gauss_backward(zv, bw["dim"], bw["layout"], bw["grouping"], noise, lam_before, bw["log2n"],
                                        bw["tolerance"], bw["divisor"], g_zhat=g_zhat if bw["zhat_diff"] else None,
                                        g_zhat_noquant=g_noquant, g_std=g_std, g_kl=g_kl, lv_range=bw["lv_range"])
        return grad_z, None, None, None, None


class _GaussianQuantBase(nn.Module):
    def _setup(self, n_samples: int, dim: int, seed: int, beta: float, backend: str,
               logvar_range: Sequence[float], tolerance: float, lam_factor: float, lam_range) -> None:
        self.n_samples = n_samples
        self.log_n_samples = int(math.log(n_samples, 2))
        self.logvar_range = logvar_range
        self.lam_factor, self.tolerance = lam_factor, tolerance
        # lam / lam_min / lam_max (gaussian.py:41-43): Python floats in the reference.  Here properties over a host copy AND a
        # float64 [3] device copy: the fused eval forward of GaussianQuantRegularizer2 advances the device copy inside its launches
        # (no host read per forward); reading an attribute pulls the device copy once, writing one makes the host copy authoritative.
        self._lam_host = [1.0, 1.0, 1.0]
        self._lam_dev = None          # float64 [3] on the module's device, or None
        self._lam_dev_newer = False   # the device copy has advanced past the host copy
        self.lam_range = lam_range
        self.beta, self.seed = beta, seed
        self.register_buffer("prior_samples", prior_samples(n_samples, dim, seed).float(), persistent=False)
        self.normal_dist = Normal(torch.zeros([1, dim]), torch.ones([1, dim]))
        self.register_buffer("normal_log_prob", self.normal_dist.log_prob(self.prior_samples).float(),
                             persistent=False)
        self.perturbed = None
        if backend not in ("hip", "cuda", "cuda-compat", "torch"):
            raise ValueError(f"unknown backend {backend!r}")
        self.backend = backend
        self._ws = _lib.Workspace()   # scratch + the codebook cache (validated by the library against the codebook's content hash on every call)

    # ---- the adaptive lambda state --------------------------------------------------------------------------------------
    def _lam_pull(self) -> None:
        if self._lam_dev_newer:
            self._lam_host = [float(v) for v in self._lam_dev.cpu().tolist()]     # the one host read, only when somebody looks
            self._lam_dev_newer = False

    def _lam_get(self, i: int) -> float:
        self._lam_pull()
        return self._lam_host[i]

    def _lam_set(self, i: int, v) -> None:
        self._lam_pull()
        self._lam_host[i] = float(v)
        self._lam_dev = None          # re-uploaded by the next fused forward

    lam = property(lambda self: self._lam_get(0), lambda self, v: self._lam_set(0, v))
    lam_min = property(lambda self: self._lam_get(1), lambda self, v: self._lam_set(1, v))
    lam_max = property(lambda self: self._lam_get(2), lambda self, v: self._lam_set(2, v))

    def _lam_state_on(self, device) -> torch.Tensor:
        """The device copy of (lam, lam_min, lam_max), current; the caller's launch advances it in place."""
        if self._lam_dev is None or self._lam_dev.device != device:
            self._lam_pull()
            self._lam_dev = torch.tensor(self._lam_host, dtype=torch.float64, device=device)
        self._lam_dev_newer = True
        return self._lam_dev

    def _compat(self) -> bool:
        """True when the caller asked for the score-matrix call sequence instead of the fused kernels."""
        return self.backend == "cuda-compat" or (self.backend == "cuda" and os.environ.get("GQHIP_COMPAT", "0") == "1")

    # the reference's "cuda" call sequence on rows (gaussian.py:124-133 / :289-298)
    def _compat_rows(self, mu: torch.Tensor, std: torch.Tensor, dim: int):
        import gq_cuda

        if self.perturbed is None or self.perturbed.shape[0] != mu.shape[0] or self.perturbed.device != mu.device:
            self.perturbed = torch.zeros([mu.shape[0], self.n_samples], device=mu.device).contiguous()
        gq_cuda.ops.gq_cuda(mu, std, self.prior_samples, self.perturbed, dim, mu.shape[0], self.n_samples, self.beta)
        indices = torch.argmax(self.perturbed, dim=1).clone()
        return torch.index_select(self.prior_samples, 0, indices), indices

    def _update_lambdas(self, kl2_mean, kl2_min, kl2_max, buggy_lam_max: bool) -> None:
        # gaussian.py:103-117 (GQ1) / :238-252 (GQ2, whose lam_max decrease is a no-op: line 251)
        n, tol, f = self.log_n_samples, self.tolerance, self.lam_factor
        self.lam = self.lam * f if kl2_mean > n else self.lam / f
        if kl2_max > n + tol:
            self.lam_max = self.lam_max * f
        elif not buggy_lam_max:
            self.lam_max = self.lam_max / f
        self.lam_max = max(min(self.lam_max, self.lam_range[1]), 1.0)
        self.lam_min = self.lam_min / f if kl2_min < n - tol else self.lam_min * f
        self.lam_min = max(min(self.lam_min, 1.0), self.lam_range[0])

    def _weighted_kl(self, kl2: torch.Tensor) -> torch.Tensor:
        n, tol = self.log_n_samples, self.tolerance
        ge = (kl2 > n + tol).type(kl2.dtype) * self.lam_max
        eq = (kl2 <= n + tol).type(kl2.dtype) * (kl2 >= n - tol).type(kl2.dtype)
        le = (kl2 < n - tol).type(kl2.dtype) * self.lam_min
        return ge * kl2 + eq * kl2 + le * kl2


class GaussianQuantRegularizer(_GaussianQuantBase):
    """train(): Gaussian VAE sample + KL-to-log2(N) loss; eval(): VQ with the fixed
    quasi-random codebook (reference gaussian.py:22-178)."""

    def __init__(self, format, n_samples, group=1, logvar_range=[-30.0, 20.0], tolerance=0.5, lam_factor=1.01,
                 seed=42, beta=1.0, backend="hip"):
        super().__init__()
        assert format in ["bchw", "blc"]
        self.format, self.group = format, group
        self._setup(n_samples, group, seed, beta, backend, logvar_range, tolerance, lam_factor, (1e-3, 1e3))

    def _forward_fused(self, z):
        """Eval branch (gaussian.py:120-160) as ONE call: chunk / clamp / exp, the group permutes, zhat_noquant, the
        rows x n score matrix, arg-max and gather all happen inside libgqhip's three launches.  A channels_last z
        (what the NHWC conv stack hands over) is read, and zhat / indices / zhat_noquant are written, in that memory
        layout directly (_fused.format_view), so nothing is transposed."""
        z = z.float()
        assert z.dim() == (4 if self.format == "bchw" else 3)
        zv, layout, restore = format_view(z, self.format)
        # one draw of the size of mu (advances the generator like gaussian.py:121)
        noise = torch.randn(mu_shape(zv, layout), dtype=torch.float32, device=z.device)
        indices, zhat, zhat_noquant = _lib.gq_quantize_z(zv, self.prior_samples, self.group, layout, _lib.GQHIP_GROUP_STRIDED,
                                                         self.logvar_range, self.beta, self._ws, noise=noise)
        return restore(zhat), {"indices": restore(indices), "zhat_noquant": restore(zhat_noquant)}

    def _forward_train_fused(self, z):
        """Train branch (gaussian.py:77-119) as ONE forward library call (gq_gauss_train_f32: sample, per-row KL bits, statistics,
        re-weighted loss, lambda update on the device) and, under autograd, ONE backward call.  The noise is one torch.randn draw in
        the shape and memory layout of zhat.  info keeps the reference's keys: kl_loss (0-d fp32, carries grad), bits-mean / -min /
        -max (0-d fp32, detached: INTEGRATION.md), lam (0-d fp32, the value after the update).  Nothing is read back: m.lam,
        m.lam_min, m.lam_max pull the device state when somebody looks."""
        z = z.float()
        assert z.dim() == (4 if self.format == "bchw" else 3)
        zv, layout, restore = format_view(z, self.format)
        b = z.shape[0]
        noise = torch.randn(mu_shape(zv, layout), dtype=torch.float32, device=z.device)

        def run(zv_, noise_, lam_state):
            zhat, _, _, sc = _lib.gq_gauss_train(zv_, self.group, layout, _lib.GQHIP_GROUP_STRIDED, noise_, lam_state,
                                                 self.log_n_samples, self.tolerance, self.lam_factor, self.lam_range,
                                                 lam_max_decreases=True, loss_divisor=b, lv_range=self.logvar_range)
            return zhat, None, None, sc, ()

        bw = {"dim": self.group, "layout": layout, "grouping": _lib.GQHIP_GROUP_STRIDED, "log2n": self.log_n_samples,
              "tolerance": self.tolerance, "divisor": b, "lv_range": tuple(self.logvar_range), "zhat_diff": True}
        zhat, _, _, kl_loss, sc = _GaussTrainFn.apply(zv, noise, self._lam_state_on(z.device), run, bw)
        f32, f64 = sc[:16].view(torch.float32), sc[32:56].view(torch.float64)
        info = {"kl_loss": kl_loss, "bits-mean": f32[1], "bits-min": f32[2], "bits-max": f32[3],
                "lam": f64[0].to(torch.float32)}
        return restore(zhat), info

    def forward(self, z):
        if not self.training and not self._compat():
            return self._forward_fused(z)
        if self.training and z.is_cuda and z.numel() > 0 and train_fused():
            return self._forward_train_fused(z)
        z = z.float()
        if self.format == "bchw":
            b, c2, h, w = z.shape
            l = h * w
            zf = z.reshape(b, c2, l).transpose(1, 2)  # b (h w) c, a view
        else:
            b, l, c2 = z.shape
            zf = z
        c = c2 // 2
        mu, logvar = zf.chunk(2, 2)
        logvar = torch.clamp(logvar, self.logvar_range[0], self.logvar_range[1])
        std = torch.exp(0.5 * logvar)

        if self.training:
            var = torch.exp(logvar)
            zhat = mu + torch.randn_like(mu) * std
            kl2 = _kl_bits(mu, var, logvar).reshape(b, l, self.group, c // self.group).sum(dim=2)
            kl2_mean, kl2_min, kl2_max = torch.mean(kl2), torch.min(kl2), torch.max(kl2)
            kl_loss = torch.sum(self._weighted_kl(kl2), dim=[1, 2])
            kl_loss = torch.sum(kl_loss) / kl_loss.shape[0] * self.lam
            self._update_lambdas(kl2_mean, kl2_min, kl2_max, buggy_lam_max=False)
            if self.format == "bchw":
                zhat = zhat.transpose(1, 2).reshape(b, c, h, w)
            info = {"kl_loss": torch.mean(kl_loss), "bits-mean": kl2_mean, "bits-min": kl2_min,
                    "bits-max": kl2_max, "lam": torch.zeros_like(kl_loss) + self.lam}
            return zhat, info

        # backend "cuda-compat": the reference's own call sequence (score matrix -> argmax -> index_select)
        zhat_noquant = mu + torch.randn_like(mu) * std  # consumes RNG in eval, like gaussian.py:121
        k = c // self.group
        mu_r = mu.reshape(b, l, self.group, k).permute(0, 1, 3, 2).reshape(-1, self.group)
        std_r = std.reshape(b, l, self.group, k).permute(0, 1, 3, 2).reshape(-1, self.group)
        zq, ind = self._compat_rows(mu_r.contiguous(), std_r.contiguous(), self.group)
        zhat = zq.reshape(b, l, k, self.group).permute(0, 1, 3, 2).reshape(b, l, c).float()
        indices = ind.reshape(b, l, k)
        if self.format == "bchw":
            zhat = zhat.transpose(1, 2).reshape(b, c, h, w)
            indices = indices.transpose(1, 2).reshape(b, k, h, w)
            zhat_noquant = zhat_noquant.transpose(1, 2).reshape(b, c, h, w)
        return zhat, {"indices": indices, "zhat_noquant": zhat_noquant}

    def dequant(self, indices):
        return _lib.gq_dequant(indices, self.prior_samples, self.group, self.format, _lib.GQHIP_GROUP_STRIDED)


class GaussianQuantRegularizer2(_GaussianQuantBase):
    """Contiguous-channel grouping, arbitrary channel axis, Gaussian + VQ branches mixed
    by a straight-through estimator (reference gaussian.py:181-362)."""

    def __init__(self, dim, codebook_size, dim_idx=1, logvar_range=[-30.0, 20.0], tolerance=0.5, lam_factor=1.01,
                 seed=42, beta=1.0, use_ste=True, backend="hip"):
        super().__init__()
        self.dim, self.dim_idx, self.use_ste = dim, dim_idx, use_ste
        self._setup(codebook_size, dim, seed, beta, backend, logvar_range, tolerance, lam_factor, (1e-7, 1e7))

    def _split(self, z):
        z = torch.movedim(z, self.dim_idx, -1)
        assert z.shape[-1] % (self.dim * 2) == 0
        z_shape = z.shape
        z = z.reshape(-1, z_shape[-1])
        mu, logvar = z.chunk(2, -1)
        logvar = torch.clamp(logvar, self.logvar_range[0], self.logvar_range[1])
        return z, z_shape, mu, logvar, torch.exp(0.5 * logvar)

    def _restore(self, t, z_shape):
        return torch.movedim(t.reshape(*z_shape[:-1], -1), -1, self.dim_idx)

    def quant_gaussian(self, z):
        z2, z_shape, mu, logvar, std = self._split(z)
        knum = z2.shape[-1] // (self.dim * 2)
        var = torch.exp(logvar)
        zhat = mu + torch.randn_like(mu) * std
        kl2 = _kl_bits(mu, var, logvar).reshape(-1, knum, self.dim).sum(dim=-1)
        kl2_mean, kl2_min, kl2_max = torch.mean(kl2), torch.min(kl2), torch.max(kl2)
        kl_loss = torch.mean(self._weighted_kl(kl2)) * self.lam
        self._update_lambdas(kl2_mean, kl2_min, kl2_max, buggy_lam_max=True)
        info = {"kl_loss": torch.mean(kl_loss), "bits-mean": kl2_mean, "bits-min": kl2_min, "bits-max": kl2_max,
                "lam-min": self.lam_min, "lam-max": self.lam_max, "lam": self.lam,
                "mu": self._restore(mu, z_shape), "std": self._restore(std, z_shape),
                "zhat_noquant": self._restore(zhat, z_shape)}
        return info["zhat_noquant"], info

    def quant_vq(self, z):
        z2, z_shape, mu, _, std = self._split(z.float())
        knum = z2.shape[-1] // (self.dim * 2)
        if self._compat():
            zq, ind = self._compat_rows(mu.reshape(-1, self.dim).contiguous(), std.reshape(-1, self.dim).contiguous(),
                                        self.dim)
            zhat = zq.reshape(-1, knum * self.dim).float()
            indices = ind.reshape(-1, knum)
        else:
            # rows are already "position-major, channel-last": one BLC image of L = #positions
            ind, zq = _lib.gq_quantize_z(z2.contiguous()[None], self.prior_samples, self.dim, "blc",
                                         _lib.GQHIP_GROUP_CONTIGUOUS, self.logvar_range, self.beta, self._ws)
            zhat, indices = zq[0], ind[0]
        zhat = self._restore(zhat, z_shape)
        indices = self._restore(indices, z_shape)
        return zhat, {"indices": indices, "zhat_quant": zhat}

    def _forward_fused(self, z, autograd=False):
        """Eval forward (gaussian.py:333-345) as ONE library call: quant_gaussian's sample, statistics, re-weighted loss and lambda
        update, quant_vq's arg-max and gather, and the straight-through mix all happen in gq_quantize_z_gauss_f32's launches.  The
        lambda state advances on the device: info["lam"], ["lam-min"], ["lam-max"] are 0-d float64 device tensors (float(...) gives
        the reference's Python floats) and nothing is read back unless an attribute is inspected.
        ``autograd``: the same call behind _GaussTrainFn, whose backward is ONE gq_gauss_backward_f32 call: zhat (with use_ste:
        (g - g) + v, whose gradient goes to the Gaussian sample), info["zhat_noquant"], info["std"] and info["kl_loss"] are its
        differentiable outputs, info["mu"] stays the differentiable view of z; without use_ste in eval zhat holds codewords and
        nothing flows through it.  The noise is one torch.randn draw in the shape and memory layout of zhat."""
        z = z.float()
        assert z.shape[self.dim_idx] % (self.dim * 2) == 0
        zv, layout, restore = axis_view(z, self.dim_idx)
        # one draw of the size of mu (gaussian.py:222)
        noise = torch.randn(mu_shape(zv, layout), dtype=torch.float32, device=z.device)

        def run(zv_, noise_, lam_state):
            ind, zhat, zq, noq, std, sc = _lib.gq_quantize_z_gauss(
                zv_, self.prior_samples, self.dim, layout, _lib.GQHIP_GROUP_CONTIGUOUS, noise_, lam_state,
                self.log_n_samples, self.tolerance, self.lam_factor, self.lam_range, lam_max_decreases=False, use_ste=self.use_ste,
                lv_range=self.logvar_range, beta=self.beta, ws=self._ws)
            return zhat, noq, std, sc, ((ind, zq) if self.use_ste else (ind,))      # without use_ste zq IS zhat

        if autograd:
            bw = {"dim": self.dim, "layout": layout, "grouping": _lib.GQHIP_GROUP_CONTIGUOUS, "log2n": self.log_n_samples,
                  "tolerance": self.tolerance, "divisor": zv.numel() // (2 * self.dim), "lv_range": tuple(self.logvar_range),
                  "zhat_diff": bool(self.use_ste)}
            zhat, noq, std, kl_loss, sc, ind, *rest = _GaussTrainFn.apply(zv, noise, self._lam_state_on(z.device), run, bw)
        else:
            zhat, noq, std, sc, (ind, *rest) = run(zv, noise, self._lam_state_on(z.device))
            kl_loss = sc[:16].view(torch.float32)[0]
        zq = rest[0] if rest else zhat
        f32, f64 = sc[:16].view(torch.float32), sc[32:56].view(torch.float64)
        zhat_o = restore(zhat)                    # with use_ste the kernels stored (zhat_g - zhat_g) + zhat_v here
        d = self.dim_idx % z.dim()
        info = {"kl_loss": kl_loss, "bits-mean": f32[1], "bits-min": f32[2], "bits-max": f32[3],
                "lam-min": f64[1], "lam-max": f64[2], "lam": f64[0],
                "mu": z.narrow(d, 0, z.shape[d] // 2), "std": restore(std), "zhat_noquant": restore(noq),
                "indices": restore(ind), "zhat_quant": restore(zq)}
        if not self.use_ste and self.training:
            return info["zhat_noquant"], info
        return zhat_o, info

    def forward(self, z):
        if z.is_cuda and not self._compat():
            if not (torch.is_grad_enabled() and z.requires_grad):
                return self._forward_fused(z)
            if train_fused() and z.numel() > 0:
                return self._forward_fused(z, autograd=True)
        zhat_g, info_g = self.quant_gaussian(z)
        with torch.no_grad():
            zhat_v, info_v = self.quant_vq(z)
        if self.use_ste:
            zhat = zhat_g - zhat_g.detach() + zhat_v
        else:
            zhat = zhat_g if self.training else zhat_v
        return zhat, info_g | info_v

    def dequant(self, indices):
        flat, layout, restore = positions_view(indices, self.dim_idx % indices.dim())
        return restore(_lib.gq_dequant(flat, self.prior_samples, self.dim, layout, _lib.GQHIP_GROUP_CONTIGUOUS))


class IdentityRegularizer(nn.Module):
    def forward(self, z):
        return z, dict()
