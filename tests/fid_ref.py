"""What the FID tests share: the g32 fixtures (tests/golden/make_golden_fid.py), an independent numpy statement of the moments rule,
the derived bounds, and the stub model / extractor of the evaluate_sharded tests."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_FIXTURES = 5
F4_PARTS = 2          # the largest fixture's feature blocks are stored in halves: no committed file above 1 MiB


def load_fixtures():
    """[{x, y, mu_x, cov_x, mu_y, cov_y, fid}] of the five fixtures, reassembled from the files the generator wrote."""
    g = dict(np.load(os.path.join(G, "g32_fid.npz")))
    big = N_FIXTURES - 1
    for name in ("x", "y"):
        g[f"f{big}.{name}"] = np.concatenate([np.load(os.path.join(G, f"g32_fid_f{big}_{name}{h}.npz"))["rows"] for h in range(F4_PARTS)])
    packed = np.load(os.path.join(G, f"g32_fid_f{big}_cov.npz"))
    for name in ("cov_x", "cov_y"):
        D = g[f"f{big}.x"].shape[1]
        c = np.zeros((D, D))
        c[np.triu_indices(D)] = packed[name]             # the upper triangle, row by row; np.cov's result is symmetric bit for bit
        g[f"f{big}.{name}"] = c + np.triu(c, 1).T
    return [{k: g[f"f{i}.{k}"] for k in ("x", "y", "mu_x", "cov_x", "mu_y", "cov_y", "fid")} for i in range(N_FIXTURES)]


def moments_loop(x, state=None):
    """The rule in numpy, one row at a time: (outer [D, D], sum [D], count) in fp64.  np.outer's products of fp32 values are exact
    in fp64, so each += is one rounding."""
    D = x.shape[1]
    S, s, n = (np.zeros((D, D)), np.zeros(D), 0.0) if state is None else state
    for r in np.asarray(x, dtype=np.float64):
        S += np.outer(r, r)
        s += r
        n += 1.0
    return S, s, n


def split_state(state, D):
    """(outer [D, D], sum [D], count) views of a [D D + D + 1] state as numpy."""
    a = state.detach().cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
    return a[: D * D].reshape(D, D), a[D * D: D * D + D], float(a[-1])


def assert_state_bits(got, want, D, what=""):
    """The defined part of two states -- upper triangle of outer, sum, count -- bit for bit."""
    (S, s, n), (S0, s0, n0) = split_state(got, D), split_state(want, D)
    iu = np.triu_indices(D)
    assert np.array_equal(S[iu].view(np.int64), S0[iu].view(np.int64)), f"{what}: outer differs"
    assert np.array_equal(s.view(np.int64), s0.view(np.int64)), f"{what}: sum differs"
    assert n == n0, f"{what}: count {n} != {n0}"


def fid_scale(mu1, sigma1, mu2, sigma2):
    d = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(np.trace(sigma1) + np.trace(sigma2) + d.dot(d))


FID_RTOL = 1e-9       # |delta| <= FID_RTOL * fid_scale: five orders above the eigh route's own error, FID is read to four decimals


def numpy_fid(x, y):
    """The reference's formula on np.mean / np.cov(rowvar=False) of feature blocks x (inputs) and y (reconstructions), both in
    fp64 -> (fid, scale).  The formula is restated with scipy's sqrtm as pit/evaluations/fid/fid_score.py has it (main path)."""
    from scipy import linalg

    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m1, s1, m2, s2 = y.mean(0), np.cov(y, rowvar=False), x.mean(0), np.cov(x, rowvar=False)
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    assert np.isfinite(covmean).all()
    d = m1 - m2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean.real)), fid_scale(m1, s1, m2, s2)


# ---- evaluate_sharded: a stub model and a stub extractor that shows every feature block -------------------------------------------
class StubModel:
    """encode: indices from the image content; decode: a fixed distortion of the image, so the two feature sets differ."""

    def encode(self, x, return_reg_log=True):
        ids = (x[:, 0, 0, 0] * 1000).round().long().abs()
        tok = (ids[:, None] * 7 + torch.arange(4, device=x.device)[None]) % 65536
        return x, {"indices": tok.reshape(-1, 1, 2, 2)}

    def decode(self, z):
        return z * 0.9 + 0.02 * torch.sin(7.0 * z)


def stub_images(ids, hw=8):
    """[len(ids), 3, hw, hw] in [-1, 1], a function of the dataset index alone."""
    out = torch.empty(len(ids), 3, hw, hw)
    for k, i in enumerate(ids):
        out[k] = torch.rand(3, hw, hw, generator=torch.Generator().manual_seed(1000 + int(i))) * 2 - 1
    return out


class StubExtractor:
    """A fixed projection of the 2 x 2-pooled image followed by relu -> fp32 [B, D]; ``blocks`` keeps a host copy of every block it
    returned, in call order (inputs, reconstructions, inputs, ...)."""

    def __init__(self, D=8, spatial=False):
        self.proj = torch.randn(12, D, generator=torch.Generator().manual_seed(77)) * 0.5
        self.spatial = spatial
        self.blocks = []

    def __call__(self, images):
        pooled = torch.nn.functional.adaptive_avg_pool2d(images, (2, 2)).reshape(images.shape[0], -1)
        feats = torch.relu(pooled @ self.proj.to(images.device) + 0.3)
        self.blocks.append(feats.detach().cpu().numpy().copy())
        return feats[:, :, None, None] if self.spatial else feats

    def inputs(self):
        return np.concatenate(self.blocks[0::2])

    def reconstructions(self):
        return np.concatenate(self.blocks[1::2])
