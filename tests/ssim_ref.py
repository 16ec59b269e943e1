"""fp64 numpy restatement of the SSIM / MS-SSIM that pit/evaluations/ssim.py computes through pytorch_msssim (data_range 255,
size_average False): the fp32 Gaussian window and fp32-scaled inputs, everything after that in fp64.  The yardstick of
tests/test_ssim_host.py and tests/test_gpu_ssim.py."""
import numpy as np

C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
MS_WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float32).astype(np.float64)


def window32(size=11, sigma=1.5):
    """exp(-(k - size // 2)^2 / (2 sigma^2)) in fp32, divided by its fp32 sum (left to right)."""
    coords = np.arange(size, dtype=np.float32) - np.float32(size // 2)
    g = np.exp(-(coords * coords) / np.float32(2 * sigma ** 2)).astype(np.float32)
    s = np.float32(0)
    for v in g:
        s = np.float32(s + v)
    return (g / s).astype(np.float32)


def window64(size=11, sigma=1.5):
    k = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(k * k) / (2 * sigma ** 2))
    return g / g.sum()


def scale(x, zero_mean):
    """The wrapper's scaling, in fp32 like the reference."""
    x = np.asarray(x, dtype=np.float32)
    return (x + np.float32(1)) * np.float32(127.5) if zero_mean else x * np.float32(255)


def gfilter(x, w):
    """Valid separable filter over the last two axes: along H, then W; a side shorter than the window is left alone."""
    n = len(w)
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-2] >= n:
        h = x.shape[-2] - n + 1
        x = sum(float(w[k]) * x[..., k:k + h, :] for k in range(n))
    if x.shape[-1] >= n:
        v = x.shape[-1] - n + 1
        x = sum(float(w[k]) * x[..., k:k + v] for k in range(n))
    return x


def level(X, Y, w):
    """One scale: (ssim, cs) per (image, channel) and the maps."""
    mu1, mu2 = gfilter(X, w), gfilter(Y, w)
    s11 = gfilter(X * X, w) - mu1 * mu1
    s22 = gfilter(Y * Y, w) - mu2 * mu2
    s12 = gfilter(X * Y, w) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
    return ssim_map.mean(axis=(-2, -1)), cs_map.mean(axis=(-2, -1)), ssim_map


def pool(X):
    """avg_pool2d(kernel 2, stride 2, padding = side % 2, count_include_pad): zeros before an odd side, / 4."""
    ph, pw = X.shape[-2] % 2, X.shape[-1] % 2
    X = np.pad(X, [(0, 0)] * (X.ndim - 2) + [(ph, 0), (pw, 0)])
    h, w = X.shape[-2] // 2, X.shape[-1] // 2
    X = X[..., :2 * h, :2 * w]
    return (X[..., 0::2, 0::2] + X[..., 0::2, 1::2] + X[..., 1::2, 0::2] + X[..., 1::2, 1::2]) / 4


def ssim_msssim_scaled(X, Y, w=None):
    """X, Y: [B, C, H, W] already on the 0..255 scale.  Returns fp64 (ssim [B], ms_ssim [B]; NaN below 256 x 256)."""
    w = window32() if w is None else w
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    s0, cs, _ = level(X, Y, w)
    ssim = s0.mean(axis=1)
    if X.shape[-2] < 256 or X.shape[-1] < 256:
        return ssim, np.full_like(ssim, np.nan)
    vals = []
    for lv in range(5):
        s, cs, _ = level(X, Y, w)
        if lv < 4:
            vals.append(np.maximum(cs, 0))
            X, Y = pool(X), pool(Y)
        else:
            vals.append(np.maximum(s, 0))
    ms = np.prod([v ** MS_WEIGHTS[k] for k, v in enumerate(vals)], axis=0).mean(axis=1)
    return ssim, ms


def ssim_msssim(x, y, zero_mean=False, is_video=False, w=None):
    """get_ssim_and_msssim of pit/evaluations/ssim.py in fp64: x, y [B, C, H, W] (or [B, C, T, H, W] with is_video)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if is_video:
        per = [ssim_msssim_scaled(scale(x[:, :, t], zero_mean), scale(y[:, :, t], zero_mean), w) for t in range(x.shape[2])]
        return np.mean([p[0] for p in per], axis=0), np.mean([p[1] for p in per], axis=0)
    return ssim_msssim_scaled(scale(x, zero_mean), scale(y, zero_mean), w)
