"""fp64 restatement of one train step of BSQQuantizer (reference pit/quantization/bsq.py:14-37, 64-133) and of FSQQuantizer
(pit/quantization/fsq.py:6-9, 29-68) with their gradients -- the checker of tests/test_gpu_bsq_fsq_train_step.py, proven on the
CPU by tests/test_bsq_fsq_train_host.py and used by tests/golden/make_golden_bsq_fsq_train.py to fill g26 / g27 (and by
make_golden_train_variants.py to fill g29).  numpy only.

BSQ.  A position holds C = 16 d channels, channel i d + j = codebook i, bit plane j; M = B L 16.  The scalar loss differentiated:
    loss = sum(quantized * w) + g_aux * entropy_aux_loss
    n = ||x||_2, u = x / max(n, 1e-12), q = u > 0 ? 1 : -1, quantized = (u + (q - u).detach()) q_scale, q_scale = 1 / sqrt(C)
    s = -400 u / sqrt(C), p = sigma(s), h(p) = -p log(p + eps) - (1 - p) log(1 - p + eps), eps = 1e-5
    per_sample_entropy = (1 / M) sum h;  avg[j] = (mean p, mean 1 - p) over bit plane j;  codebook_entropy = -sum avg log(avg + eps)
    entropy_aux_loss = w_s per_sample_entropy - w_b codebook_entropy
    g_u = q_scale w + g_aux (-400 / sqrt(C)) p (1 - p) ((w_s / M) h'(p) - (w_b / M) A'_j)
    h'(p) = -log(p + eps) - p / (p + eps) + log(1 - p + eps) + (1 - p) / (1 - p + eps),  A'_j = the same at avg[j]
    grad_x = (g_u - u (u . g_u)) / n  when n >= 1e-12,  g_u / 1e-12 otherwise
FSQ.  Per channel with L levels (half_l, offset, shift are the reference's fp32 values, also in its fp64 run: ``levels`` is an int32
parameter that .double() leaves alone):
    grad_z = g (half_l / half_width) sech^2(z + shift)
Next to every value comes the SUM OF THE ABSOLUTE VALUES of the terms it was added up from: errors are stated in units of 2^-24 of
that sum (tests/train_step_ref.py has the reasoning)."""
import numpy as np

U = 2.0 ** -24
EPS = 1e-5
NORM_MIN = 1e-12


def to_pos(t, fmt):
    """An x-shaped array -> [P, C] with position p = b L + l, and the function that maps [P, any] back to the module shape."""
    t = np.asarray(t)
    if fmt == "bchw":
        b, c = t.shape[:2]
        x = t.reshape(b, c, -1).transpose(0, 2, 1)
    else:
        x = t
    lead = x.shape

    def back(r):
        y = r.reshape(lead[0], lead[1], -1)                        # any channel count: the indices come back this way too
        return y.transpose(0, 2, 1).reshape(t.shape[0], -1, *t.shape[2:]) if fmt == "bchw" else y
    return x.reshape(-1, x.shape[-1]), back


def _prob(s):
    """(p = sigma(s), 1 - p) without cancellation."""
    e = np.exp(-np.abs(s))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(s > 0, big, small), np.where(s > 0, small, big)


def _dh(p, om):
    """h'(p) and the sum of its |terms|."""
    t = (-np.log(p + EPS), -p / (p + EPS), np.log(om + EPS), om / (om + EPS))
    return t[0] + t[1] + t[2] + t[3], np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2]) + np.abs(t[3])


def _weights(cfg):
    return float(cfg.get("w_s", 1.0)), float(cfg.get("w_b", 1.0))


def bsq64(x, cfg, w=None, g_aux=0.0):
    """One BSQ step in fp64 from fp32 inputs.  Returns the three scalars (each with its ``_abs``), ``avg`` [d, 2], the fp64 ``u``,
    ``indices`` (module shape), ``grad_x`` and ``grad_x_abs`` (shape of x)."""
    x64 = np.asarray(x, np.float64)
    rows, back = to_pos(x64, cfg["format"])
    P, C = rows.shape
    d = cfg["d"]
    assert C == 16 * d
    M = P * 16.0
    n = np.sqrt((rows * rows).sum(axis=1, keepdims=True))
    u = rows / np.maximum(n, NORM_MIN)
    cs = -400.0 / np.sqrt(C)
    qs = 1.0 / np.sqrt(C)
    p, om = _prob(cs * u)
    tp, tq = p * np.log(p + EPS), om * np.log(om + EPS)
    se, se_abs = float(-(tp + tq).sum() / M), float((np.abs(tp) + np.abs(tq)).sum() / M)
    avg = np.stack([p.reshape(P, 16, d).sum(axis=(0, 1)) / M, om.reshape(P, 16, d).sum(axis=(0, 1)) / M], axis=-1)      # [d, 2]
    ta = avg * np.log(avg + EPS)
    ce, ce_abs = float(-ta.sum()), float(np.abs(ta).sum())
    ws, wb = _weights(cfg)
    out = {"per_sample_entropy": se, "per_sample_entropy_abs": se_abs, "codebook_entropy": ce, "codebook_entropy_abs": ce_abs,
           "entropy_aux_loss": ws * se - wb * ce, "entropy_aux_loss_abs": abs(ws) * se_abs + abs(wb) * ce_abs, "avg": avg, "u": back(u)}
    bits = (u > 0).reshape(P, 16, d)
    ind = np.zeros((P, d), np.int64)
    for i in range(16):
        ind = ind * 2 + bits[:, i, :]
    out["indices"] = back(ind)
    ga = float(g_aux)
    w64 = np.zeros_like(rows) if w is None else to_pos(np.asarray(w, np.float64), cfg["format"])[0]
    hp, hp_abs = _dh(p, om)
    Ap, Ap_abs = _dh(avg[:, 0], avg[:, 1])                                  # [d]
    Aj, Aj_abs = np.tile(Ap, 16)[None, :], np.tile(Ap_abs, 16)[None, :]     # channel i d + j -> plane j
    k = ga * cs * p * om
    gu = qs * w64 + k * ((ws / M) * hp - (wb / M) * Aj)
    gu_abs = np.abs(qs * w64) + np.abs(k) * ((abs(ws) / M) * hp_abs + (abs(wb) / M) * Aj_abs)
    dot, dot_abs = (u * gu).sum(axis=1, keepdims=True), (np.abs(u) * gu_abs).sum(axis=1, keepdims=True)
    big = n >= NORM_MIN
    nn = np.where(big, n, 1.0)
    grad = np.where(big, (gu - u * dot) / nn, gu / NORM_MIN)
    grad_abs = np.where(big, (gu_abs + np.abs(u) * dot_abs) / nn, gu_abs / NORM_MIN)
    out.update(grad_x=back(grad), grad_x_abs=back(grad_abs))
    return out


def bsq_loss64(x, cfg, w, g_aux):
    """The scalar loss above in fp64, without the constant of the detached branch (for central differences)."""
    s = bsq64(x, cfg)
    C = 16 * cfg["d"]
    return float((s["u"] * np.asarray(w, np.float64)).sum() / np.sqrt(C) + float(g_aux) * s["entropy_aux_loss"])


def fsq_consts(levels):
    """(half_l, offset, shift, half_width) per channel: the reference's fp32 values as float64."""
    lev = np.asarray(levels, np.int32)
    half_l = ((lev - 1).astype(np.float32) * np.float32(1 + 1e-3) / np.float32(2)).astype(np.float32)
    offset = np.where(lev % 2 == 0, np.float32(0.5), np.float32(0.0)).astype(np.float32)
    shift = np.arctanh((offset / half_l).astype(np.float32)).astype(np.float32)
    return half_l.astype(np.float64), offset.astype(np.float64), shift.astype(np.float64), (lev // 2).astype(np.float64)


def fsq64(z, levels, fmt, g=None):
    """FSQ in fp64 from fp32 inputs: ``bounded``, ``r`` = rint(bounded), ``zhat`` = r / half_width (all shape of z) and, with ``g``,
    ``grad_z`` and ``grad_z_abs`` = |g| (half_l / half_width) (1 + tanh^2): the unit the GPU test states errors in."""
    rows, back = to_pos(np.asarray(z, np.float64), fmt)
    half_l, offset, shift, hw = fsq_consts(levels)
    t = rows + shift[None, :]
    th = np.tanh(t)
    bounded = th * half_l - offset
    r = np.rint(bounded)
    out = {"bounded": back(bounded), "r": back(r), "zhat": back(r / hw), "half_width": hw}
    if g is not None:
        g64 = to_pos(np.asarray(g, np.float64), fmt)[0]
        e = np.exp(-2.0 * np.abs(t))
        sech2 = 4.0 * e / (1.0 + e) ** 2
        out["grad_z"] = back(g64 * (half_l / hw) * sech2)
        out["grad_z_abs"] = back(np.abs(g64) * (half_l / hw) * (1.0 + th * th))
    return out


def fsq_loss64(z, levels, fmt, g):
    """sum(g * bounded / half_width): the differentiable branch of round_ste (for central differences)."""
    s = fsq64(z, levels, fmt)
    rows, _ = to_pos(s["bounded"], fmt)
    return float((rows / s["half_width"] * to_pos(np.asarray(g, np.float64), fmt)[0]).sum())


def err_units(got, want, want_abs):
    """max |got - want| / (2^-24 sum |terms|) over the elements with a non-zero sum; elements without terms must be exact zeros."""
    got, want, want_abs = (np.asarray(a, np.float64) for a in (got, want, want_abs))
    live = want_abs > 0
    assert np.all(got[~live] == 0.0), "an element without terms is not exactly zero"
    return float((np.abs(got - want)[live] / (U * want_abs[live])).max()) if live.any() else 0.0


SCALARS = ("entropy_aux_loss", "per_sample_entropy", "codebook_entropy")
G_AUX = 0.37

# the fixtures' cases (tests/golden/make_golden_bsq_fsq_train.py): the smallest shapes at which each piece can go wrong
BSQ_CASES = {
    "bchw_d1": dict(format="bchw", d=1, shape=(2, 16, 8, 8), kind="randn", scale=1.0),                       # the shipped config
    "blc_d2_small": dict(format="blc", d=2, shape=(3, 37, 32), kind="randn", scale=0.02, w_s=0.7, w_b=1.3),  # 111 rows: no tile's multiple
    "blc_d3_special": dict(format="blc", d=3, shape=(2, 19, 48), kind="special", scale=1.0),                 # C no power of two; the clamp
    "bchw_d1_saturated": dict(format="bchw", d=1, shape=(2, 16, 8, 8), kind="positive", scale=1.0),          # every p ~ 1.4e-11
    "bchw_d1_cl": dict(format="bchw", d=1, shape=(2, 16, 8, 8), kind="randn", scale=1.0, channels_last=True),
}
# The "blc" kernel pairs BSQ_CASES never launches (fixture g29, tests/golden/make_golden_train_variants.py).  A row of C = 16 d
# floats is C4 = 4 d chunks of 16 bytes on 16 lanes, NS = ceil(d / 4) chunks per lane; 37 rows = two whole 16-row groups and 5 rows.
BSQ_VARIANT_CASES = {
    "blc_d5": dict(format="blc", d=5, shape=(1, 37, 80), kind="randn", scale=1.0),        # <16, 2>: 4 of 16 lanes live in chunk 2
    "blc_d6": dict(format="blc", d=6, shape=(1, 37, 96), kind="randn", scale=1.0),        # <16, 2>: 8 live
    "blc_d8": dict(format="blc", d=8, shape=(1, 37, 128), kind="randn", scale=1.0),       # <16, 2>: no idle lane
    "blc_d9": dict(format="blc", d=9, shape=(1, 37, 144), kind="randn", scale=1.0),       # <16, 3>: 4 live in chunk 3
    "blc_d10": dict(format="blc", d=10, shape=(1, 37, 160), kind="randn", scale=1.0),     # <16, 3>: 8 live
    "blc_d11": dict(format="blc", d=11, shape=(1, 37, 176), kind="randn", scale=1.0),     # <16, 3>: 12 live
    "blc_d12": dict(format="blc", d=12, shape=(1, 37, 192), kind="randn", scale=1.0),     # <16, 3>: no idle lane
    "blc_d13": dict(format="blc", d=13, shape=(1, 37, 208), kind="randn", scale=1.0),     # <16, 4>: 4 live in chunk 4
    "blc_d14": dict(format="blc", d=14, shape=(1, 37, 224), kind="randn", scale=1.0),     # <16, 4>: 8 live
    "blc_d15": dict(format="blc", d=15, shape=(1, 37, 240), kind="randn", scale=1.0),     # <16, 4>: 12 live
    "bchw_d9": dict(format="bchw", d=9, shape=(1, 144, 7, 11), kind="randn", scale=1.0),  # bchw at a d no power of two: 64 + 13 positions
    "bchw_d15": dict(format="bchw", d=15, shape=(2, 240, 3, 3), kind="randn", scale=1.0),       # two images in one block of 18 positions
    "bchw_d10_cl": dict(format="bchw", d=10, shape=(1, 160, 5, 7), kind="randn", scale=1.0, channels_last=True),   # <16, 3> from NHWC
}
BSQ_UNDERFLOW = dict(format="blc", d=1, shape=(1, 3, 16))       # forward only, stored fp32: row 1 holds 1e18, 1e-30, -1e-30 and zeros
FSQ_CASES = {
    "bchw_6": dict(format="bchw", levels=[8, 8, 8, 5, 5, 5], shape=(2, 6, 8, 8)),
    "bchw_6_cl": dict(format="bchw", levels=[8, 8, 8, 5, 5, 5], shape=(2, 6, 8, 8), channels_last=True),
    "blc_5": dict(format="blc", levels=[7, 5, 5, 5, 5], shape=(2, 19, 5)),
}
