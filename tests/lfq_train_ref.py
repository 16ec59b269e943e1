"""fp64 restatement of one train step of LFQQuantizer (reference pit/quantization/lfq.py:56-76, 127-206) and of its gradient -- the
checker of tests/test_gpu_lfq_train_step.py, proven on the CPU by tests/test_lfq_train_host.py and used by
tests/golden/make_golden_lfq_train.py to fill g25_lfq_train_step.npz (make_golden_train_variants.py: g28).  numpy only.

Row r = (b L + l) nc + ci holds the d channels ci d + i of position (b, l); R rows, N = 2^d codes, T = 0.01, eps = 1e-5.  The scalar
loss that is differentiated:
    loss = sum(quantized * w) + g_aux * entropy_aux_loss + g_commit * commit_loss
    quantized = x + (q - x).detach(),  q = x > 0 ? 1 : -1                       (gradient straight to x)
    entropy_aux_loss = w_s * per_sample_entropy - w_b * codebook_entropy,   commit_loss = mean((x - q)^2)
``dense64`` states the entropies as the reference does, with the [R, N] logits; ``factorised64`` never builds them: the softmax
over the product codebook {-1,+1}^d is a product of d Bernoullis with p_i = sigma(400 x_i), so
    per_sample_entropy = mean_r sum_i H_b(r, i),                      H_b = log1p(e) + |s| e / (1 + e),  s = 400 x,  e = exp(-|s|)
    avg[u, v] = (1 / R) sum_r A_r[u] B_r[v]                           (A over the high dh = d - d // 2 bits, B over the low d // 2)
    codebook_entropy = -sum avg log(avg + eps)
    grad_x = w + g_commit 2 (x - q) / numel + g_aux 400 (w_s / R (-s p q) - w_b d codebook_entropy / d s)
    d codebook_entropy / d s_i = (1 / R) sum_u (G B_r)[u] A_r[u] (bit_i(u) ? q_i : -p_i),   G = -(log(avg + eps) + avg / (avg + eps))
Next to every value comes the SUM OF THE ABSOLUTE VALUES of the terms it was added up from: errors are stated in units of 2^-24 of
that sum (tests/train_step_ref.py has the reasoning)."""
import numpy as np

U = 2.0 ** -24
T = 0.01
EPS = 1e-5


def to_rows(t, cfg):
    """An x-shaped array -> [R, d] with row = (b L + l) nc + ci, and the function that undoes it."""
    t = np.asarray(t)
    d = cfg["d"]
    if cfg["format"] == "bchw":
        b, c = t.shape[:2]
        x = t.reshape(b, c, -1).transpose(0, 2, 1)                 # b l c
    else:
        x = t
    lead = x.shape

    def back(r):
        y = r.reshape(lead)
        return y.transpose(0, 2, 1).reshape(t.shape) if cfg["format"] == "bchw" else y
    return x.reshape(-1, d), back


def _prob(rows):
    """(s, p = sigma(s), q = sigma(-s), H_b) of [R, d] float64 values, each without cancellation."""
    s = 400.0 * rows
    a = np.abs(s)
    e = np.exp(-a)
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    p = np.where(s > 0, big, small)
    q = np.where(s > 0, small, big)
    return s, p, q, np.log1p(e) + a * e / (1.0 + e)


def _table(p, q, bits):
    """[R, 2^len(bits)]: entry u = prod over k of (bit_k(u) ? p[:, bits[k]] : q[:, bits[k]])."""
    t = np.ones((p.shape[0], 1))
    for i in bits:
        t = np.concatenate([t * q[:, i:i + 1], t * p[:, i:i + 1]], axis=1)
    return t


def _weights(cfg):
    """The two entropy weights as the fp64 reference run sees them: Python floats, not rounded to fp32."""
    return float(cfg.get("w_s", 1.0)), float(cfg.get("w_b", 1.0))


def _scalars(se, ce, ce_abs, commit, cfg):
    ws, wb = _weights(cfg)
    return {"per_sample_entropy": se, "per_sample_entropy_abs": se, "codebook_entropy": ce, "codebook_entropy_abs": ce_abs,
            "entropy_aux_loss": ws * se - wb * ce, "entropy_aux_loss_abs": abs(ws) * se + abs(wb) * ce_abs,
            "commit_loss": commit, "commit_loss_abs": commit}


def _commit(x64):
    q = np.where(x64 > 0, 1.0, -1.0)
    return q, float(((x64 - q) ** 2).sum() / x64.size)


def dense64(x, cfg):
    """The reference's formula with the [R, N] logits (only where R N 8 B is small).  Returns the four scalars and their abs sums."""
    x64 = np.asarray(x, np.float64)
    rows, _ = to_rows(x64, cfg)
    d = cfg["d"]
    codes = ((np.arange(1 << d)[:, None] >> np.arange(d)[None, :]) & 1) * 2.0 - 1.0          # bit i of code j (lfq.py:119-121)
    logits = 2.0 * rows @ codes.T / T
    shifted = logits - logits.max(axis=1, keepdims=True)
    logp = shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True))                       # log_softmax(. + eps): the shift cancels
    probs = np.exp(logp)
    avg = probs.mean(axis=0)
    t = avg * np.log(avg + EPS)
    se = float((-(probs * logp).sum(axis=1)).mean())
    return _scalars(se, float(-t.sum()), float(np.abs(t).sum()), _commit(x64)[1], cfg)


def factorised64(x, cfg, w=None, g_aux=0.0, g_commit=0.0):
    """One step in fp64 from fp32 inputs without the logits.  Returns the four scalars, ``avg`` [2^dh, 2^dl], ``grad_x`` and
    ``grad_x_abs`` (shape of x), each scalar with its ``_abs``."""
    x64 = np.asarray(x, np.float64)
    rows, back = to_rows(x64, cfg)
    R, d = rows.shape
    dl = d // 2
    lo, hi = list(range(dl)), list(range(dl, d))
    s, p, q, hb = _prob(rows)
    A, B = _table(p, q, hi), _table(p, q, lo)
    avg = A.T @ B / R
    t = avg * np.log(avg + EPS)
    qv, commit = _commit(x64)
    out = _scalars(float(hb.sum() / R), float(-t.sum()), float(np.abs(t).sum()), commit, cfg)
    G = -(np.log(avg + EPS) + avg / (avg + EPS))
    dce, dce_abs = np.zeros_like(rows), np.zeros_like(rows)
    for tab, other, g, bits in ((A, B, G, hi), (B, A, G.T, lo)):
        wt, wt_abs = (other @ g.T) * tab, (other @ np.abs(g).T) * tab                         # [R, entries]: (G B_r)[u] A_r[u]
        for k, i in enumerate(bits):
            setk = ((np.arange(tab.shape[1]) >> k) & 1).astype(bool)
            dce[:, i] = (wt[:, setk].sum(axis=1) * q[:, i] - wt[:, ~setk].sum(axis=1) * p[:, i]) / R
            dce_abs[:, i] = (wt_abs[:, setk].sum(axis=1) * q[:, i] + wt_abs[:, ~setk].sum(axis=1) * p[:, i]) / R
    ws, wb = _weights(cfg)
    ga, gc = float(g_aux), float(g_commit)
    w64 = np.zeros_like(x64) if w is None else np.asarray(w, np.float64)
    t_commit = gc * 2.0 * (x64 - qv) / x64.size
    t_sample = back(ga * 400.0 * ws / R * (-s * p * q))
    t_batch, t_batch_abs = back(-ga * 400.0 * wb * dce), back(abs(ga * 400.0 * wb) * dce_abs)
    out.update(avg=avg, grad_x=w64 + t_commit + t_sample + t_batch,
               grad_x_abs=np.abs(w64) + np.abs(t_commit) + np.abs(t_sample) + t_batch_abs)
    return out


def loss64(x, cfg, w, g_aux, g_commit, q):
    """The scalar loss above in fp64 with the signs ``q`` frozen (for central differences)."""
    x64 = np.asarray(x, np.float64)
    s = factorised64(x64, cfg)
    commit = ((x64 - q) ** 2).sum() / x64.size
    return (x64 * np.asarray(w, np.float64)).sum() + float(g_aux) * s["entropy_aux_loss"] + float(g_commit) * commit


def err_units(got, want, want_abs):
    """max |got - want| / (2^-24 sum |terms|) over the elements with a non-zero sum; elements without terms must be exact zeros."""
    got, want, want_abs = (np.asarray(a, np.float64) for a in (got, want, want_abs))
    live = want_abs > 0
    assert np.all(got[~live] == 0.0), "an element without terms is not exactly zero"
    return float((np.abs(got - want)[live] / (U * want_abs[live])).max()) if live.any() else 0.0


SCALARS = ("entropy_aux_loss", "per_sample_entropy", "codebook_entropy", "commit_loss")

# the fixture's cases (tests/golden/make_golden_lfq_train.py): the smallest shapes at which each piece can go wrong
CASES = {
    "bchw_256x2": dict(format="bchw", d=8, nc=2, shape=(2, 16, 8, 8), scale=1.0),                 # the shipped config; sigma(400 x) saturated
    "blc_65536x1": dict(format="blc", d=16, nc=1, shape=(1, 37, 16), scale=0.02),                 # live entropies, odd rows, 256 x 256 table
    "blc_32x3_odd": dict(format="blc", d=5, nc=3, shape=(2, 9, 15), scale=0.02, w_s=0.7, w_b=1.3, special=True),   # odd d, weights, x = 0, +-1e-4, +-50
    "bchw_2x16": dict(format="bchw", d=1, nc=16, shape=(1, 16, 3, 3), scale=0.02),                # d = 1: empty low half
    "bchw_4096x1_cl": dict(format="bchw", d=12, nc=1, shape=(1, 12, 5, 5), scale=0.02, channels_last=True),
}
G_AUX, G_COMMIT = 0.37, 1.3

# The kernel variants CASES never launches (fixture g28, tests/golden/make_golden_train_variants.py).  With dl = d // 2 and
# dh = d - dl the host picks lfq_bwd_kernel<MT>, MT = max(1, 2^dh / 32), and 64 x 64 forward tiles below d = 14, 128 x 128 from there.
# Rows: 70 = a partial 256-row chunk of the forward, one 64-row block of the backward and 6 rows; 300 = a whole chunk and 44 rows
# (a partial 32-row step), four whole backward blocks and one whose second wave is partly dead.
VARIANT_CASES = {
    "blc_d2": dict(format="blc", d=2, nc=1, shape=(1, 70, 2), scale=0.02),           # dh = dl = 1: two live entries per table, the rest padding
    "blc_d3x2": dict(format="blc", d=3, nc=2, shape=(1, 35, 6), scale=0.02),         # odd d below 5 with nc > 1: row -> (position, ci)
    "blc_d4": dict(format="blc", d=4, nc=1, shape=(1, 70, 4), scale=0.02),           # 4 x 4 entries in a 64 x 64 tile
    "blc_d6": dict(format="blc", d=6, nc=1, shape=(1, 70, 6), scale=0.02),           # k-table of 8: slots 3 and 4 of ck are padding
    "blc_d7": dict(format="blc", d=7, nc=1, shape=(1, 70, 7), scale=0.02),           # dh 4, dl 3: MT = 1, both passes generic
    "blc_d9": dict(format="blc", d=9, nc=1, shape=(1, 300, 9), scale=0.02),          # dh 5, dl 4: MT = 1 with kdim = 16, slot 4 of ck padded
    "blc_d10": dict(format="blc", d=10, nc=1, shape=(1, 300, 10), scale=0.02),       # dh = dl = 5: the 16-byte slab copy at MT = 1
    "blc_d11x2": dict(format="blc", d=11, nc=2, shape=(1, 150, 22), scale=0.02),     # lfq_bwd_kernel<2>, generic second pass, nc > 1
    "blc_d13": dict(format="blc", d=13, nc=1, shape=(1, 300, 13), scale=0.02),       # lfq_bwd_kernel<4>; forward grid 2 x 1 of 64 x 64
    "blc_d13x4": dict(format="blc", d=13, nc=4, shape=(1, 75, 52), scale=0.02, same_as="blc_d13"),    # the same memory, rows of 4
    "blc_d14": dict(format="blc", d=14, nc=1, shape=(1, 300, 14), scale=0.02),       # lfq_bwd_kernel<4>, both passes slab copies; 1 x 1 wide
    "blc_d15": dict(format="blc", d=15, nc=1, shape=(1, 300, 15), scale=0.02),       # lfq_bwd_kernel<8>, generic second pass; 2 x 1 wide
    "bchw_d13x4_cl": dict(format="bchw", d=13, nc=4, shape=(1, 52, 5, 5), scale=0.02, channels_last=True),     # the module's NHWC route
}


def variant(fix, tag, key):
    """Array ``key`` of a VARIANT_CASES case in g28.  A case with ``same_as`` views the other case's x, w and grad_x64."""
    cfg = VARIANT_CASES[tag]
    if "same_as" in cfg and key in ("x", "w", "grad_x64"):
        return fix[f"{cfg['same_as']}_{key}"].reshape(cfg["shape"])
    return fix[f"{tag}_{key}"]
