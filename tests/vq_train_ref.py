"""fp64 restatement of one train step of VQQuantizer (reference pit/quantization/vq.py:39-99) and of its gradients -- the checker
of tests/test_gpu_vq_train_step.py, proven on the CPU by tests/test_vq_train_host.py and used by
tests/golden/make_golden_vq_train.py to fill g24_vq_train_step.npz.  numpy only.

Item p = (b L + l) K + k holds the channels d K + k, d < dim, of position (b, l); idx_p is its code, e_p = emb[idx_p].  The scalar
loss that is differentiated:
    loss = sum(z_q * w) + g_loss * codebook_loss
    z_q  = z + (e - z).detach()                                   (value e up to one fp32 rounding; gradient straight to z)
    codebook_loss = a mean((e.detach() - z)^2) + b mean((e - z.detach())^2),  (a, b) = (1, beta) legacy | (beta, 1)
With N = z.size and gl = float32(g_loss) (a Python scalar times an fp32 tensor is an fp32 product):
    grad_z          = w + gl a 2 / N (z - e)
    grad_emb[j][d]  = sum over p with idx_p = j of gl b 2 / N (e_p[d] - z_p[d])
Next to every value comes the SUM OF THE ABSOLUTE VALUES of the terms it was added up from: errors are stated in units of 2^-24 of
that sum (tests/train_step_ref.py has the reasoning)."""
import numpy as np

U = 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def to_items(t, cfg):
    """A z-shaped array -> [items, dim] with item = (b L + l) K + k, and the function that undoes it."""
    t = np.asarray(t)
    dim, K = cfg["dim"], cfg["K"]
    if cfg["format"] == "bchw":
        b, c, h, w = t.shape
        x = t.reshape(b, c, h * w).transpose(0, 2, 1)              # b l c
    else:
        b, _, c = t.shape
        x = t
    lead = x.shape
    items = x.reshape(lead[0], lead[1], dim, K).transpose(0, 1, 3, 2).reshape(-1, dim)      # channel d K + k -> (k, d)

    def back(r):
        y = r.reshape(lead[0], lead[1], K, dim).transpose(0, 1, 3, 2).reshape(lead)
        return y.transpose(0, 2, 1).reshape(t.shape) if cfg["format"] == "bchw" else y
    return items, back


def idx_to_items(idx, cfg):
    """Indices in the module layout ([b, K, h, w] / [b, l, K]) -> [items]."""
    idx = np.asarray(idx)
    if cfg["format"] == "bchw":
        b, K = idx.shape[:2]
        return idx.reshape(b, K, -1).transpose(0, 2, 1).reshape(-1)
    return idx.reshape(-1)


def step(z, emb, idx, cfg, w=None, g_loss=0.0):
    """One step in fp64 from fp32 inputs and the indices (module layout).  Returns a dict: e (shape of z: the codewords), loss,
    grad_z / grad_z_abs (shape of z), grad_emb / grad_emb_abs ([n, dim])."""
    z64 = np.asarray(z, np.float64)
    emb64 = np.asarray(emb, np.float64)
    zi, back = to_items(z64, cfg)
    ii = idx_to_items(idx, cfg)
    e = emb64[ii]
    diff = zi - e
    N = float(z64.size)
    a, b = (1.0, f32(cfg["beta"])) if cfg["legacy"] else (f32(cfg["beta"]), 1.0)
    mean = float((diff * diff).sum() / N)
    gl = f32(g_loss)
    wz = np.zeros_like(z64) if w is None else np.asarray(w, np.float64)
    tz = back(gl * a * 2.0 / N * diff)
    te = gl * b * 2.0 / N * (-diff)
    ge, ge_abs = np.zeros_like(emb64), np.zeros_like(emb64)
    np.add.at(ge, ii, te)
    np.add.at(ge_abs, ii, np.abs(te))
    return {"e": back(e), "loss": a * mean + b * mean, "grad_z": wz + tz, "grad_z_abs": np.abs(wz) + np.abs(tz),
            "grad_emb": ge, "grad_emb_abs": ge_abs}


def loss64(z, emb, idx, cfg, w, g_loss):
    """The scalar loss above in fp64 with the indices frozen (for central differences)."""
    z64, emb64 = np.asarray(z, np.float64), np.asarray(emb, np.float64)
    zi, back = to_items(z64, cfg)
    e = emb64[idx_to_items(idx, cfg)]
    a, b = (1.0, f32(cfg["beta"])) if cfg["legacy"] else (f32(cfg["beta"]), 1.0)
    mean = ((zi - e) ** 2).sum() / float(z64.size)
    return (z64 * np.asarray(w, np.float64)).sum() + f32(g_loss) * (a + b) * mean       # (sum(z_q w): d z_q / d z = 1, d z_q / d e = 0)


def err_units(got, want, want_abs):
    """max |got - want| / (2^-24 sum |terms|) over the elements with a non-zero sum; elements without terms must be exact zeros."""
    got, want, want_abs = (np.asarray(a, np.float64) for a in (got, want, want_abs))
    live = want_abs > 0
    assert np.all(got[~live] == 0.0), "an element without terms is not exactly zero"
    return float((np.abs(got - want)[live] / (U * want_abs[live])).max()) if live.any() else 0.0


# the fixture's cases (tests/golden/make_golden_vq_train.py): the smallest shapes at which each piece can go wrong
CASES = {
    "bchw_d16_legacy": dict(format="bchw", dim=16, K=1, n=1024, shape=(2, 16, 8, 8), beta=0.25, legacy=True),
    "blc_d8_k2": dict(format="blc", dim=8, K=2, n=4096, shape=(2, 16, 16), beta=0.25, legacy=False),       # two sub-codebooks, one grad_emb
    "bchw_d4_k4_odd": dict(format="bchw", dim=4, K=4, n=16384, shape=(1, 16, 5, 5), beta=0.25, legacy=True),   # L % 4 != 0; dim 4, no cache
    "bchw_d16_crowded": dict(format="bchw", dim=16, K=1, n=256, shape=(3, 16, 12, 12), beta=0.25, legacy=True),  # 432 items on 256 codes
}
STEPS = 2
G_LOSS = (0.37, 1.3)
MIN_GAP = 1e-4          # every row's fp64 top-2 distance gap (the existing VQ parity rule)
