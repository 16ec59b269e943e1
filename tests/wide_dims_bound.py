"""Test infrastructure beside tests/f16_bound_model.py: the record check of tests/test_gpu_f16_bound.py with the bound coefficient as
an argument -- the wide route (gqhip.h: gqhip_set_wide_dims) charges its 128 products per value with a coefficient of its own, which
the caller reads from gqhip_debug_plan."""
import numpy as np

import f16_bound_model as M


def records_within_bound(ws, rows, n, dim, A, B, rs, cb, beta, mode, k):
    """max over (set, row) of |m1 - max_group f| / max_group E(j), E(j) = k u T_j + E_abs.  A, B, rs, cb: the operands at the FILTER dim
    (zero-padded where the call's dim is below it); `dim`: the call's.  The second and third values of a record travel as fp16 gaps
    below m1, rounded towards zero (csrc/gq_common.h:Rec): what the re-rank reconstructs must never be below the group's true maximum
    minus the same bound, and not above it by more than the gap's fp16 resolution."""
    from pit_hip import _lib

    pl = _lib.debug_plan(rows, n, dim)
    assert pl["bf16"] == 3 and pl["ef_coeff"] == int(k), pl
    m, ids = _lib.debug_records(ws, rows, n, dim)
    m = m.cpu().numpy().astype(np.float64)
    ids = ids.cpu().numpy()
    r = M.analyse(A, B, rs, cb, beta, mode, k=float(k))
    E = float(k) * M.U * r["T_j"] + r["E_abs"][:, None]
    gt = pl["gt"]
    q = np.arange(16 * gt)
    worst = 0.0
    ar = np.arange(rows)
    for s in range(pl["nsplit"]):
        for j in range(3):
            mk = m[s, :, j]
            ok_rec = np.isfinite(mk)
            gid = ids[s, :, j]
            tile = (gid >> 1)[:, None] * gt + (q >> 4)[None, :]
            code = tile * 32 + (q & 3)[None, :] + 8 * ((q & 15) >> 2)[None, :] + 4 * (gid & 1)[:, None]
            inside = code < n
            cc = np.minimum(code, n - 1)
            fg = np.where(inside, r["f"][ar[:, None], cc], -np.inf).max(1)
            Eg = np.where(inside, E[ar[:, None], cc], 0.0).max(1)
            sel = ok_rec & np.isfinite(fg)
            if j == 0:
                ratio = np.abs(mk - fg) / np.maximum(Eg, 1e-300)
                worst = max(worst, float(ratio[sel].max(initial=0.0)))
            else:
                gap = m[s, :, 0] - mk
                low = (fg - mk) / np.maximum(Eg, 1e-300)                   # <= 1: never below the filter's own value - bound
                assert float(low[sel].max(initial=0.0)) <= 1.0, (s, j, float(low[sel].max()))
                over = mk - fg - Eg - gap * 2.0 ** -9 - 2.0 ** -22 * np.abs(m[s, :, 0]) - 2.0 ** -24     # gap: fp16, 2^-24 floor
                assert float(over[sel].max(initial=-1.0)) <= 0.0, (s, j, float(over[sel].max()))
                assert (gap[ok_rec] >= 0).all()
    return worst
