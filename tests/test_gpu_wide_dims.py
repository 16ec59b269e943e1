"""-m gpu: the wide route of the codebook dims 33-64 (gqhip.h: gqhip_set_wide_dims; the fp16 filter and the re-rank run at dim 64,
dims 33-63 on zero-padded operands, the re-rank scores with the true dim).  The references are the C oracle (oracle/gq_oracle.py:
the reference's arg-max, pit/quantization/gaussian.py:142-150; VQ: vq.py:58-73) and the exhaustive route of the same build; every
comparison is bit for bit over every row, and every comparison first shows that the route ran: gqhip_filter_dim says 64 and the
profiling recorder saw a filter launch (the exhaustive kernel is never recorded).  Every test that flips the selection restores it."""
import contextlib

import numpy as np
import pytest
import torch

import f16_bound_model as M
from oracle import gq_oracle as O
from wide_dims_bound import records_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (33, 40, 48, 63, 64)
K_128_PRODUCTS = 16384 + 4 + 3 + 4 * 128


@contextlib.contextmanager
def route(kind):
    from pit_hip import _lib

    prev = _lib.get_wide_dims()
    _lib.set_wide_dims(kind)
    try:
        yield
    finally:
        _lib.set_wide_dims(prev)


@contextlib.contextmanager
def filter_launches():
    """box["n"]: launches the profiling recorder saw inside the block (it records the filter, never the exhaustive kernel)"""
    from pit_hip import _lib

    box = {}
    _lib.profile_enable(True)
    _lib.profile_collect()
    try:
        yield box
        torch.cuda.synchronize()
        box["n"] = _lib.profile_collect()[0]
    finally:
        _lib.profile_enable(False)


def _bits(t):
    """NaN-proof equality: compare the words"""
    return t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _both_routes(fn, n, dim):
    """fn() under EXHAUSTIVE and under FILTER, where the route is shown to run: (exhaustive outputs, filter outputs)"""
    from pit_hip import _lib

    with route("exhaustive"):
        assert _lib.filter_dim(n, dim) == 0
        with filter_launches() as none:
            e = fn()
    assert none["n"] == 0
    with route("filter"):
        assert _lib.filter_dim(n, dim) == 64, (n, dim)
        with filter_launches() as ran:
            p = fn()
    assert ran["n"] >= 1, "no filter launch: the call fell back to the exhaustive kernel"
    return e, p


def _gq_rows(kind, rows, dim, g):
    mu = torch.randn(rows, dim, generator=g)
    if kind == "flat":
        sd = torch.randn(rows, dim, generator=g).abs() + 0.5
    elif kind == "tiny-sd":             # the expansion cancels: the finish scan runs
        sd = torch.randn(rows, dim, generator=g).abs() + 1e-3
    elif kind == "trained":
        sd = torch.rand(rows, dim, generator=g) * 0.25 + 0.05
    else:
        sd = torch.rand(rows, dim, generator=g) * 0.9 + 0.05
    return mu, sd


def _check_rows(mu, sd, cb, beta, tag, given_logsd, ref=None):
    """FILTER = EXHAUSTIVE = oracle on idx and zhat; returns (oracle indices, rows the in-block scan finished on the filter route)"""
    from pit_hip import _lib

    n, dim = cb.shape
    mud, sdd, cbd = mu.to(DEV), sd.to(DEV), cb.to(DEV)
    lsd = O.torch_log(sd.numpy()) if given_logsd else np.log(sd.numpy().astype(np.float64)).astype(np.float32)
    if ref is None:
        ref = O.argmax_rows(mu.numpy(), sd.numpy(), cb.numpy(), beta, logstd=lsd)[0]
    lg = torch.from_numpy(lsd).to(DEV) if given_logsd else None
    ws = _lib.Workspace()
    (ie, ze), (ip, zp) = _both_routes(lambda: _lib.gq_argmax(mud, sdd, cbd, beta, logsd=lg, ws=ws), n, dim)
    assert np.array_equal(ie.cpu().numpy(), ref), (tag, "exhaustive vs oracle")
    assert torch.equal(ip, ie), (tag, int((ip != ie).sum()))
    assert _same(zp, ze) and torch.equal(zp, cbd[ip]), tag
    return ref, _lib.debug_counters(ws)[0]          # (of the filter call, the last one on ws)


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("rows,n", [(1, 64), (37, 96), (777, 4096 + 33)])
@pytest.mark.parametrize("dim", DIMS)
def test_rows_filter_equals_exhaustive_equals_oracle(dim, rows, n, beta):
    g = torch.Generator().manual_seed(1000 * dim + rows + int(beta * 8))
    cb = torch.randn(n, dim, generator=g)
    for kind, given in (("random", False), ("trained", True)):
        mu, sd = _gq_rows(kind, rows, dim, g)
        _check_rows(mu, sd, cb, beta, f"dim {dim} rows {rows} n {n} beta {beta} {kind}", given)


@pytest.mark.parametrize("dim", [40, 64])
def test_rows_at_the_full_codebook_size(dim):
    g = torch.Generator().manual_seed(dim)
    cb = torch.randn(65536, dim, generator=g)
    mu, sd = _gq_rows("trained", 300, dim, g)
    _check_rows(mu, sd, cb, 1.0, f"dim {dim} 300 rows x 65536 codes", True)


@pytest.mark.parametrize("dim", [40, 64])
def test_row_kinds(dim):
    """Trained-like rows, ill-conditioned rows (tiny sd), a duplicated winning code (the lowest index wins) and two codes that differ
    in the last bit of one coordinate.  (No row can reach the finish scan through its records here: at 4129 codes a record set holds
    two candidate groups, and a row is undecided only when a FOURTH group of one set is inside the margin.  The scan is driven by
    test_flat_rows_reach_the_finish_scan and by the non-finite rows.)"""
    rows, n, beta = 200, 4096 + 33, 1.0
    g = torch.Generator().manual_seed(77 + dim)
    cb = torch.randn(n, dim, generator=g)
    mu, sd = _gq_rows("trained", rows, dim, g)
    ref, _ = _check_rows(mu, sd, cb, beta, f"dim {dim} trained", False)
    mu_t, sd_t = _gq_rows("tiny-sd", 64, dim, g)
    _check_rows(mu_t, sd_t, cb, beta, f"dim {dim} tiny sd", True)
    # the winners once more at the end of the codebook: the first index must win
    cb2 = cb.clone()
    winners = np.unique(ref[ref < n // 2])[: n // 8]
    cb2[n - len(winners):] = cb[torch.from_numpy(winners)]
    hit = np.isin(ref, winners)
    assert hit.any()
    ref2, _ = _check_rows(mu, sd, cb2, beta, f"dim {dim} duplicated winners", False)
    assert (ref2[hit] < n - len(winners)).all()
    # each of the first rows' winners again, one ulp away in one coordinate (up for even rows, down for odd ones)
    cb3 = cb.clone()
    for r in range(32):
        twin = cb[ref[r]].clone()
        c = (7 * r) % dim
        twin[c] = torch.nextafter(twin[c], torch.tensor(float("inf") if r % 2 == 0 else float("-inf")))
        cb3[n - 1 - r] = twin
    _check_rows(mu, sd, cb3, beta, f"dim {dim} last-bit twins", False)


@pytest.mark.parametrize("dim", [40, 64])
def test_flat_rows_reach_the_finish_scan(dim):
    """Flat rows (sd = |randn| + 0.5): FILTER = EXHAUSTIVE = oracle, and some of them are finished by the re-rank's in-block scan, at
    the true dim.  A row is undecided when the FOURTH candidate group of one record set is inside the margin of the row's maximum, so
    the shape must give a set at least four groups -- 65 576 codes: 68 tiles = 17 groups of 128 codes per split (4129 codes: two
    groups per set, no fourth) -- and the codebook must put four of them that close: every run of 1024 codes is eight copies of one
    block of 128, each copy perturbed in its last three bits (relative 2^-21, far inside the margin, whose E_r share alone is
    80 u G with G in the hundreds).  Whichever block holds a row's best code, its copies are seven more groups of the same lane half,
    at least four of them in the same split.  The copies also make the scan decide between near-ties by the reference's arithmetic
    and the lowest index."""
    n, beta, rows = 65536 + 40, 1.0, 64
    g = torch.Generator().manual_seed(177 + dim)
    base = torch.randn(n, dim, generator=g)
    j = torch.arange(n)
    cb = base[(j // 1024) * 1024 + j % 128].clone()          # (the 40 codes behind the last whole run copy themselves)
    cb = cb * (1.0 + 2.0 ** -21 * torch.randint(-4, 5, (n, dim), generator=g).float())
    mu_f, sd_f = _gq_rows("flat", rows, dim, g)
    _, fb_flat = _check_rows(mu_f, sd_f, cb, beta, f"dim {dim} flat", False)
    print(f"dim {dim}: flat rows finished by the in-block scan: {fb_flat} of {rows}")
    assert fb_flat >= 1, "no flat row reached the finish scan"


@pytest.mark.parametrize("dim", [40, 64])
def test_non_finite_rows_equal_the_exhaustive_route(dim):
    """Seven special rows among 64 ordinary ones; then a NaN code; then a NaN beta on its own call."""
    from pit_hip import _lib

    g = torch.Generator().manual_seed(50 + dim)
    n = 4096 + 33
    cb = torch.randn(n, dim, generator=g)
    mu, sd = torch.randn(71, dim, generator=g), torch.rand(71, dim, generator=g) * 0.6 + 0.2
    at = [3, 11, 19, 27, 35, 43, 51]
    mu[at[0], 1] = float("nan")
    sd[at[1], 2] = 0.0
    sd[at[2], 0] = float("inf")
    mu[at[3], dim - 1] = float("inf")
    mu[at[4], 0] = float("-inf")
    sd[at[5], 3] = -0.5
    sd[at[6], dim - 1] = float("nan")
    cb_nan = cb.clone()
    cb_nan[1234, dim - 1] = float("nan")
    for tag, book, beta in (("special rows", cb, 1.0), ("special rows, beta 0.25", cb, 0.25), ("a NaN code", cb_nan, 1.0),
                            ("a NaN beta", cb, float("nan"))):
        for given in (None, torch.log(sd)):
            ws = _lib.Workspace()
            lg = None if given is None else given.to(DEV)
            (ie, ze), (ip, zp) = _both_routes(lambda: _lib.gq_argmax(mu.to(DEV), sd.to(DEV), book.to(DEV), beta, logsd=lg, ws=ws), n, dim)
            assert torch.equal(ip, ie), (tag, given is not None, ip[at].tolist(), ie[at].tolist())
            assert _same(zp, ze), tag
            fb = _lib.debug_counters(ws)[0]                     # (of the filter call, the last one on ws)
            assert fb >= (71 if tag in ("a NaN code", "a NaN beta") else 4), (tag, fb)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -8, 200.0])
@pytest.mark.parametrize("dim", [40, 64])
def test_vq_filter_equals_exhaustive_equals_oracle(dim, scale):
    from pit_hip import _lib

    rows, n = 777, 4096 + 33
    g = torch.Generator().manual_seed(7 * dim + int(scale))
    emb = torch.randn(n, dim, generator=g)
    z = torch.randn(rows, dim, generator=g)
    # an exact tie between two codes: +-w around z = 0, both nearer than any other code; and a duplicated code
    emb[3000], emb[17] = torch.full((dim,), 2.0 ** -10), torch.full((dim,), -(2.0 ** -10))
    z[5] = 0.0
    emb[4000] = emb[100]
    z[6] = emb[100]
    emb, z = emb * scale, z * scale
    ws = _lib.Workspace()
    (ie, ze), (ip, zp) = _both_routes(lambda: _lib.vq_argmin(z.to(DEV), emb.to(DEV), ws=ws), n, dim)
    ref = O.vq_argmin_rows(z.numpy(), emb.numpy())
    assert np.array_equal(ie.cpu().numpy(), ref)
    assert torch.equal(ip, ie) and _same(zp, ze)
    assert int(ip[5]) == 17 and int(ip[6]) == 100


@pytest.mark.parametrize("scale,beta", [(2.0 ** -8, 1.0), (16.0, 0.25), (254.9, 1.0)])
@pytest.mark.parametrize("dim", [40, 64])
def test_bound_attack_at_wide_dims(dim, scale, beta):
    """The constructed operand sets of tests/f16_bound_model.py at the TRUE dim: the indices equal the oracle's, and every record the
    filter left is within the bound the plan charges (its coefficient read from gqhip_debug_plan) -- the model evaluates filter, sums
    and bound on the operands the kernels saw, zero-padded to dim 64 (mu 0, sd 1, code 0 in the pad columns)."""
    from pit_hip import _lib

    rng = np.random.default_rng(41 * dim + int(scale * 3) + int(beta * 7))
    n, rows, dp = 2048, 256, 64
    cb = M.codebooks(rng, n, dim, scale)
    cbd = torch.from_numpy(cb).to(DEV)
    pad = lambda a, v: np.concatenate([a, np.full((a.shape[0], dp - dim), v, np.float32)], 1)
    for name, (A0, B0) in M.coefficient_sets(rng, rows, dim, beta, cb).items():
        mu, sd = M.rows_from_coefficients(A0, B0, beta)
        A, B, rs = M.coefficients(pad(mu, 0.0), pad(sd, 1.0), beta)
        ok = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(rs).all(1) & (sd > 0).all(1)
        mu, sd, A, B, rs = mu[ok], sd[ok], A[ok], B[ok], rs[ok]
        lsd = O.torch_log(sd)
        ws = _lib.Workspace()
        with route("filter"):
            assert _lib.filter_dim(n, dim) == 64
            k = _lib.debug_plan(len(mu), n, dim)["ef_coeff"]
            assert k >= K_128_PRODUCTS
            with filter_launches() as ran:
                idx, zhat = _lib.gq_argmax(torch.from_numpy(mu).to(DEV), torch.from_numpy(sd).to(DEV), cbd, beta,
                                           logsd=torch.from_numpy(lsd).to(DEV), ws=ws)
            assert ran["n"] >= 1
            w = records_within_bound(ws, len(mu), n, dim, A, B, rs, pad(cb, 0.0), beta, "gq", k)
        ref, _ = O.argmax_rows(mu, sd, cb, beta, logstd=lsd)
        got = idx.cpu().numpy()
        print(f"dim {dim} -> {dp} max|cb| {scale} beta {beta} k {k}: {name:70s} records within {w:.3f} of the charged bound")
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
        assert np.array_equal(zhat.cpu().numpy(), cb[got])
        assert w <= 1.0, (name, w)


def _trained_z(shape_mu, g, channel_dim):
    return torch.cat([0.9 * torch.randn(shape_mu, generator=g), -1.5 + 0.3 * torch.randn(shape_mu, generator=g)], channel_dim)


@pytest.mark.parametrize("fmt", ["bchw", "blc"])
def test_gq1_module_eval_forward(fmt):
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    q = GaussianQuantRegularizer(fmt, 4096, group=64).eval().to(DEV)
    g = torch.Generator().manual_seed(3)
    z = (_trained_z((2, 64, 4, 4), g, 1) if fmt == "bchw" else _trained_z((2, 16, 64), g, 2)).to(DEV)
    assert z.shape == ((2, 128, 4, 4) if fmt == "bchw" else (2, 16, 128))

    def fwd():
        torch.manual_seed(11)
        with torch.no_grad():
            zhat, info = q(z)
        return zhat, info["indices"], info["zhat_noquant"]

    e, p = _both_routes(fwd, 4096, 64)
    for a, b in zip(e, p):
        assert _same(a, b)
    assert torch.equal(q.dequant(p[1]), p[0])


def test_gq2_module_three_eval_forwards():
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer2

    g = torch.Generator().manual_seed(4)
    zs = [_trained_z((2, 48, 8, 8), g, 1).to(DEV) for _ in range(3)]
    keys = ("indices", "zhat_noquant", "zhat_quant", "std", "kl_loss", "bits-mean", "bits-min", "bits-max", "lam", "lam-min", "lam-max")

    def three():
        torch.manual_seed(40)
        q = GaussianQuantRegularizer2(dim=48, codebook_size=512, dim_idx=1).eval().to(DEV)
        out = []
        for i, z in enumerate(zs):
            torch.manual_seed(20 + i)
            with torch.no_grad():
                zhat, info = q(z)
            out.append([zhat.clone()] + [info[k].clone() for k in keys])
            assert torch.equal(q.dequant(info["indices"]), info["zhat_quant"])
        return out, (q.lam, q.lam_min, q.lam_max)

    (e, lam_e), (p, lam_p) = _both_routes(three, 512, 48)
    for i, (a, b) in enumerate(zip(e, p)):
        for name, x, y in zip(("zhat",) + keys, a, b):
            assert _same(x, y), (i, name)
    assert lam_e == lam_p and lam_p[0] != 1.0


@pytest.mark.parametrize("channels_last", [False, True])
def test_vq_module_two_codebooks(channels_last):
    from pit_hip.quantization.vq import VQQuantizer

    torch.manual_seed(5)
    q = VQQuantizer("bchw", 1024, 40, codebook_num=2)
    q.embedding.weight.data.normal_()
    q = q.eval().to(DEV)
    z = torch.randn(2, 80, 8, 8, generator=torch.Generator().manual_seed(6)).to(DEV)
    if channels_last:
        z = z.contiguous(memory_format=torch.channels_last)

    def fwd():
        with torch.no_grad():
            zq, info = q(z)
        return zq, info["indices"], info["codebook_loss"]

    e, p = _both_routes(fwd, 1024, 40)
    for a, b in zip(e, p):
        assert _same(a, b)
    # the forward stores z + (e - z): two fp32 roundings, each below 2^-24 (2 |e| + |z|), around the codeword e that dequant returns
    big = max(float(z.abs().max()), float(q.embedding.weight.detach().abs().max()))
    assert float((q.dequant(p[1]).detach() - p[0]).abs().max()) <= 2.0 ** -22 * big
    want = O.vq_forward(z.cpu().numpy(), q.embedding.weight.detach().cpu().numpy(), 2, "bchw")
    assert np.array_equal(p[1].cpu().numpy(), want[1])


def test_one_train_forward_of_gq2_and_of_vq():
    """The train forwards reach the same arg-max (vq_quantize_z_f32 / the Gaussian train step's forward): same bits on either route,
    gradients included."""
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer2
    from pit_hip.quantization.vq import VQQuantizer

    g = torch.Generator().manual_seed(14)
    z2 = _trained_z((2, 48, 8, 8), g, 1).to(DEV)
    w2 = torch.randn(2, 48, 8, 8, generator=g).to(DEV)
    zv = torch.randn(2, 80, 8, 8, generator=g).to(DEV)
    wv = torch.randn(2, 80, 8, 8, generator=g).to(DEV)

    def gq2_step():
        torch.manual_seed(41)
        q = GaussianQuantRegularizer2(dim=48, codebook_size=512, dim_idx=1).to(DEV).train()
        zi = z2.clone().requires_grad_(True)
        torch.manual_seed(42)
        zhat, info = q(zi)
        ((zhat * w2).sum() + 0.37 * info["kl_loss"]).backward()
        return zhat.detach(), info["indices"], info["kl_loss"].detach(), zi.grad

    def vq_step():
        torch.manual_seed(43)
        q = VQQuantizer("bchw", 1024, 40, codebook_num=2)
        q.embedding.weight.data.normal_()
        q = q.to(DEV).train()
        zi = zv.clone().requires_grad_(True)
        zq, info = q(zi)
        ((zq * wv).sum() + 0.5 * info["codebook_loss"]).backward()
        return zq.detach(), info["indices"], info["codebook_loss"].detach(), zi.grad, q.embedding.weight.grad

    for step, n, dim in ((gq2_step, 512, 48), (vq_step, 1024, 40)):
        e, p = _both_routes(step, n, dim)
        for i, (a, b) in enumerate(zip(e, p)):
            assert _same(a, b), (step.__name__, i)


def test_scratch_contract_at_dims_40_and_64():
    """The workspace may hold anything on entry: 0xFF bytes before the call, and a larger shape's leftovers before a smaller one."""
    from pit_hip import _lib

    n = 4096 + 33
    g = torch.Generator().manual_seed(8)
    with route("filter"):
        for dim in (40, 64):
            cb = torch.randn(n, dim, generator=g).to(DEV)
            ws = _lib.Workspace()
            for rows in (777, 100):                       # the larger first: its leftovers lie under and behind the smaller one's regions
                mu, sd = (t.to(DEV) for t in _gq_rows("trained", rows, dim, g))
                clean = _lib.gq_argmax(mu, sd, cb, 1.0, ws=_lib.Workspace())
                again = _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
                ws.buf.fill_(0xFF)
                dirty = _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
                vq_clean = _lib.vq_argmin(mu, cb, ws=_lib.Workspace())
                ws.buf.fill_(0xFF)
                vq_dirty = _lib.vq_argmin(mu, cb, ws=ws)
                for a, b in ((clean, again), (clean, dirty), (vq_clean, vq_dirty)):
                    assert torch.equal(a[0], b[0]) and _same(a[1], b[1]), (dim, rows)
            z = _trained_z((2, 2 * dim, 8, 8), g, 1).to(DEV)
            noise = torch.randn(2, 2 * dim, 8, 8, generator=g).to(DEV)
            run = lambda w: _lib.gq_quantize_z(z, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED, ws=w, noise=noise)
            clean = run(_lib.Workspace())
            run(ws)
            ws.buf.fill_(0xFF)
            for a, b in zip(clean, run(ws)):
                assert _same(a, b), dim


def test_workspace_regrows_after_the_selection_changes():
    """One Workspace across a change of the selection: it asks the library again and grows by itself."""
    from pit_hip import _lib

    g = torch.Generator().manual_seed(18)
    dim, n = 48, 4096
    cb = torch.randn(n, dim, generator=g).to(DEV)
    mu, sd = (t.to(DEV) for t in _gq_rows("trained", 300, dim, g))
    ws = _lib.Workspace()
    (ie, ze), (ip, zp) = _both_routes(lambda: _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws), n, dim)
    assert torch.equal(ie, ip) and _same(ze, zp)
    with route("filter"):
        assert ws.buf.numel() >= _lib.lib().gqhip_workspace_bytes(300, n, dim)


def test_graph_capture_of_the_module_call():
    from pit_hip import _lib

    dim, n = 48, 4096
    g = torch.Generator().manual_seed(9)
    cb = torch.randn(n, dim, generator=g).to(DEV)
    mk = lambda: _trained_z((2, 96, 16, 16), g, 1)
    z_static = mk().to(DEV)
    with route("filter"):
        assert _lib.filter_dim(n, dim) == 64
        ws = _lib.Workspace()
        run = lambda: _lib.gq_quantize_z(z_static, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED, ws=ws)
        run()                                          # warm-up: sizes the workspace outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                  # one stream, no side branches
            idx_g, zhat_g = run()
        z_new = mk().to(DEV)
        z_static.copy_(z_new)
        graph.replay()
        torch.cuda.synchronize()
    idx_e, zhat_e = _lib.gq_quantize_z(z_new, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED)     # the exhaustive route
    assert torch.equal(idx_g, idx_e) and torch.equal(zhat_g, zhat_e)


@pytest.mark.parametrize("rows,dim,n", [(1000, 16, 65536), (777, 32, 4096), (1000, 12, 65536), (1000, 4, 65536)])
def test_no_existing_route_moved(rows, dim, n):
    from pit_hip import _lib

    g = torch.Generator().manual_seed(31)
    mu = torch.randn(rows, dim, generator=g).to(DEV)
    sd = (torch.randn(rows, dim, generator=g).abs() + 1e-3).to(DEV)
    cb = torch.randn(n, dim, generator=g).to(DEV)

    def both():
        ws = _lib.Workspace()
        return (_lib.debug_plan(rows, n, dim), _lib.lib().gqhip_workspace_bytes(rows, n, dim), _lib.lib().gqhip_cb_cache_bytes(n, dim),
                _lib.filter_dim(n, dim), _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws))

    with route("exhaustive"):
        pe, we, ce, fe, (ie, ze) = both()
    with route("filter"):
        pp, wp, cp, fp, (ip, zp) = both()
    torch.cuda.synchronize()
    assert pe == pp and we == wp and ce == cp and fe == fp
    assert torch.equal(ie, ip) and _same(ze, zp)
