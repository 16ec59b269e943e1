"""-m gpu: the padded route of the codebook dims between the filter dims (gqhip.h: gqhip_set_odd_dims; dims 5-7, 9-15, 17-31 run the
filter at 8 / 16 / 32 on zero-padded operands, the re-rank scores with the true dim).  The references are the C oracle
(oracle/gq_oracle.py: the reference's arg-max, pit/quantization/gaussian.py:142-150; VQ: vq.py:58-73) and the exhaustive route of
the same build; every comparison is bit for bit.  Every test that flips the selection restores it."""
import contextlib

import numpy as np
import pytest
import torch

import f16_bound_model as M
from oracle import gq_oracle as O
from test_gpu_f16_bound import _records_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (5, 7, 9, 15, 17, 31, 6, 12, 24)


def _dp(d):
    return 8 if d < 8 else (16 if d < 16 else 32)


@contextlib.contextmanager
def route(kind):
    from pit_hip import _lib

    prev = _lib.get_odd_dims()
    _lib.set_odd_dims(kind)
    try:
        yield
    finally:
        _lib.set_odd_dims(prev)


def _bits(t):
    """NaN-proof equality: compare the words"""
    return t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _both_routes(fn):
    """fn() under EXHAUSTIVE and under PADDED: (exhaustive outputs, padded outputs)"""
    with route("exhaustive"):
        e = fn()
    with route("padded"):
        p = fn()
    torch.cuda.synchronize()
    return e, p


def _gq_rows(kind, rows, dim, g):
    if kind in ("flat", "tiny-sd"):
        rows = 64
    mu = torch.randn(rows, dim, generator=g)
    if kind == "flat":                  # (measured: no row of this kind is left undecided at these dims)
        sd = torch.randn(rows, dim, generator=g).abs() + 0.5
    elif kind == "tiny-sd":             # the conditioning of test_gpu_quantiser's undecided rows: the expansion cancels, the finish scan runs
        sd = torch.randn(rows, dim, generator=g).abs() + 1e-3
    elif kind == "trained":
        sd = torch.rand(rows, dim, generator=g) * 0.25 + 0.05
    else:
        sd = torch.rand(rows, dim, generator=g) * 0.9 + 0.05
    return mu, sd


def _lsd_variants(sd):
    """(logsd handed to the library, logsd the oracle scores with): none given -> float(log(double(sd))) inside the kernels"""
    plain = np.log(sd.numpy().astype(np.float64)).astype(np.float32)
    return [(None, plain), (torch.from_numpy(O.torch_log(sd.numpy())), O.torch_log(sd.numpy()))]


def _check_rows(mu, sd, cb, beta, tag, want_fb=False, need_fb=False):
    from pit_hip import _lib

    n, dim = cb.shape
    mud, sdd, cbd = mu.to(DEV), sd.to(DEV), cb.to(DEV)
    refs = {}
    for given, lsd in _lsd_variants(sd):
        key = lsd.tobytes()
        if key not in refs:
            refs[key] = O.argmax_rows(mu.numpy(), sd.numpy(), cb.numpy(), beta, logstd=lsd)[0]
        ws = _lib.Workspace()
        lg = None if given is None else given.to(DEV)
        (ie, ze), (ip, zp) = _both_routes(lambda: _lib.gq_argmax(mud, sdd, cbd, beta, logsd=lg, ws=ws))
        what = (tag, "logsd given" if given is not None else "no logsd")
        assert np.array_equal(ie.cpu().numpy(), refs[key]), what + ("exhaustive vs oracle",)
        assert torch.equal(ip, ie), what + (int((ip != ie).sum()),)
        assert _same(zp, ze) and torch.equal(zp, cbd[ip]), what
        if want_fb:
            fb = _lib.debug_counters(ws)[0]             # (of the padded call, the last one on ws)
            print(f"{tag}: {fb} of {mu.shape[0]} rows finished by the in-block scan")
            assert fb >= 1 or not need_fb, tag
    return next(iter(refs.values()))


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("rows,n", [(37, 96), (777, 4096 + 33)])
@pytest.mark.parametrize("dim", DIMS)
def test_rows_padded_equals_exhaustive_equals_oracle(dim, rows, n, beta):
    _row_kinds(dim, rows, n, beta)


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("dim", [6, 12, 31])
def test_rows_at_the_full_codebook_size(dim, beta):
    _row_kinds(dim, 257, 65536 + 40, beta)


def _row_kinds(dim, rows, n, beta):
    from pit_hip import _lib

    with route("padded"):
        assert _lib.filter_dim(n, dim) == _dp(dim) and _lib.debug_plan(rows, n, dim)["nsplit"] > 0
    g = torch.Generator().manual_seed(1000 * dim + rows + int(beta * 8))
    cb = torch.randn(n, dim, generator=g)
    first = None
    for kind in ("random", "trained", "flat", "tiny-sd"):
        mu, sd = _gq_rows(kind, rows, dim, g)
        ref = _check_rows(mu, sd, cb, beta, f"dim {dim} rows {mu.shape[0]} n {n} beta {beta} {kind}", want_fb=kind in ("flat", "tiny-sd"),
                          need_fb=kind == "tiny-sd" and n > 65536)
        if kind == "random":
            first = (mu, sd, ref)
    # rows whose winning code is duplicated later in the codebook: the first index must win
    mu, sd, ref = first
    cb2 = cb.clone()
    winners = np.unique(ref[ref < n // 2])[: max(1, n // 8)]
    cb2[n - len(winners):] = cb[torch.from_numpy(winners)]
    hit = np.isin(ref, winners)
    assert hit.any()
    ref2 = _check_rows(mu, sd, cb2, beta, f"dim {dim} rows {rows} n {n} beta {beta} duplicated winners")
    assert (ref2[hit] < n - len(winners)).all()


@pytest.mark.parametrize("dim", [6, 12])
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
            (ie, ze), (ip, zp) = _both_routes(lambda: _lib.gq_argmax(mu.to(DEV), sd.to(DEV), book.to(DEV), beta, logsd=lg, ws=ws))
            assert torch.equal(ip, ie), (tag, given is not None, ip[at].tolist(), ie[at].tolist())
            assert _same(zp, ze), tag
            fb = _lib.debug_counters(ws)[0]                     # (of the padded call, the last one on ws)
            assert fb >= (71 if tag in ("a NaN code", "a NaN beta") else 4), (tag, fb)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -8, 200.0])
@pytest.mark.parametrize("dim", [6, 12, 24])
def test_vq_padded_equals_exhaustive_equals_oracle(dim, scale):
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
    (ie, ze), (ip, zp) = _both_routes(lambda: _lib.vq_argmin(z.to(DEV), emb.to(DEV), ws=ws))
    ref = O.vq_argmin_rows(z.numpy(), emb.numpy())
    assert np.array_equal(ie.cpu().numpy(), ref)
    assert torch.equal(ip, ie) and _same(zp, ze)
    assert int(ip[5]) == 17 and int(ip[6]) == 100


def test_every_filter_selection_at_dim_12():
    from pit_hip import _lib

    rows, n, dim = 300, 8192, 12
    g = torch.Generator().manual_seed(12)
    cb = torch.randn(n, dim, generator=g)
    mu, sd = _gq_rows("trained", rows, dim, g)
    lsd = np.log(sd.numpy().astype(np.float64)).astype(np.float32)
    ref = O.argmax_rows(mu.numpy(), sd.numpy(), cb.numpy(), 1.0, logstd=lsd)[0]
    prev = _lib.get_filter()
    words = {}
    try:
        for kind in ("auto", "fp32", "bf16", "mixed"):
            _lib.set_filter(kind)
            with route("padded"):
                words[kind] = _lib.debug_plan(rows, n, dim)["bf16"]
                idx, zhat = _lib.gq_argmax(mu.to(DEV), sd.to(DEV), cb.to(DEV), 1.0)
                vi, _ = _lib.vq_argmin(mu.to(DEV), cb.to(DEV))
            assert np.array_equal(idx.cpu().numpy(), ref), kind
            assert torch.equal(zhat, cb.to(DEV)[idx])
            assert np.array_equal(vi.cpu().numpy(), O.vq_argmin_rows(mu.numpy(), cb.numpy())), kind
    finally:
        _lib.set_filter(prev)
    assert words == {"auto": 3, "fp32": 0, "bf16": 1, "mixed": 2}     # the four filters of dim 16 all ran


@pytest.mark.parametrize("scale,beta", [(2.0 ** -8, 1.0), (16.0, 0.25), (254.9, 1.0)])
@pytest.mark.parametrize("dim", [6, 12, 24])
def test_bound_attack_at_padded_dims(dim, scale, beta):
    """The constructed operand sets of tests/f16_bound_model.py at the TRUE dim (fp16 ties, the class boundary, A -> 0, slack -> 0,
    fp16-subnormal coefficients and code features, max|cb| at the subnormal and near-overflow scales): the indices equal the oracle's,
    and every record the filter left is within the bound the plan charges -- the model evaluates filter, sums and bound on the
    zero-padded operands the kernels saw (mu 0, sd 1, code 0 in the pad columns), at the padded dim."""
    from pit_hip import _lib

    rng = np.random.default_rng(41 * dim + int(scale * 3) + int(beta * 7))
    n, rows, dp = 2048, 256, _dp(dim)
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
        with route("padded"):
            pl = _lib.debug_plan(len(mu), n, dim)
            assert pl["bf16"] == 3 and pl["ef_coeff"] == int(M.K_F16), pl
            idx, zhat = _lib.gq_argmax(torch.from_numpy(mu).to(DEV), torch.from_numpy(sd).to(DEV), cbd, beta,
                                       logsd=torch.from_numpy(lsd).to(DEV), ws=ws)
            torch.cuda.synchronize()
            w = _records_within_bound(ws, len(mu), n, dim, A, B, rs, pad(cb, 0.0), beta, "gq")
        ref, _ = O.argmax_rows(mu, sd, cb, beta, logstd=lsd)
        got = idx.cpu().numpy()
        print(f"dim {dim} -> {dp} max|cb| {scale} beta {beta}: {name:70s} records within {w:.3f} of the charged bound")
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
        assert np.array_equal(zhat.cpu().numpy(), cb[got])
        assert w <= 1.0, (name, w)


def _trained_z(shape_mu, g, channel_dim):
    return torch.cat([0.9 * torch.randn(shape_mu, generator=g), -1.5 + 0.3 * torch.randn(shape_mu, generator=g)], channel_dim)


@pytest.mark.parametrize("fmt", ["bchw", "blc"])
def test_gq1_module_eval_forward(fmt):
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    q = GaussianQuantRegularizer(fmt, 4096, group=12).eval().to(DEV)
    g = torch.Generator().manual_seed(3)
    z = (_trained_z((2, 24, 8, 8), g, 1) if fmt == "bchw" else _trained_z((2, 64, 24), g, 2)).to(DEV)

    def fwd():
        torch.manual_seed(11)
        with torch.no_grad():
            zhat, info = q(z)
        return zhat, info["indices"], info["zhat_noquant"]

    e, p = _both_routes(fwd)
    for a, b in zip(e, p):
        assert _same(a, b)
    assert torch.equal(q.dequant(p[1]), p[0])


def test_gq2_module_three_eval_forwards():
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer2

    g = torch.Generator().manual_seed(4)
    zs = [_trained_z((2, 12, 8, 8), g, 1).to(DEV) for _ in range(3)]
    keys = ("indices", "zhat_noquant", "zhat_quant", "std", "kl_loss", "bits-mean", "bits-min", "bits-max", "lam", "lam-min", "lam-max")

    def three():
        q = GaussianQuantRegularizer2(dim=6, codebook_size=512, dim_idx=1).eval().to(DEV)
        out = []
        for i, z in enumerate(zs):
            torch.manual_seed(20 + i)
            with torch.no_grad():
                zhat, info = q(z)
            out.append([zhat.clone()] + [info[k].clone() for k in keys])
            assert torch.equal(q.dequant(info["indices"]), info["zhat_quant"])
        return out, (q.lam, q.lam_min, q.lam_max)

    (e, lam_e), (p, lam_p) = _both_routes(three)
    for i, (a, b) in enumerate(zip(e, p)):
        for name, x, y in zip(("zhat",) + keys, a, b):
            assert _same(x, y), (i, name)
    assert lam_e == lam_p and lam_p[0] != 1.0


@pytest.mark.parametrize("channels_last", [False, True])
def test_vq_module_two_codebooks(channels_last):
    from pit_hip.quantization.vq import VQQuantizer

    torch.manual_seed(5)
    q = VQQuantizer("bchw", 1024, 12, codebook_num=2)
    q.embedding.weight.data.normal_()
    q = q.eval().to(DEV)
    z = torch.randn(2, 24, 8, 8, generator=torch.Generator().manual_seed(6)).to(DEV)
    if channels_last:
        z = z.contiguous(memory_format=torch.channels_last)

    def fwd():
        with torch.no_grad():
            zq, info = q(z)
        return zq, info["indices"], info["codebook_loss"]

    e, p = _both_routes(fwd)
    for a, b in zip(e, p):
        assert _same(a, b)
    # the forward stores z + (e - z): two fp32 roundings, each below 2^-24 (2 |e| + |z|), around the codeword e that dequant returns
    big = max(float(z.abs().max()), float(q.embedding.weight.detach().abs().max()))
    assert float((q.dequant(p[1]).detach() - p[0]).abs().max()) <= 2.0 ** -22 * big
    want = O.vq_forward(z.cpu().numpy(), q.embedding.weight.detach().cpu().numpy(), 2, "bchw")
    assert np.array_equal(p[1].cpu().numpy(), want[1])


def test_scratch_contract_at_dim_12():
    """The workspace may hold anything on entry: 0xFF bytes before the call, and a larger shape's leftovers before a smaller one."""
    from pit_hip import _lib

    dim, n = 12, 4096 + 33
    g = torch.Generator().manual_seed(8)
    cb = torch.randn(n, dim, generator=g).to(DEV)
    with route("padded"):
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
                assert torch.equal(a[0], b[0]) and _same(a[1], b[1]), rows
        z = _trained_z((2, 24, 8, 8), g, 1).to(DEV)
        noise = torch.randn(2, 24, 8, 8, generator=g).to(DEV)
        run = lambda w: _lib.gq_quantize_z(z, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED, ws=w, noise=noise)
        clean = run(_lib.Workspace())
        run(ws)
        ws.buf.fill_(0xFF)
        for a, b in zip(clean, run(ws)):
            assert _same(a, b)


def test_graph_capture_of_the_padded_module_call():
    from pit_hip import _lib

    dim, n = 12, 4096
    g = torch.Generator().manual_seed(9)
    cb = torch.randn(n, dim, generator=g).to(DEV)
    mk = lambda: _trained_z((2, 24, 16, 16), g, 1)
    z_static = mk().to(DEV)
    with route("padded"):
        ws = _lib.Workspace()
        run = lambda: _lib.gq_quantize_z(z_static, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED, ws=ws)
        run()                                          # warm-up: sizes the workspace outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                  # one stream, no side branches
            idx_g, zhat_g = run()
        for _ in range(2):
            z_new = mk().to(DEV)
            z_static.copy_(z_new)
            graph.replay()
            torch.cuda.synchronize()
            idx_e, zhat_e = _lib.gq_quantize_z(z_new, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED)
            assert torch.equal(idx_g, idx_e) and torch.equal(zhat_g, zhat_e)


@pytest.mark.parametrize("rows,dim,n", [(1000, 16, 65536), (96, 16, 65536), (1000, 8, 20000), (777, 32, 4096), (1000, 4, 65536)])
def test_no_existing_route_moved(rows, dim, n):
    from pit_hip import _lib

    g = torch.Generator().manual_seed(31)
    mu = torch.randn(rows, dim, generator=g).to(DEV)
    sd = (torch.randn(rows, dim, generator=g).abs() + 1e-3).to(DEV)
    cb = torch.randn(n, dim, generator=g).to(DEV)

    def both():
        ws = _lib.Workspace()
        return (_lib.debug_plan(rows, n, dim), _lib.lib().gqhip_workspace_bytes(rows, n, dim), _lib.lib().gqhip_cb_cache_bytes(n, dim),
                _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws))

    (pe, we, ce, (ie, ze)), (pp, wp, cp, (ip, zp)) = _both_routes(both)
    assert pe == pp and we == wp and ce == cp
    assert torch.equal(ie, ip) and _same(ze, zp)
