"""-m gpu: the pruned exact search of the codebook dims 1-3 (gqhip.h: gqhip_set_low_dims; csrc/gq_lowdim.h).  Three parties: the C
oracle (oracle/gq_oracle.py: the reference's arg-max, pit/quantization/gaussian.py:142-150), the exhaustive route of the same build,
and the search; every comparison is bit for bit, NaN-proof by words.  Every test that flips the selection restores it.

A fresh ``Workspace`` per compared call unless a test is about the cache: the search then always starts from an index it has to
build, and the one look a Workspace takes at a degenerate index (which sends the codebook back to the exhaustive route) never
replaces the path under test."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import gq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (1, 2, 3)
N_FULL = 65536


@contextlib.contextmanager
def route(kind):
    from pit_hip import _lib

    prev = _lib.get_low_dims()
    _lib.set_low_dims(kind)
    try:
        yield
    finally:
        _lib.set_low_dims(prev)


def _bits(t):
    """NaN-proof equality: compare the words"""
    return t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _both_routes(fn):
    """fn() under EXHAUSTIVE and under SEARCH: (exhaustive outputs, search outputs)"""
    with route("exhaustive"):
        e = fn()
    with route("search"):
        s = fn()
    torch.cuda.synchronize()
    return e, s


def _gq_rows(kind, rows, dim, g):
    mu = torch.randn(rows, dim, generator=g)
    if kind == "flat":                  # includes A >= 0 at beta = 1 (sd > 1)
        sd = torch.randn(rows, dim, generator=g).abs() + 0.5
    elif kind == "tiny-sd":
        sd = torch.randn(rows, dim, generator=g).abs() + 1e-3
    elif kind == "trained":
        sd = torch.rand(rows, dim, generator=g) * 0.25 + 0.05
    elif kind == "far":                 # mu far outside the codebook's range
        mu = torch.where(torch.rand(rows, dim, generator=g) < 0.5, -50.0, 50.0) + mu
        sd = torch.rand(rows, dim, generator=g) * 0.9 + 0.05
    else:                               # uniform
        sd = torch.rand(rows, dim, generator=g) * 0.9 + 0.05
    return mu, sd


def _lsd_variants(sd):
    """(logsd handed to the library, logsd the oracle scores with): none given -> float(log(double(sd))) inside the kernels"""
    with np.errstate(all="ignore"):
        plain = np.log(sd.numpy().astype(np.float64)).astype(np.float32)
    return [(None, plain), (torch.from_numpy(O.torch_log(sd.numpy())), O.torch_log(sd.numpy()))]


def _check_rows(mu, sd, cb, beta, tag, oracle=True, variants=(0, 1)):
    """oracle == exhaustive == search on these rows; returns (oracle or exhaustive indices, finish-launch rows of the search call)"""
    from pit_hip import _lib

    n, dim = cb.shape
    mud, sdd, cbd = mu.to(DEV), sd.to(DEV), cb.to(DEV)
    ref, fb = None, None
    for v in variants:
        given, lsd = _lsd_variants(sd)[v]
        ws = _lib.Workspace()
        lg = None if given is None else given.to(DEV)
        (ie, ze), (i_s, z_s) = _both_routes(lambda: _lib.gq_argmax(mud, sdd, cbd, beta, logsd=lg, ws=ws))
        what = (tag, "logsd given" if given is not None else "no logsd")
        if oracle:
            ref = O.argmax_rows(mu.numpy(), sd.numpy(), cb.numpy(), beta, logstd=lsd)[0]
            assert np.array_equal(ie.cpu().numpy(), ref), what + ("exhaustive vs oracle",)
        else:
            ref = ie.cpu().numpy()
        assert torch.equal(i_s, ie), what + (int((i_s != ie).sum()),)
        assert _same(z_s, ze), what
        assert (ws.cache_buf is not None) == (4096 <= n <= (1 << 20)), what      # a cache was taken exactly where the search applies
        fb = _lib.debug_counters(ws)[0]                 # (of the search call, the last one on ws)
    return ref, fb


@functools.lru_cache(maxsize=None)
def _book(kind, dim, n=N_FULL):
    from pit_hip.quantization.gaussian import prior_samples

    g = torch.Generator().manual_seed(77 * dim + len(kind))
    if kind == "module":
        return prior_samples(n, dim, 42).float()
    cb = torch.randn(n, dim, generator=g)
    if kind == "dup-after":             # 1000 codes copied to the END: the originals (lower indices) must win
        cb[n - 1000:] = cb[:1000]
    elif kind == "dup-before":          # 1000 codes copied to the FRONT: the copies (lower indices) must win
        cb[:1000] = cb[n - 1000:]
    elif kind == "collapsed":
        cb[:] = cb[0]
    elif kind == "nan":
        cb[1234, dim - 1] = float("nan")
    elif kind == "inf":
        cb[4321, 0] = float("inf")
    elif kind == "ball":                # 90 % of the codes in a ball of radius 1e-3: overfull cells
        k = int(0.9 * n)
        d = torch.randn(k, dim, generator=g)
        cb[:k] = 0.3 + 1e-3 * torch.rand(k, 1, generator=g) * d / d.norm(dim=1, keepdim=True)
    return cb


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("rows,n", [(37, 4096 + 33), (777, 16384), (257, N_FULL + 40)])
@pytest.mark.parametrize("dim", DIMS)
def test_rows_search_equals_exhaustive_equals_oracle(dim, rows, n, beta):
    g = torch.Generator().manual_seed(1000 * dim + rows + int(beta * 8))
    cb = torch.randn(n, dim, generator=g)
    for kind in ("uniform", "trained", "flat", "tiny-sd", "far"):
        mu, sd = _gq_rows(kind, rows if kind in ("uniform", "trained") else 64, dim, g)
        _check_rows(mu, sd, cb, beta, f"dim {dim} rows {mu.shape[0]} n {n} beta {beta} {kind}")


@pytest.mark.parametrize("dim", DIMS)
def test_a_shape_below_the_range_stays_exhaustive(dim):
    g = torch.Generator().manual_seed(dim)
    cb = torch.randn(96, dim, generator=g)
    mu, sd = _gq_rows("uniform", 37, dim, g)
    _check_rows(mu, sd, cb, 1.0, f"dim {dim} n 96")          # (asserts that no cache was taken)


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("dim", DIMS)
def test_special_rows_get_exhaustive_semantics(dim, beta):
    from pit_hip import _lib

    g = torch.Generator().manual_seed(50 + dim)
    n = 4096 + 33
    cb = torch.randn(n, dim, generator=g)
    mu, sd = torch.randn(71, dim, generator=g), torch.rand(71, dim, generator=g) * 0.6 + 0.2
    at = [3, 11, 19, 27, 35, 43]
    mu[at[0], 0] = float("nan")
    mu[at[1], dim - 1] = float("inf")
    sd[at[2], 0] = 0.0
    sd[at[3], dim - 1] = -0.5
    sd[at[4], 0] = float("inf")
    mu[at[5], 0] = float("-inf")
    for given in (None, torch.log(sd)):
        ws = _lib.Workspace()
        lg = None if given is None else given.to(DEV)
        (ie, ze), (i_s, z_s) = _both_routes(lambda: _lib.gq_argmax(mu.to(DEV), sd.to(DEV), cb.to(DEV), beta, logsd=lg, ws=ws))
        assert torch.equal(i_s, ie), (given is not None, i_s[at].tolist(), ie[at].tolist())
        assert _same(z_s, ze)
        fb = _lib.debug_counters(ws)[0]
        assert len(at) <= fb <= len(at) + 4, fb              # the special rows, and next to nothing else, went to the finish launch
    good = np.setdiff1d(np.arange(71), at)
    ref = O.argmax_rows(mu.numpy()[good], sd.numpy()[good], cb.numpy(), beta, logstd=O.torch_log(sd.numpy()[good]))[0]
    assert np.array_equal(i_s.cpu().numpy()[good], ref)


@pytest.mark.parametrize("kind", ["module", "randn", "dup-after", "dup-before", "collapsed", "nan", "inf", "ball"])
@pytest.mark.parametrize("dim", DIMS)
def test_codebooks(dim, kind):
    cb = _book(kind, dim)
    g = torch.Generator().manual_seed(9 * dim + len(kind))
    rows = 128
    mu, sd = _gq_rows("uniform", rows, dim, g)
    if kind.startswith("dup"):          # rows that sit on duplicated codes: an exact tie between the copy and the original
        src = cb[N_FULL - 1000:][:rows]
        mu, sd = src.clone(), torch.full((rows, dim), 0.05)
    if kind == "ball":
        # half of the rows well inside the ball (its 59 000 codes span ten cells of ~6000 at dim 1, one cell at dims 2 and 3: all
        # beyond the cap of 256), with sd 0.02 so that the score's vertex mu / (1 - beta sd^2) = 1.0004 mu lies inside it as well: their
        # winner is in an overfull cell
        mu[: rows // 2] = 0.3 + 5e-4 * (2.0 * torch.rand(rows // 2, dim, generator=g) - 1.0) / dim
        sd[: rows // 2] = 0.02
    ref, fb = _check_rows(mu, sd, cb, 1.0, f"dim {dim} {kind} book", variants=(1,))
    print(f"dim {dim} {kind}: {fb} of {rows} rows finished by the finish launch")
    if kind == "dup-after":
        assert (ref < N_FULL - 1000).all()
    if kind == "dup-before":
        assert (ref < 1000).any() and (ref < N_FULL - 1000).all()
    if kind in ("collapsed", "nan", "inf"):
        assert fb == rows, (kind, fb)       # an overfull cell / a non-finite book: every row through the finish launch
    if kind == "collapsed":
        assert (ref == 0).all()
    if kind == "ball":
        assert fb >= rows // 2, fb          # the rows that reach the ball's cells


def _trained_z(shape_mu, g, channel_dim):
    return torch.cat([0.9 * torch.randn(shape_mu, generator=g), -1.5 + 0.3 * torch.randn(shape_mu, generator=g)], channel_dim)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fmt", ["bchw", "blc"])
def test_gq1_module_eval_forward(fmt, group):
    from pit_hip import _lib
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    q = GaussianQuantRegularizer(fmt, N_FULL, group=group).eval().to(DEV)
    g = torch.Generator().manual_seed(3)
    z = (_trained_z((2, 8, 8, 8), g, 1) if fmt == "bchw" else _trained_z((2, 64, 8), g, 2)).to(DEV)

    def fwd():
        torch.manual_seed(11)
        with torch.no_grad():
            zhat, info = q(z)
        return zhat, info["indices"], info["zhat_noquant"]

    e, s = _both_routes(fwd)
    for a, b in zip(e, s):
        assert _same(a, b)
    assert torch.equal(q.dequant(s[1]), s[0])
    assert q._ws.cache_buf is not None and _lib.debug_counters(q._ws)[0] <= 1024 // group // 16


@pytest.mark.parametrize("dim,channels", [(1, 8), (2, 8), (3, 6)])
def test_gq2_module_three_eval_forwards(dim, channels):
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer2

    g = torch.Generator().manual_seed(4)
    zs = [_trained_z((2, channels, 8, 8), g, 1).to(DEV) for _ in range(3)]
    keys = ("indices", "zhat_noquant", "zhat_quant", "std", "kl_loss", "bits-mean", "bits-min", "bits-max", "lam", "lam-min", "lam-max")

    def three():
        q = GaussianQuantRegularizer2(dim=dim, codebook_size=N_FULL, dim_idx=1).eval().to(DEV)
        out = []
        for i, z in enumerate(zs):
            torch.manual_seed(20 + i)
            with torch.no_grad():
                zhat, info = q(z)
            out.append([zhat.clone()] + [info[k].clone() for k in keys])
            assert torch.equal(q.dequant(info["indices"]), info["zhat_quant"])
        return out, (q.lam, q.lam_min, q.lam_max), q._ws.cache_buf is not None

    (e, lam_e, cache_e), (s, lam_s, cache_s) = _both_routes(three)
    for i, (a, b) in enumerate(zip(e, s)):
        for name, x, y in zip(("zhat",) + keys, a, b):
            assert _same(x, y), (i, name)
    assert lam_e == lam_s
    assert cache_s and not cache_e


def test_vq_module_at_dim_2_takes_no_cache():
    from pit_hip.quantization.vq import VQQuantizer

    torch.manual_seed(5)
    q = VQQuantizer("bchw", N_FULL, 2)
    q.embedding.weight.data.normal_()
    q = q.eval().to(DEV)
    z = torch.randn(2, 2, 8, 8, generator=torch.Generator().manual_seed(6)).to(DEV)

    def fwd():
        with torch.no_grad():
            zq, info = q(z)
        return zq, info["indices"], info["codebook_loss"]

    e, s = _both_routes(fwd)
    for a, b in zip(e, s):
        assert _same(a, b)
    assert q._ws.buf is not None and q._ws.cache_buf is None


@pytest.mark.parametrize("dim", DIMS)
def test_cache_protocol(dim):
    """A 0xFF-filled workspace and cache cost one rebuild; a codebook edited in place is seen by the next call."""
    from pit_hip import _lib

    n = 16384
    g = torch.Generator().manual_seed(8 + dim)
    cb = torch.randn(n, dim, generator=g).to(DEV)
    mu, sd = (t.to(DEV) for t in _gq_rows("trained", 300, dim, g))
    with route("exhaustive"):
        want = _lib.gq_argmax(mu, sd, cb, 1.0)
    with route("search"):
        ws = _lib.Workspace()
        first = _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
        assert _lib.lib().gqhip_cb_cache_degenerate(ws.cache_buf.data_ptr(), n, dim) == 0
        ws.buf.fill_(0xFF)
        ws.cache_buf.fill_(0xFF)
        assert _lib.lib().gqhip_cb_cache_degenerate(ws.cache_buf.data_ptr(), n, dim) == -1
        dirty = _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
        assert _lib.lib().gqhip_cb_cache_degenerate(ws.cache_buf.data_ptr(), n, dim) == 0       # rebuilt
        for got in (first, dirty):
            assert torch.equal(got[0], want[0]) and _same(got[1], want[1])
        # move the winners of the first 50 rows far away, in place: the very next call must see it
        cb[want[0][:50]] += 100.0
        edited = _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
    with route("exhaustive"):
        want2 = _lib.gq_argmax(mu, sd, cb, 1.0)
    assert torch.equal(edited[0], want2[0]) and _same(edited[1], want2[1])
    assert not torch.equal(want2[0][:50], want[0][:50])


def test_graph_capture_of_the_search_module_call():
    from pit_hip import _lib

    dim, n = 1, N_FULL
    g = torch.Generator().manual_seed(9)
    cb = torch.randn(n, dim, generator=g).to(DEV)
    mk = lambda: _trained_z((2, 8, 16, 16), g, 1)
    z_static = mk().to(DEV)
    with route("search"):
        ws = _lib.Workspace()
        run = lambda: _lib.gq_quantize_z(z_static, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED, ws=ws)
        run()                                          # warm-up: sizes the workspace and the cache outside the capture
        run()                                          # (the call at which a Workspace looks at the index once)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                  # one stream, no side branches
            idx_g, zhat_g = run()
        for step in range(3):
            if step == 2:
                cb[idx_g.reshape(-1)[:100]] += 100.0   # an in-place codebook edit: the replay rebuilds the index in-stream
            z_new = mk().to(DEV)
            z_static.copy_(z_new)
            graph.replay()
            torch.cuda.synchronize()
            with route("exhaustive"):
                idx_e, zhat_e = _lib.gq_quantize_z(z_new, cb, dim, "bchw", _lib.GQHIP_GROUP_STRIDED)
            assert torch.equal(idx_g, idx_e) and torch.equal(zhat_g, zhat_e), step


@pytest.mark.parametrize("book", ["module", "randn"])
@pytest.mark.parametrize("kind", ["trained", "uniform", "flat"])
@pytest.mark.parametrize("dim", DIMS)
def test_the_search_ran_and_not_only_the_finish_launch(dim, kind, book):
    """At most rows / 16 rows may reach the finish launch: the arithmetic forces nothing more (<= 71 codes within the margin at dims 2
    and 3, one contiguous run at dim 1), and the cap keeps a route that hands everything to the exhaustive kernel from passing as equal."""
    rows = 1024
    g = torch.Generator().manual_seed(31 * dim + len(kind))
    mu, sd = _gq_rows(kind, rows, dim, g)
    for beta in (1.0, 0.25):
        _, fb = _check_rows(mu, sd, _book(book, dim), beta, f"dim {dim} {kind} {book} beta {beta}", oracle=False, variants=(1,))
        print(f"dim {dim} {kind} rows, {book} book, beta {beta}: {fb} of {rows} rows in the finish launch")
        assert fb <= rows // 16, fb


@pytest.mark.parametrize("dim", DIMS)
def test_null_cache_under_search_runs_the_exhaustive_route(dim):
    from pit_hip import _lib

    rows, n = 200, 16384
    g = torch.Generator().manual_seed(40 + dim)
    cb = torch.randn(n, dim, generator=g).to(DEV)
    mu, sd = (t.to(DEV) for t in _gq_rows("uniform", rows, dim, g))
    with route("exhaustive"):
        want = _lib.gq_argmax(mu, sd, cb, 1.0)
    with route("search"):
        assert _lib.lib().gqhip_cb_cache_bytes(n, dim) > 0
        ws = _lib.Workspace()
        wptr, wbytes = ws.get(rows, n, dim, mu.device)
        ws.buf.fill_(0xFF)
        for cache in ((None, 0), (torch.zeros(4096, dtype=torch.uint8, device=DEV), 4096)):     # NULL, and one that is too short
            idx = torch.empty(rows, dtype=torch.int64, device=DEV)
            zhat = torch.empty(rows, dim, dtype=torch.float32, device=DEV)
            _lib._call("gq_argmax_f32", mu.device, mu, sd, None, cb, idx, zhat, dim, rows, n, 1.0, wptr, wbytes, cache[0], cache[1])
            torch.cuda.synchronize()
            assert torch.equal(idx, want[0]) and _same(zhat, want[1])
            assert _lib.debug_counters(ws)[0] == 0        # (the exhaustive kernel over every row keeps no list)
