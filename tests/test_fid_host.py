"""Host-side tests of the Frechet statistics: the C ABI of the moments kernel before any launch, FrechetStats on its CPU route,
calculate_frechet_distance against the reference's values, and evaluate_sharded(fid_features=...) at world 1 (no GPU needed).

Fixtures: tests/golden/g32_fid*.npz (tests/golden/make_golden_fid.py), read through tests/fid_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gq_moments_state_bytes", "gq_moments_update_f32")


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


@pytest.fixture(scope="module")
def fixtures():
    return R.load_fixtures()


def _stats(x, chunks=None):
    from pit_hip.evaluations.fid.fid_score import FrechetStats

    st = FrechetStats(x.shape[1], "cpu")
    t = torch.from_numpy(np.ascontiguousarray(x))
    for part in (t,) if chunks is None else torch.split(t, chunks):
        st.update(part)
    return st


# ---- header and binding -----------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_declared():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "gqhip.h")).read()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and name in L._SIGNATURES and hasattr(dll, name) and hasattr(L.lib(), name)
        assert re.search(r"^(?:int|int64_t)\s+%s\s*\(" % name, header, flags=re.M), name
    assert L._PARAMS["gq_moments_update_f32"] == ("x", "rows", "D", "row_stride", "state", "stream")
    VP, I64 = ctypes.c_void_p, ctypes.c_int64
    assert L._SIGNATURES["gq_moments_update_f32"] == (ctypes.c_int, [VP, I64, I64, I64, VP, VP])
    assert L._SIGNATURES["gq_moments_state_bytes"] == (I64, [I64])
    assert L.lib().gqhip_abi_version() == L.ABI_VERSION == 8
    assert "#define GQHIP_ABI_VERSION 8" in header
    assert callable(L.moments_update) and callable(L.moments_state_words)


def test_state_size_function():
    L = _lib()
    lib = L.lib()
    for D, want in ((0, -1), (1, 24), (2048, (2048 * 2048 + 2048 + 1) * 8), (8192, (8192 * 8192 + 8192 + 1) * 8), (8193, -1)):
        assert lib.gq_moments_state_bytes(D) == want, D
    assert L.moments_state_words(2048) == 2048 * 2048 + 2048 + 1
    with pytest.raises(L.GqHipError):
        L.moments_state_words(8193)


def test_statuses_without_a_device():
    """Expected statuses, written here, for made-up pointers that are never dereferenced because nothing can launch without a device
    (then a call that gets past its checks returns 3).  SAFETY: never where a HIP device is present -- it skips there."""
    if torch.cuda.is_available():
        pytest.skip("passes made-up pointers: safe only where no kernel can launch")
    lib = _lib().lib()
    fake = 0x10000

    def call(x=fake, rows=16, D=64, row_stride=None, state=fake):
        return lib.gq_moments_update_f32(x, rows, D, D if row_stride is None else row_stride, state, None)

    assert call(x=None) == 1 and call(state=None) == 1
    assert call(D=0) == 1 and call(D=8193) == 1
    assert call(rows=-1) == 1
    assert call(D=64, row_stride=63) == 1
    assert call(rows=1 << 20, D=2048, row_stride=2048) == 1            # rows * row_stride = 2^31
    assert call(rows=3, row_stride=1 << 31) == 1 and call(rows=1 << 31, D=1, row_stride=1 << 40) == 1
    assert call(state=fake + 4) == 1                                    # 8-byte alignment of the state
    assert call(x=fake + 2) == 1                                        # 4-byte alignment of x
    assert call(rows=0) == 0                                            # nothing to do: no launch
    assert call(rows=0, x=None) == 1                                    # the order of the checks: arguments before "nothing to do"
    assert call() == 3                                                  # would launch
    assert call(x=fake + 4) == 3 and call(state=fake + 8) == 3          # narrower alignment only picks the narrower accesses
    assert call(D=1) == 3 and call(D=8192, rows=1) == 3 and call(D=65, row_stride=130) == 3
    assert call(rows=(1 << 20) - 1, D=2048, row_stride=2048) == 3       # the largest rows * row_stride below 2^31 at this stride


def test_wrapper_refuses_before_the_library():
    L = _lib()
    state = torch.zeros(4 * 4 + 4 + 1, dtype=torch.float64)
    x = torch.zeros(3, 4)
    for bad in (x.double(), x.half(), x[0], x[None], torch.zeros(4, 3).T):
        with pytest.raises(ValueError, match=r"\bx\b"):
            L.moments_update(bad, state)
    for bad in (state.float(), state[:-1], torch.zeros(2, 21, dtype=torch.float64)[:, ::2], torch.zeros(42, dtype=torch.float64)[::2]):
        with pytest.raises(ValueError, match="state"):
            L.moments_update(x, bad)
    with pytest.raises(L.GqHipError, match="HIP device"):               # right operands, no device: no CPU fallback in the binding
        L.moments_update(x, state)


# ---- FrechetStats on the CPU ----------------------------------------------------------------------------------------------------------
def test_state_is_bit_equal_to_an_independent_numpy_loop(fixtures):
    for k in (0, 1, 3):
        x = fixtures[k]["x"][:120]
        st = _stats(x)
        S, s, n = R.moments_loop(x)
        R.assert_state_bits(st.state, np.concatenate([S.reshape(-1), s, [n]]), x.shape[1], f"fixture {k}")
        assert float(st.count) == x.shape[0]


def test_integer_data_is_exact():
    rng = np.random.default_rng(5)
    scales = np.array([1, 1, 10, 10, 100, 100, 1000, 1000, 1, 1000, 3])
    xi = (rng.integers(-1000, 1001, size=(53, scales.size)) * scales // 1000).astype(np.int64)
    xi[0], xi[1] = 1000 * np.sign(scales), -1000
    x = xi.astype(np.float32)
    assert np.array_equal(x.astype(np.int64), xi) and np.abs(xi).max() == 1000
    S, s, n = R.split_state(_stats(x).state, scales.size)
    iu = np.triu_indices(scales.size)
    assert np.array_equal(S[iu], (xi.T @ xi)[iu].astype(np.float64)) and np.array_equal(s, xi.sum(0).astype(np.float64)) and n == 53


def test_split_invariance(fixtures):
    x = fixtures[1]["x"][:37]
    one, parts = _stats(x), _stats(x, chunks=16)          # 37 rows at once, against 16 + 16 + 5
    R.assert_state_bits(parts.state, one.state, x.shape[1], "16 + 16 + 5")
    assert float(parts.count) == 37


def test_update_takes_spatial_features_and_refuses_the_rest(fixtures):
    from pit_hip.evaluations.fid.fid_score import FrechetStats

    x = torch.from_numpy(fixtures[0]["x"][:10])
    maps = x[:, :, None, None] + torch.tensor([[-1.0, 1.0], [0.5, -0.5]])          # mean over (h, w) is x, up to fp32 rounding
    want = FrechetStats(8, "cpu").update(torch.nn.functional.adaptive_avg_pool2d(maps, (1, 1))[:, :, 0, 0])
    assert torch.equal(FrechetStats(8, "cpu").update(maps).state, want.state)
    assert torch.equal(FrechetStats(8, "cpu").update(x[:, :, None, None]).state, FrechetStats(8, "cpu").update(x).state)
    st = FrechetStats(8, "cpu")
    for bad in (x.double(), x[:, :7], x[0]):
        with pytest.raises(ValueError):
            st.update(bad)
    with pytest.raises(ValueError, match="at least 2"):
        st.update(x[:1]).moments()
    with pytest.raises(ValueError):
        FrechetStats(0, "cpu")


def test_merge_adds_in_the_order_given(fixtures):
    x = fixtures[0]["x"]
    a, b, c = _stats(x[:20]), _stats(x[20:45]), _stats(x[45:])
    merged = _stats(x[:0]).merge_([a.state, b.state, c.state])
    assert torch.equal(merged.state, (a.state + b.state) + c.state) and float(merged.count) == x.shape[0]
    n, mean, cov = merged.moments()
    assert n == x.shape[0] and np.allclose(cov.numpy(), fixtures[0]["cov_x"], rtol=0, atol=1e-12)


def test_cov_is_bit_symmetric(fixtures):
    for k in (0, 2):
        n, mean, cov = _stats(fixtures[k]["x"]).moments()
        assert cov.dtype == mean.dtype == torch.float64 and n == fixtures[k]["x"].shape[0]
        assert torch.equal(cov, cov.T)
        # ... and built from the upper triangle alone: what lies below the diagonal of `outer` does not matter
        st = _stats(fixtures[k]["x"])
        st.outer.add_(torch.tril(torch.full_like(st.outer, 1e6), -1))
        assert torch.equal(st.moments()[2], cov)


def _check_cov_bound(x, what):
    """cov of FrechetStats against an np.longdouble evaluation of the CENTRED covariance.  Bound per element, derived: sequential
    summation of n terms in fp64 is off by at most (n - 1) u sum|terms| (u = 2^-53) to first order, for outer and for both sums;
    s_i s_j / n and the subtraction and division add three more roundings: (n + 4) u (sum_r |x_ri x_rj| + |s_i| |s_j| / n) / (n - 1)."""
    n, D = x.shape
    xl = x.astype(np.longdouble)
    c = xl - xl.mean(0)
    want = (c.T @ c) / (n - 1)
    got = _stats(x).moments()[2].numpy()
    a = np.abs(xl)
    s = np.abs(xl.sum(0))
    bound = (n + 4) * 2.0 ** -53 * (a.T @ a + np.outer(s, s) / n) / (n - 1)
    err = np.abs(got.astype(np.longdouble) - want)
    rel = float((err / np.abs(want).max()).max())
    print(f"{what}: n={n} D={D} max err / bound {float((err / bound).max()):.3f}, max err / max|cov| {rel:.2e}")
    assert (err <= bound).all(), what
    return rel


def test_cov_accuracy_against_longdouble(fixtures):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than fp64 here: no arbiter")
    for k, f in enumerate(fixtures):
        _check_cov_bound(f["x"], f"fixture {k}")
    rng = np.random.default_rng(11)
    shifted = (100.0 + 0.01 * rng.standard_normal((500, 32))).astype(np.float32)       # mean / std = 10^4
    _check_cov_bound(shifted, "mean 100, std 0.01")      # the bound is in sum|terms|: it holds here too; the printed figure is DESIGN 3.4b's


# ---- calculate_frechet_distance ------------------------------------------------------------------------------------------------------
def test_frechet_distance_against_the_reference(fixtures):
    from pit_hip.evaluations.fid.fid_score import calculate_frechet_distance

    for k, f in enumerate(fixtures):
        got = calculate_frechet_distance(f["mu_y"], f["cov_y"], f["mu_x"], f["cov_x"])
        scale = R.fid_scale(f["mu_y"], f["cov_y"], f["mu_x"], f["cov_x"])
        print(f"fixture {k}: fid {got:.9f} reference {float(f['fid']):.9f} |delta| / scale {abs(got - float(f['fid'])) / scale:.2e}")
        assert isinstance(got, float) and abs(got - float(f["fid"])) <= R.FID_RTOL * scale, k
        as_torch = calculate_frechet_distance(*(torch.from_numpy(np.asarray(f[n])) for n in ("mu_y", "cov_y", "mu_x", "cov_x")), eps=0.0)
        assert as_torch == got


def test_frechet_distance_from_accumulated_statistics(fixtures):
    """The whole route -- FrechetStats then the distance -- against the reference's value; the reference's mean is np.mean of an
    fp32 block (an fp32 mean), so its means are replaced by fp64 ones in its own formula."""
    from pit_hip.evaluations.fid.fid_score import calculate_frechet_distance

    for k in (0, 1, 3):
        f = fixtures[k]
        _, mx, cx = _stats(f["x"]).moments()
        _, my, cy = _stats(f["y"]).moments()
        want, scale = R.numpy_fid(f["x"], f["y"])
        assert abs(calculate_frechet_distance(my, cy, mx, cx) - want) <= R.FID_RTOL * scale, k


def test_frechet_distance_is_finite_on_singular_covariances(fixtures):
    from pit_hip.evaluations.fid.fid_score import calculate_frechet_distance

    f = fixtures[1]
    _, mx, cx = _stats(f["x"][:10]).moments()              # n = 10 < D = 48
    _, my, cy = _stats(f["y"][:10]).moments()
    got = calculate_frechet_distance(my, cy, mx, cx)
    scale = R.fid_scale(my.numpy(), cy.numpy(), mx.numpy(), cx.numpy())
    assert np.isfinite(got) and got >= -1e-9 * scale
    f = fixtures[0]                                        # a set against itself, n > D
    assert abs(calculate_frechet_distance(f["mu_x"], f["cov_x"], f["mu_x"], f["cov_x"])) <= 2e-9 * float(np.trace(f["cov_x"]))


# ---- evaluate_sharded, world 1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [False, True])
def test_evaluate_sharded_reports_fid(spatial):
    from pit_hip.eval_dist import evaluate_sharded

    n_images, bs = 43, 4                                   # 10 steps of 4: three items never evaluated at world 1 (drop_last)
    ext = R.StubExtractor(spatial=spatial)
    out = evaluate_sharded(R.StubModel(), R.stub_images, n_images, bs, 0, 1, torch.device("cpu"), 4, fid_features=ext)
    x, y = ext.inputs(), ext.reconstructions()
    assert out["fid_count"] == x.shape[0] == y.shape[0] == 40 and len(ext.blocks) == 20
    want, scale = R.numpy_fid(x, y)
    print(f"fid {out['fid']:.9f} numpy {want:.9f} scale {scale:.3f}")
    assert isinstance(out["fid"], float) and want > 1e-4 and abs(out["fid"] - want) <= R.FID_RTOL * scale
    plain = evaluate_sharded(R.StubModel(), R.stub_images, n_images, bs, 0, 1, torch.device("cpu"), 4)
    assert set(plain) == set(out) - {"fid", "fid_count"} == {"indices", "psnr"}
    assert all(torch.equal(plain[k], out[k]) for k in plain)


def test_evaluate_sharded_without_steps():
    """Fewer images than one batch: None, as without fid_features, and the extractor is never called.  (At world 1 the sampler never
    wraps; that the wrapped items count is test_fid_dist_cpu.py's.)"""
    from pit_hip.eval_dist import evaluate_sharded

    ext = R.StubExtractor()
    assert evaluate_sharded(R.StubModel(), R.stub_images, 3, 4, 0, 1, torch.device("cpu"), 4, fid_features=ext) is None
    assert ext.blocks == []
