"""The fp64 moments kernel (csrc/gq_moments.h) and the Frechet statistics on the GPU: the state bit for bit against the CPU route
(a sequential fp64 loop) over tile tails, row chunks, strided and misaligned inputs; guard words around the state; moments() and
evaluate_sharded(fid_features=...) on the device.

Fixtures: tests/golden/g32_fid*.npz (tests/golden/make_golden_fid.py), read through tests/fid_ref.py."""
import pytest
import torch

import fid_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = (1, 3, 16, 63, 64, 65, 130)        # 63, 65, 130: tile tails (64 x 64 tiles); 130: three tiles per side, even D
ROWS = (1, 2, 15, 16, 17, 70)             # 70: more than one 16-row chunk, with a ragged last one
GUARD = 64
GUARD_BITS = 0x7FF8DEADBEEF0001           # a NaN with a payload: any write or any arithmetic on it shows


@pytest.fixture(scope="module")
def L():
    from pit_hip import _lib

    return _lib


def _features(rows, D, seed):
    """fp32 [rows, D]: relu'd Gaussians with a few exact zeros, negative zeros, a subnormal and large values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(rows, D, generator=g) + 0.3) * (1 + 9 * torch.rand(D, generator=g))
    x[0, 0] = -0.0
    x[-1, -1] = 3.0e4
    if D > 2:
        x[0, 1], x[-1, 2] = 1e-40, -7.25
    return x


def _cpu_state(blocks, D):
    from pit_hip.evaluations.fid.fid_score import FrechetStats

    st = FrechetStats(D, "cpu")
    for b in blocks:
        st.update(b.contiguous())
    return st.state


def _gpu_state(L, blocks, D, state=None):
    state = torch.zeros(D * D + D + 1, dtype=torch.float64, device=DEV) if state is None else state
    for b in blocks:
        L.moments_update(b, state)
    return state


@pytest.mark.parametrize("D", DIMS)
def test_state_bits_equal_the_cpu_route(L, D):
    """Every (D, rows) of the grid, each on a state that already holds three rows (the kernel adds to what it loads)."""
    for rows in ROWS:
        first, x = _features(3, D, 10 * D), _features(rows, D, 100 * D + rows)
        want = _cpu_state([first, x], D)
        got = _gpu_state(L, [first.to(DEV), x.to(DEV)], D)
        R.assert_state_bits(got, want, D, f"D={D} rows={rows}")


def test_state_bits_at_the_workload_shape(L):
    D, rows = 2048, 16
    blocks = [_features(rows, D, 7), _features(rows, D, 8)]
    want = _cpu_state(blocks, D)
    got = _gpu_state(L, [b.to(DEV) for b in blocks], D)
    R.assert_state_bits(got, want, D, "D=2048 rows=16, two calls")


@pytest.mark.parametrize("D,rows", [(65, 17), (130, 70), (64, 16)])
def test_strided_and_misaligned_inputs_give_the_same_bits(L, D, rows):
    x = _features(rows, D, 5 * D + rows)
    want = _gpu_state(L, [x.to(DEV)], D)
    R.assert_state_bits(want, _cpu_state([x], D), D, "aligned")
    W = (D + 12 + 3) // 4 * 4                                            # a multiple of 4: every row of the slice is 16-byte aligned
    wide = torch.full((rows, W), 1e30, device=DEV)                       # what lies beside the slice must not be read into the sums
    wide[:, 4:4 + D] = x.to(DEV)
    sliced = wide[:, 4:4 + D]                                            # row_stride > D; at D = 65 the last quad of a row straddles D
    assert sliced.stride(0) == W and sliced.data_ptr() % 16 == 0
    R.assert_state_bits(_gpu_state(L, [sliced], D), want, D, "row_stride > D")
    wide[:, 5:5 + D] = x.to(DEV)
    wide[:, 4] = 1e30
    off = wide[:, 5:5 + D]                                               # one float off: the 4-byte load route
    assert off.data_ptr() % 16 == 4
    R.assert_state_bits(_gpu_state(L, [off], D), want, D, "x offset by one float")
    buf = torch.zeros(D * D + D + 2, dtype=torch.float64, device=DEV)    # the state one double off 16-byte alignment: 8-byte accesses
    assert buf[1:].data_ptr() % 16 == 8
    R.assert_state_bits(_gpu_state(L, [x.to(DEV)], D, state=buf[1:]), want, D, "state offset by one double")


def test_two_launches_of_one_input_give_equal_bits(L):
    D, rows = 130, 70
    x = _features(rows, D, 3).to(DEV)
    a, b = _gpu_state(L, [x], D), _gpu_state(L, [x], D)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    halves = _gpu_state(L, [x[:33], x[33:]], D)                           # and a split over two calls changes no bit
    R.assert_state_bits(halves, a, D, "33 + 37")


@pytest.mark.parametrize("D", [1, 65, 130])
def test_guard_words_around_the_state_are_untouched(L, D):
    words = D * D + D + 1
    buf = torch.full((GUARD + words + GUARD,), GUARD_BITS, dtype=torch.int64, device=DEV)
    state = buf[GUARD:GUARD + words].view(torch.float64)
    state.zero_()
    blocks = [_features(r, D, 9 * D + r) for r in (17, 70, 1)]
    _gpu_state(L, [b.to(DEV) for b in blocks], D, state=state)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == GUARD_BITS).all()) and bool((host[-GUARD:] == GUARD_BITS).all())
    R.assert_state_bits(state, _cpu_state(blocks, D), D, f"D={D} inside guards")


def test_moments_on_the_device_equal_the_cpu_route_bit_for_bit():
    from pit_hip.evaluations.fid.fid_score import FrechetStats

    f = R.load_fixtures()[2]                                               # D = 64, n = 500
    x = torch.from_numpy(f["x"])
    cpu, gpu = FrechetStats(64, "cpu"), FrechetStats(64, DEV)
    for part in torch.split(x, 48):
        cpu.update(part)
        gpu.update(part.to(DEV))
    (n0, m0, c0), (n1, m1, c1) = cpu.moments(), gpu.moments()
    assert n0 == n1 == 500 and torch.equal(m0, m1) and torch.equal(c0, c1) and torch.equal(c1, c1.T)
    maps = x[:48, :, None, None].to(DEV) + torch.tensor([[-1.0, 1.0], [0.5, -0.5]], device=DEV)     # [B, D, h, w] is pooled first
    pooled = torch.nn.functional.adaptive_avg_pool2d(maps, (1, 1))[:, :, 0, 0]
    assert torch.equal(FrechetStats(64, DEV).update(maps).state, FrechetStats(64, DEV).update(pooled).state)
    with pytest.raises(ValueError):
        gpu.update(x[:4].to(DEV).double())


def test_evaluate_sharded_reports_fid_on_the_device():
    from pit_hip.eval_dist import evaluate_sharded

    ext = R.StubExtractor()
    out = evaluate_sharded(R.StubModel(), R.stub_images, 43, 4, 0, 1, torch.device(DEV), 4, fid_features=ext)
    x, y = ext.inputs(), ext.reconstructions()
    want, scale = R.numpy_fid(x, y)
    print(f"fid {out['fid']:.9f} numpy {want:.9f} scale {scale:.3f}")
    assert out["fid_count"] == x.shape[0] == 40
    assert isinstance(out["fid"], float) and want > 1e-4 and abs(out["fid"] - want) <= R.FID_RTOL * scale
