"""The route selection of the codebook dims 33-64 (gqhip.h: gqhip_set_wide_dims) as the host dispatch sees it: which dim the filter
runs at, the plan, the bound coefficient, the workspace and cache sizes -- and that with the selection back at EXHAUSTIVE every word
is the recorded one (tests/golden/plan_table.json).  Host-only: no GPU.  Every test that flips a selection restores it."""
import contextlib
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_plan", os.path.join(ROOT, "tests", "golden", "make_golden_plan.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)
GOLDEN = json.load(open(P.FIXTURE))

EXHAUSTIVE, FILTER = 0, 1
INVALID_ARG = 1
WIDE = tuple(range(33, 65))
N = 65536
# 128 products per filter value: two fp16 roundings (16384 + 4), the fp32 roundings of the operands (3), 4 u per accumulation step
K_128_PRODUCTS = 16384 + 4 + 3 + 4 * 128


@pytest.fixture(scope="module")
def L():
    from pit_hip import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = P.load(_lib.LIB_PATH)
    lib.gqhip_filter_dim.restype = ctypes.c_int64
    lib.gqhip_filter_dim.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.gqhip_set_wide_dims.argtypes = [ctypes.c_int]
    lib.gqhip_set_odd_dims.argtypes = [ctypes.c_int]
    for name in ("GQHIP_WIDE_DIMS", "GQHIP_ODD_DIMS", "GQHIP_FILTER"):
        assert not os.environ.get(name), f"this test pins the default environment; unset {name}"
    return lib


@contextlib.contextmanager
def selection(L, kind):
    before = L.gqhip_get_wide_dims()
    try:
        assert L.gqhip_set_wide_dims(kind) == 0
        yield
    finally:
        L.gqhip_set_wide_dims(before)


@contextlib.contextmanager
def filter_kind(L, kind):
    before = L.gqhip_get_filter()
    try:
        assert L.gqhip_set_filter(kind) == 0
        yield
    finally:
        L.gqhip_set_filter(before)


def test_the_binding_reads_the_new_prototypes_from_the_header():
    from pit_hip import _lib

    header = open(os.path.join(ROOT, "include", "gqhip.h")).read()
    assert "#define GQHIP_WIDE_DIMS_EXHAUSTIVE 0" in header and "#define GQHIP_WIDE_DIMS_FILTER 1" in header
    assert "#define GQHIP_ABI_VERSION 8 " in header                    # additive: the version stays
    assert _lib._SIGNATURES["gqhip_set_wide_dims"] == (ctypes.c_int, [ctypes.c_int])
    assert _lib._SIGNATURES["gqhip_get_wide_dims"] == (ctypes.c_int, [])


def test_default_selection_is_exhaustive(L):
    assert L.gqhip_get_wide_dims() == EXHAUSTIVE
    assert L.gqhip_abi_version() == 8
    for d in WIDE:
        assert L.gqhip_filter_dim(N, d) == 0, d
    assert L.gqhip_filter_dim(N, 65) == -1


def test_filter_dim_under_filter(L):
    narrow = {d: L.gqhip_filter_dim(N, d) for d in range(1, 33)}
    with selection(L, FILTER):
        assert L.gqhip_get_wide_dims() == FILTER
        for d in WIDE:
            assert L.gqhip_filter_dim(N, d) == 64, d
        assert {d: L.gqhip_filter_dim(N, d) for d in narrow} == narrow
        assert L.gqhip_filter_dim(N, 65) == -1 and L.gqhip_filter_dim(0, 40) == -1
        for kind in (1, 2, 3):                                   # fp32, bf16, mixed: no dim-64 kernel of theirs
            with filter_kind(L, kind):
                for d in WIDE:
                    assert L.gqhip_filter_dim(N, d) == 0, (kind, d)
    assert narrow == {d: (d if d in (4, 8, 16, 32) else 0) for d in narrow}
    assert L.gqhip_get_wide_dims() == EXHAUSTIVE


def test_odd_dims_selection_does_not_reach_the_wide_dims(L):
    before = L.gqhip_get_odd_dims()
    try:
        assert L.gqhip_set_odd_dims(1) == 0
        for d in WIDE:
            assert L.gqhip_filter_dim(N, d) == 0, d
        with selection(L, FILTER):
            assert L.gqhip_filter_dim(N, 12) == 16 and L.gqhip_filter_dim(N, 40) == 64
    finally:
        L.gqhip_set_odd_dims(before)


@pytest.mark.parametrize("rows", [100, 4096, 16384])
def test_plan_coefficient_and_workspace_under_filter(L, rows):
    today40, today64, today32 = P.entry(L, rows, N, 40), P.entry(L, rows, N, 64), P.entry(L, rows, N, 32)
    with selection(L, FILTER):
        got40, got64, got32 = P.entry(L, rows, N, 40), P.entry(L, rows, N, 64), P.entry(L, rows, N, 32)
    assert today40[1] == 0 and today40[4] == 0 and today64[1] == 0        # no record sets, no filter on the exhaustive kernel
    assert got40[:8] == got64[:8]                                         # word for word the plan of dim 64
    assert got64[1] > 0 and got64[4] == 3                                 # record sets; the fp16 main product
    assert got64[5] >= K_128_PRODUCTS                                     # the bound coefficient at 128 products
    assert got32 == today32 and got32[5] == 16700                         # dim 32: unchanged, 64 products
    assert got40[8] > today40[8] and got64[8] > today64[8]                # the operand images, records (and padded copies) need room
    # the padded copies of rows and codebook, n x 64 x 4 bytes among them, are dim 40's alone
    assert got40[8] - got64[8] >= N * 64 * 4 - 3 * 4 * rows * (64 - 40) - 4096
    # the fp16 image: n x 128 slots x 2 bytes
    assert got64[8] - today64[8] >= N * 128 * 2


def test_no_cache_and_no_grid_search_at_wide_dims(L):
    for kind in (EXHAUSTIVE, FILTER):
        with selection(L, kind):
            for d in WIDE:
                for n in (1000, 16384, N, 1 << 20):
                    assert L.gqhip_cb_cache_bytes(n, d) == 0, (kind, n, d)
                    assert L.gqhip_grid_search_applies(n, d) == 0, (kind, n, d)


def test_invalid_kind_is_refused_and_changes_nothing(L):
    for start in (EXHAUSTIVE, FILTER):
        with selection(L, start):
            for bad in (-1, 2, 7):
                assert L.gqhip_set_wide_dims(bad) == INVALID_ARG
                assert L.gqhip_get_wide_dims() == start


def test_a_codebook_beyond_the_split_cap_stays_exhaustive(L):
    with selection(L, FILTER):
        big = 0x3fffffff
        assert L.gqhip_filter_dim(big, 64) == L.gqhip_filter_dim(big, 40) == 0
        assert P.entry(L, 100, big, 40)[1] == 0


def test_recorded_words_under_filter_at_narrow_dims_and_after_restoring(L):
    """Dims 1..32 of the recorded sweep keep their words under FILTER; dim 64 moves and comes back."""
    shapes = P.default_shapes()
    pick = [i for i, (r, n, d) in enumerate(shapes) if r in (100, 16384) and n in (1000, N, 1 << 20)]
    with selection(L, FILTER):
        got = P.table(L, [shapes[i] for i in pick])
        moved = P.entry(L, 16384, N, 64)
    for k in GOLDEN["default"]:
        for j, i in enumerate(pick):
            if shapes[i][2] != 64 or k != "0":                  # under the other filter selections dim 64 stays unrouted too
                assert got[k][j] == GOLDEN["default"][k][i], (k, shapes[i])
    at = shapes.index((16384, N, 64))
    want = {k: GOLDEN["default"][k][at] for k in GOLDEN["default"]}
    back = P.table(L, [(16384, N, 64)])
    assert {k: v[0] for k, v in back.items()} == want
    assert moved[:9] != want["0"][:9]


def test_python_binding_round_trip():
    from pit_hip import _lib

    assert _lib.get_wide_dims() == "exhaustive"
    before = _lib.lib().gqhip_workspace_bytes(1000, N, 48)
    try:
        _lib.set_wide_dims("filter")
        assert _lib.get_wide_dims() == "filter" and _lib.filter_dim(N, 48) == 64
        assert _lib.lib().gqhip_workspace_bytes(1000, N, 48) > before
        with pytest.raises(_lib.GqHipError):
            _lib.set_wide_dims("filter-ish")
        assert _lib.get_wide_dims() == "filter"
    finally:
        _lib.set_wide_dims("exhaustive")
    assert _lib.filter_dim(N, 48) == 0 and _lib.lib().gqhip_workspace_bytes(1000, N, 48) == before
