"""The route selection of the codebook dims 1-3 (gqhip.h: gqhip_set_low_dims) as the host dispatch sees it: where a codebook cache is
asked for, where the search applies -- and that with the selection back at EXHAUSTIVE every word is the recorded one
(tests/golden/plan_table.json).  Host-only: no GPU.  Every test that flips the selection restores it."""
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

EXHAUSTIVE, SEARCH = 0, 1
INVALID_ARG = 1
NS = (1, 96, 4095, 4096, 4096 + 33, 16384, 65536, 65536 + 40, 1 << 20, (1 << 20) + 1, 1 << 23)


@pytest.fixture(scope="module")
def L():
    from pit_hip import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = P.load(_lib.LIB_PATH)
    i64 = ctypes.c_int64
    lib.gqhip_filter_dim.restype = i64
    lib.gqhip_filter_dim.argtypes = [i64, i64]
    lib.gqhip_set_low_dims.argtypes = [ctypes.c_int]
    lib.gqhip_low_dim_search_applies.argtypes = [i64, i64]
    assert not os.environ.get("GQHIP_LOW_DIMS"), "this test pins the default environment; unset GQHIP_LOW_DIMS"
    return lib


@contextlib.contextmanager
def selection(L, kind):
    before = L.gqhip_get_low_dims()
    try:
        assert L.gqhip_set_low_dims(kind) == 0
        yield
    finally:
        L.gqhip_set_low_dims(before)


def _in_range(n, d):
    return d in (1, 2, 3) and 4096 <= n <= (1 << 20)


def test_the_binding_reads_the_new_prototypes_from_the_header():
    from pit_hip import _lib

    i64 = ctypes.c_int64
    assert _lib._SIGNATURES["gqhip_set_low_dims"] == (ctypes.c_int, [ctypes.c_int])
    assert _lib._SIGNATURES["gqhip_get_low_dims"] == (ctypes.c_int, [])
    assert _lib._SIGNATURES["gqhip_low_dim_search_applies"] == (ctypes.c_int, [i64, i64])
    for name in ("gqhip_set_low_dims", "gqhip_get_low_dims", "gqhip_low_dim_search_applies"):
        assert name in _lib.EXPORTED_SYMBOLS


def test_default_is_exhaustive_and_the_recorded_table_survives_a_round_trip(L):
    assert L.gqhip_get_low_dims() == EXHAUSTIVE
    with selection(L, SEARCH):
        assert L.gqhip_get_low_dims() == SEARCH
        moved = L.gqhip_cb_cache_bytes(65536, 1)
    assert L.gqhip_get_low_dims() == EXHAUSTIVE
    assert moved > 0 and L.gqhip_cb_cache_bytes(65536, 1) == 0
    assert P.table(L, P.default_shapes()) == GOLDEN["default"]


def test_cache_bytes_and_applies_under_search(L):
    grid = [(n, d) for n in NS for d in range(1, 65)]
    today = {k: L.gqhip_cb_cache_bytes(*k) for k in grid}
    assert all(L.gqhip_low_dim_search_applies(*k) == 0 for k in grid)
    assert all(today[(n, d)] == 0 for n, d in grid if d < 4)
    with selection(L, SEARCH):
        for n, d in grid:
            got = L.gqhip_cb_cache_bytes(n, d)
            if _in_range(n, d):
                # the sorted codes and their indices at least
                assert got >= 4096 + 4 * n * (d + 1), (n, d, got)
                assert L.gqhip_low_dim_search_applies(n, d) == 1, (n, d)
            else:
                assert got == today[(n, d)], (n, d)
                assert L.gqhip_low_dim_search_applies(n, d) == 0, (n, d)
        assert L.gqhip_cb_cache_bytes(0, 1) == -1 and L.gqhip_cb_cache_bytes(65536, 65) == -1
    assert {k: L.gqhip_cb_cache_bytes(*k) for k in grid} == today


def test_filter_dim_grid_search_plan_and_workspace_are_unchanged(L):
    grid = [(n, d) for n in NS for d in range(1, 65)]

    def words():
        return ({k: (L.gqhip_filter_dim(*k), L.gqhip_grid_search_applies(*k)) for k in grid},
                [P.entry(L, rows, n, d)[:9] for rows in (100, 16384) for n in (4096 + 33, 65536) for d in (1, 2, 3, 4, 5)])

    today = words()
    with selection(L, SEARCH):
        assert words() == today
        assert all(L.gqhip_filter_dim(65536, d) == 0 for d in (1, 2, 3))
    assert words() == today


def test_the_search_does_not_depend_on_the_filter_or_the_odd_dims_selection(L):
    with selection(L, SEARCH):
        want = {(n, d): L.gqhip_cb_cache_bytes(n, d) for n in (4096, 65536) for d in (1, 2, 3)}
        before = L.gqhip_get_filter(), L.gqhip_get_odd_dims()
        try:
            for k in P.KINDS:
                for odd in (0, 1):
                    assert L.gqhip_set_filter(k) == 0 and L.gqhip_set_odd_dims(odd) == 0
                    assert {key: L.gqhip_cb_cache_bytes(*key) for key in want} == want
                    assert all(L.gqhip_low_dim_search_applies(*key) == 1 for key in want)
        finally:
            L.gqhip_set_filter(before[0])
            L.gqhip_set_odd_dims(before[1])


def test_invalid_kind_is_refused_and_changes_nothing(L):
    for start in (EXHAUSTIVE, SEARCH):
        with selection(L, start):
            for bad in (-1, 2, 7):
                assert L.gqhip_set_low_dims(bad) == INVALID_ARG
                assert L.gqhip_get_low_dims() == start
    assert L.gqhip_set_odd_dims(2) == INVALID_ARG               # (the odd-dims switch keeps refusing this kind)
    assert L.gqhip_get_low_dims() == EXHAUSTIVE


def test_degenerate_query_without_a_cache(L):
    L.gqhip_cb_cache_degenerate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    with selection(L, SEARCH):
        assert L.gqhip_cb_cache_degenerate(None, 65536, 1) == -1


def test_python_binding_round_trip():
    from pit_hip import _lib

    assert _lib.get_low_dims() == "exhaustive" and not _lib.low_dim_search_applies(65536, 1)
    try:
        _lib.set_low_dims("search")
        assert _lib.get_low_dims() == "search"
        assert _lib.low_dim_search_applies(65536, 1) and _lib.low_dim_search_applies(4096, 3)
        assert not _lib.low_dim_search_applies(65536, 4) and not _lib.low_dim_search_applies(96, 2)
        with pytest.raises(_lib.GqHipError):
            _lib.set_low_dims("search-ish")
        assert _lib.get_low_dims() == "search"
    finally:
        _lib.set_low_dims("exhaustive")
    assert not _lib.low_dim_search_applies(65536, 1)
