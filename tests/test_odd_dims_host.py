"""The route selection of the codebook dims between the filter dims (gqhip.h: gqhip_set_odd_dims) as the host dispatch sees it:
which dim the filter runs at, the plan, the workspace and cache sizes -- and that with the selection back at EXHAUSTIVE every word
is the recorded one (tests/golden/plan_table.json).  Host-only: no GPU.  Every test that flips the selection restores it."""
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

EXHAUSTIVE, PADDED = 0, 1
INVALID_ARG = 1
ROUTED = {d: 8 for d in range(5, 8)} | {d: 16 for d in range(9, 16)} | {d: 32 for d in range(17, 32)}
N = 65536


@pytest.fixture(scope="module")
def L():
    from pit_hip import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = P.load(_lib.LIB_PATH)
    lib.gqhip_filter_dim.restype = ctypes.c_int64
    lib.gqhip_filter_dim.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.gqhip_set_odd_dims.argtypes = [ctypes.c_int]
    assert not os.environ.get("GQHIP_ODD_DIMS"), "this test pins the default environment; unset GQHIP_ODD_DIMS"
    return lib


@contextlib.contextmanager
def selection(L, kind):
    before = L.gqhip_get_odd_dims()
    try:
        assert L.gqhip_set_odd_dims(kind) == 0
        yield
    finally:
        L.gqhip_set_odd_dims(before)


def test_the_binding_reads_the_new_prototypes_from_the_header():
    from pit_hip import _lib

    assert "GQHIP_ERR_INVALID_ARG = 1," in open(os.path.join(ROOT, "include", "gqhip.h")).read()
    assert _lib._SIGNATURES["gqhip_filter_dim"] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64])
    assert _lib._SIGNATURES["gqhip_set_odd_dims"] == (ctypes.c_int, [ctypes.c_int])
    assert _lib._SIGNATURES["gqhip_get_odd_dims"] == (ctypes.c_int, [])


def test_default_selection_is_exhaustive(L):
    assert L.gqhip_get_odd_dims() == EXHAUSTIVE
    for d in (4, 8, 16, 32):
        assert L.gqhip_filter_dim(N, d) == d
    for d in (1, 5, 12, 31, 64):
        assert L.gqhip_filter_dim(N, d) == 0
    assert L.gqhip_filter_dim(0, 8) == -1 and L.gqhip_filter_dim(N, 65) == -1 and L.gqhip_filter_dim(N, 0) == -1


def test_filter_dim_under_padded(L):
    unrouted = {d: L.gqhip_filter_dim(N, d) for d in range(1, 65) if d not in ROUTED}
    with selection(L, PADDED):
        assert L.gqhip_get_odd_dims() == PADDED
        for d, dp in ROUTED.items():
            assert L.gqhip_filter_dim(N, d) == dp, d
        assert {d: L.gqhip_filter_dim(N, d) for d in unrouted} == unrouted
    assert unrouted == {d: (d if d in (4, 8, 16, 32) else 0) for d in unrouted}
    assert L.gqhip_get_odd_dims() == EXHAUSTIVE


def test_plan_and_workspace_of_dim_12_under_padded(L):
    rows = 4096
    today = P.entry(L, rows, N, 12)
    with selection(L, PADDED):
        got, at16 = P.entry(L, rows, N, 12), P.entry(L, rows, N, 16)
    assert today[1] == 0 and today[4] == 0                     # no record sets, no filter on the exhaustive kernel
    assert got[1] > 0 and got[1] == at16[1]                    # record sets
    assert got[4] == at16[4] == 3                              # the filter word: that of dim 16 (the fp16 main product)
    assert got[:8] == at16[:8]                                 # ... and with it the whole plan, bound coefficient included
    assert at16[9] > 0                                         # dim 16 keeps its operand image in the cache; dim 12 rebuilds one per call
    assert got[8] >= at16[8] - at16[9]
    assert got[8] > today[8]


def test_no_cache_and_no_grid_search_at_routed_dims(L):
    for kind in (EXHAUSTIVE, PADDED):
        with selection(L, kind):
            for d in ROUTED:
                for n in (1000, 16384, N, 1 << 20):
                    assert L.gqhip_cb_cache_bytes(n, d) == 0, (kind, n, d)
                    assert L.gqhip_grid_search_applies(n, d) == 0, (kind, n, d)


def test_invalid_kind_is_refused_and_changes_nothing(L):
    for start in (EXHAUSTIVE, PADDED):
        with selection(L, start):
            for bad in (-1, 2, 7):
                assert L.gqhip_set_odd_dims(bad) == INVALID_ARG
                assert L.gqhip_get_odd_dims() == start


def test_a_codebook_beyond_the_split_cap_stays_exhaustive(L):
    with selection(L, PADDED):
        big = 0x3fffffff
        assert L.gqhip_filter_dim(big, 16) == L.gqhip_filter_dim(big, 12) == 0


def test_recorded_words_after_restoring_exhaustive(L):
    with selection(L, PADDED):
        moved = P.entry(L, 16384, N, 5)
    at = P.default_shapes().index((16384, N, 5))
    want = {k: GOLDEN["default"][k][at] for k in GOLDEN["default"]}
    got = P.table(L, [(16384, N, 5)])
    assert {k: v[0] for k, v in got.items()} == want
    assert moved[:9] != want["0"][:9]                          # (and under PADDED they were other words)


def test_python_binding_round_trip():
    from pit_hip import _lib

    assert _lib.get_odd_dims() == "exhaustive"
    try:
        _lib.set_odd_dims("padded")
        assert _lib.get_odd_dims() == "padded" and _lib.filter_dim(N, 12) == 16
        with pytest.raises(_lib.GqHipError):
            _lib.set_odd_dims("padded-ish")
        assert _lib.get_odd_dims() == "padded"
    finally:
        _lib.set_odd_dims("exhaustive")
    assert _lib.filter_dim(N, 12) == 0
