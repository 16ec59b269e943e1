"""-m gpu: the codebook index itself, as the one-block builders leave it in the codebook cache (csrc/gq_index.h; dims 4 / 8 for
gq_grid.h, dims 1-3 for gq_lowdim.h) -- read back through ``Workspace.cache_buf`` after one arg-max call and checked word by word against
a model of the layout (tests/golden/make_golden_index.py), one set of assertions for both builders; and that its deterministic parts are
the recorded ones (tests/golden/index_digests.json, written by the build before the builders were made one).

Books: finite (a NaN box has no unique byte image; the NaN and inf books are in test_gpu_grid.py / test_gpu_low_dims.py).  The dim-8
index exists only under GQHIP_GRID=48, read once per process: those cases are observed by ONE child process."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_index", os.path.join(ROOT, "tests", "golden", "make_golden_index.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)
GOLDEN = json.load(open(M.FIXTURE))

pytestmark = pytest.mark.gpu


def _model_matches_the_library():
    """the layout model's total is the library's cache size (host-only; dim 8 asserts the same inside its child process)"""
    from pit_hip import _lib

    if not os.path.exists(_lib.LIB_PATH):      # (nothing is built during collection; every observation repeats the check)
        return
    prev = _lib.get_low_dims()
    _lib.set_low_dims("search")
    try:
        for dim, n, _ in M.CASES:
            if dim != 8 or _lib.lib().gqhip_grid_search_applies(n, 8):
                assert _lib.lib().gqhip_cb_cache_bytes(n, dim) == M.layout(n, dim)["total"], (n, dim)
    finally:
        _lib.set_low_dims(prev)


_model_matches_the_library()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("index")


@functools.lru_cache(maxsize=None)
def _seen(case, tmp):
    """(the raw observation, the parsed first index, the parsed rebuilt index) of a case, observed once"""
    dim, n, _ = case
    obs = M.observe_any(case, tmp)
    return obs, M.parse(obs["first_cache"], n, dim), M.parse(obs["rebuilt_cache"], n, dim)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


cases = pytest.mark.parametrize("case", M.CASES, ids=M.case_id)


@cases
def test_header_and_start_arrays(case, tmp):
    dim, n, _ = case
    obs, p, _ = _seen(case, tmp)
    assert (p["magic"], p["n"], p["dim"], p["stale"]) == (M.MAGIC[M.kind_of(dim)], n, dim, 0)
    assert np.array_equal(p["blk_sum"], obs["first_cbsum"])
    start = p["start"]
    assert start[0] == 0 and (np.diff(start[:M.BUCKETS + 1]) >= 0).all() and (start[M.BUCKETS:] == n).all()
    if "leaf_start" in p:
        assert np.array_equal(p["leaf_start"][:1024], start[0:M.BUCKETS:4]) and (p["leaf_start"][1024:] == n).all()


@cases
def test_codes_are_scattered_whole_and_boxes_are_tight(case, tmp):
    dim, n, kind = case
    _, p, _ = _seen(case, tmp)
    cb = M.book(kind, n, dim).numpy()
    assert np.array_equal(np.sort(p["sidx"]), np.arange(n))
    assert np.array_equal(_bits(p["scb"]), _bits(cb[p["sidx"]]))
    start = p["start"][:M.BUCKETS + 1]
    size = np.diff(start)
    full = size > 0
    want = np.empty((M.BUCKETS, 2, dim), np.float32)
    want[:, 0], want[:, 1] = np.inf, -np.inf                       # an empty bucket: lo = +inf, hi = -inf
    want[full, 0] = np.minimum.reduceat(p["scb"], start[:-1][full], axis=0)
    want[full, 1] = np.maximum.reduceat(p["scb"], start[:-1][full], axis=0)
    assert (~full).any()
    assert np.array_equal(_bits(p["boxes"][0]), _bits(want))
    for (_, fan), child, parent in zip(M.layout(n, dim)["levels"][1:], p["boxes"], p["boxes"][1:]):
        kids = child.reshape(-1, fan, 2, dim)
        union = np.stack([kids[:, :, 0].min(axis=1), kids[:, :, 1].max(axis=1)], axis=1)
        assert np.array_equal(_bits(parent), _bits(union)), fan


@cases
def test_census_and_the_degenerate_answer(case, tmp):
    dim, n, kind = case
    obs, p, _ = _seen(case, tmp)
    largest = int(np.diff(p["start"][:M.BUCKETS + 1]).max())
    assert p["max_sub"] == largest
    assert int(obs["first_degenerate"]) == (1 if largest > M.cap_of(n, dim) else 0)
    assert (largest > M.cap_of(n, dim)) == (kind == "clustered")      # the books exercise both answers


@cases
def test_a_clobbered_cache_is_rebuilt_to_the_same_index_and_the_recorded_one(case, tmp):
    dim, n, _ = case
    obs, p, q = _seen(case, tmp)
    assert np.array_equal(obs["first_idx"], obs["rebuilt_idx"])
    assert int(obs["rebuilt_degenerate"]) == int(obs["first_degenerate"])
    assert M.deterministic_parts(q, dim) == M.deterministic_parts(p, dim)
    assert M.digests(p, dim) == GOLDEN[M.case_id(case)]
