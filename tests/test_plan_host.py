"""What the quantiser's host dispatch decides -- launch plan, workspace and cache sizes, which shapes run the grid search -- equals,
word for word, the table recorded before that dispatch was restructured (tests/golden/plan_table.json, written by
tests/golden/make_golden_plan.py).  Host-only: no GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_plan", os.path.join(ROOT, "tests", "golden", "make_golden_plan.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)
GOLDEN = json.load(open(P.FIXTURE))


def _lib_path():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.LIB_PATH


def _first_difference(got, want, shapes):
    for kind in want:
        for shape, g, w in zip(shapes, got[kind], want[kind]):
            if g != w:
                return f"filter kind {kind}, (rows, n, dim) = {shape}: got {g}, recorded {w}"
    return None


def test_the_issue_example_is_in_the_table():
    at = P.default_shapes().index((16384, 65536, 16))
    assert GOLDEN["default"]["0"][at] == [8192, 16, 4, 256, 3, 16700, 2, 8, 16097280, 4231168, 0]
    assert GOLDEN["default"]["1"][at] == [8192, 8, 2, 256, 0, 36, 2, 4, 8134656, 0, 0]
    assert GOLDEN["default"]["2"][at] == [8192, 8, 4, 256, 1, 604, 2, 8, 18685952, 0, 0]
    assert GOLDEN["default"]["3"][at] == [8192, 16, 4, 256, 2, 2450, 2, 8, 20848640, 0, 0]


def test_plan_and_sizes_in_the_default_environment():
    knobs_set = sorted({k.split("=")[0] for k in P.KNOBS} & set(os.environ))
    assert not knobs_set, f"this test pins the default environment; unset {knobs_set}"
    L = P.load(_lib_path())
    before = L.gqhip_get_filter()
    shapes = P.default_shapes()
    assert len(shapes) == 8 * 9 * 7 and sorted(GOLDEN["default"]) == ["0", "1", "2", "3"]
    got = P.table(L, shapes)
    assert L.gqhip_get_filter() == before
    assert all(len(GOLDEN["default"][k]) == len(shapes) for k in GOLDEN["default"])
    assert got == GOLDEN["default"], _first_difference(got, GOLDEN["default"], shapes)


@pytest.mark.parametrize("knob", P.KNOBS)
def test_plan_and_sizes_under_one_knob(knob):
    want = GOLDEN["knobs"][knob]
    got = P.knob_part_in_child(_lib_path(), knob)
    assert got["initial_filter"] == want["initial_filter"]
    assert got["kinds"] == want["kinds"], _first_difference(got["kinds"], want["kinds"], P.KNOB_SHAPES)
    if knob.startswith("GQHIP_FILTER="):
        assert want["initial_filter"] == {"fp32": 1, "bf16": 2, "mixed": 3}[knob.split("=")[1]]
    else:
        assert want["initial_filter"] == 0
