"""Pins what the quantiser's host dispatch decides: for a sweep of (filter kind, rows, n, dim) the eight words of
gqhip_debug_plan, gqhip_workspace_bytes, gqhip_cb_cache_bytes and gqhip_grid_search_applies, in the default environment and
under one diagnostic knob at a time.  All four are host-only: no GPU is needed.

    python tests/golden/make_golden_plan.py LIB            # writes tests/golden/plan_table.json from the build at LIB
    python tests/golden/make_golden_plan.py LIB --knobs    # prints the knob part of THIS process's environment as JSON

tests/test_plan_host.py imports the sweeps from here and compares the current build with the fixture, which was written from
a build of the commit before the dispatch was restructured (point LIB at such a build to regenerate it)."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "plan_table.json")

KINDS = (0, 1, 2, 3)                                 # gqhip_set_filter: auto, fp32, bf16, mixed
ROWS = (1, 100, 4096, 8191, 8192, 16384, 65536, 262144)
NS = (1, 31, 32, 1000, 16384, 65536, 1 << 20, (1 << 22) + 1, 1 << 23)
DIMS = (1, 4, 5, 8, 16, 32, 64)
# one knob per child process, over a handful of shapes (every filter kind each)
KNOBS = ("GQHIP_RT=1", "GQHIP_NSPLIT=1", "GQHIP_TARGET_BLOCKS=256", "GQHIP_BF16_WAVES=4", "GQHIP_BF16_CT=8", "GQHIP_GRID=0",
         "GQHIP_GRID=48", "GQHIP_IMG_CACHE=0", "GQHIP_FILTER=fp32", "GQHIP_FILTER=bf16", "GQHIP_FILTER=mixed")
KNOB_SHAPES = ((16384, 65536, 16), (4096, 65536, 16), (16384, 65536, 4), (100, 65536, 4), (16384, 65536, 8), (65536, 1 << 20, 8),
               (16384, 65536, 32), (262144, (1 << 22) + 1, 16), (100, 1000, 16), (16384, 65536, 5))


def load(path):
    L = ctypes.CDLL(path)
    i64 = ctypes.c_int64
    L.gqhip_debug_plan.argtypes = [i64, i64, i64, ctypes.POINTER(i64)]
    L.gqhip_workspace_bytes.restype = i64
    L.gqhip_workspace_bytes.argtypes = [i64, i64, i64]
    L.gqhip_cb_cache_bytes.restype = i64
    L.gqhip_cb_cache_bytes.argtypes = [i64, i64]
    L.gqhip_grid_search_applies.argtypes = [i64, i64]
    return L


def entry(L, rows, n, dim):
    """[the 8 plan words, workspace bytes, cache bytes, grid search applies]"""
    out = (ctypes.c_int64 * 8)()
    assert L.gqhip_debug_plan(rows, n, dim, out) == 0
    return list(out) + [L.gqhip_workspace_bytes(rows, n, dim), L.gqhip_cb_cache_bytes(n, dim), L.gqhip_grid_search_applies(n, dim)]


def table(L, shapes):
    """{filter kind: [entry per shape]}; the filter selection is restored afterwards."""
    before = L.gqhip_get_filter()
    try:
        out = {}
        for k in KINDS:
            assert L.gqhip_set_filter(k) == 0
            out[str(k)] = [entry(L, *s) for s in shapes]
        return out
    finally:
        L.gqhip_set_filter(before)


def default_shapes():
    return [(r, n, d) for r in ROWS for n in NS for d in DIMS]


def knob_part(L):
    return {"initial_filter": L.gqhip_get_filter(), "kinds": table(L, KNOB_SHAPES)}


def knob_part_in_child(lib_path, knob):
    """The knob part as a fresh process with that one knob set sees it (the library reads its knobs once per process)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("GQHIP_")}
    name, value = knob.split("=")
    env[name] = value
    out = subprocess.run([sys.executable, os.path.abspath(__file__), lib_path, "--knobs"], env=env, capture_output=True, text=True,
                         check=True)
    return json.loads(out.stdout)


if __name__ == "__main__":
    lib_path = os.path.abspath(sys.argv[1])
    if "--knobs" in sys.argv[2:]:
        print(json.dumps(knob_part(load(lib_path))))
    else:
        assert not [k for k in os.environ if k.startswith("GQHIP_")], "generate the fixture in the default environment"
        fixture = {"default": table(load(lib_path), default_shapes()),
                   "knobs": {knob: knob_part_in_child(lib_path, knob) for knob in KNOBS}}
        with open(FIXTURE, "w") as f:
            json.dump(fixture, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {FIXTURE}: {len(default_shapes())} shapes x {len(KINDS)} kinds, {len(KNOBS)} knobs")
