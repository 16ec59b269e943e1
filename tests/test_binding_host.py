"""CPU: the ctypes signatures pit_hip._lib derives from include/gqhip.h, and the argument conversion of its one call path
(_call_args: a pure function of the entry's name and the caller's arguments -- no launch, no GPU)."""
import ctypes
import os
import re

import pytest
import torch

VP, I, I64, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
SCALARS = (I, I64, F, D)

SYNTHETIC = """
/* a block comment with a prototype inside:
 * int inside_block_comment(int a);
 */
typedef struct thing thing_t;
int no_arguments(void);
// int inside_line_comment(float x);
int64_t every_scalar(int a, int64_t b, float c, double d);   // int after_code_on_the_line(void);
const char *pointers(const float *in, void *out, thing_t *opaque, const int32_t *x_host, double *y_host, void *stream);
int broken_over_lines(const float *x,
                      int64_t n, /* a comment between parameters */
                      float scale);
"""


def _lib():
    from pit_hip import _lib as L

    return L


def test_parser_on_a_synthetic_header():
    L = _lib()
    signatures, params = L._parse_header(SYNTHETIC)
    assert signatures == {
        "no_arguments": (I, []),
        "every_scalar": (I64, [I, I64, F, D]),
        "pointers": (ctypes.c_char_p, [VP, VP, VP, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(D), VP]),
        "broken_over_lines": (I, [VP, I64, F]),
    }
    assert params == {
        "no_arguments": (),
        "every_scalar": ("a", "b", "c", "d"),
        "pointers": ("in", "out", "opaque", "x_host", "y_host", "stream"),
        "broken_over_lines": ("x", "n", "scale"),
    }


@pytest.mark.parametrize("prototype", [
    "int unknown_scalar(size_t n);",                 # a width the mapping does not list
    "int by_value(thing_t t);",                      # a typedef passed by value
    "int pointer_to_pointer(float **rows);",
    "int unknown_host_element(const uint8_t *mask_host);",
    "int unnamed(int);",
    "int two_words(unsigned int n);",
])
def test_parser_refuses_what_it_does_not_know(prototype):
    L = _lib()
    with pytest.raises(L.GqHipError, match=re.search(r"int (\w+)\(", prototype).group(1)):
        L._parse_header(SYNTHETIC + prototype + "\n")


def test_parser_on_the_real_header():
    """Every argument is of a known kind; the typed pointers are exactly the *_host parameters (so no device pointer is typed
    and none is named *_host).  That the names are the library's exports is test_host.py's."""
    L = _lib()
    assert set(L._SIGNATURES) == set(L._PARAMS) == set(L.EXPORTED_SYMBOLS) and len(L._SIGNATURES) >= 95
    host_elements = {ctypes.POINTER(t) for t in (I, I64, D, ctypes.c_int32, F)}
    typed, named_host = set(), set()
    for name, (restype, argtypes) in L._SIGNATURES.items():
        assert restype in (I, I64, ctypes.c_char_p), name
        assert len(argtypes) == len(L._PARAMS[name]), name
        for t, p in zip(argtypes, L._PARAMS[name]):
            assert t in SCALARS or t is VP or t in host_elements, (name, p, t)
            if t not in SCALARS and t is not VP:
                typed.add((name, p))
            if p.endswith("_host"):
                named_host.add((name, p))
            if p == "stream":
                assert t is VP and p == L._PARAMS[name][-1], name
    assert typed == named_host
    assert ("gqhip_debug_plan", "out8_host") in typed and ("fsq_train_f32", "levels_host") in typed and len(typed) == 10
    # both float widths are in the ABI on purpose
    assert L._SIGNATURES["gq_quantize_z_f32"][1].count(D) == 3 and L._SIGNATURES["lfq_train_f32"][1].count(F) == 2


def test_a_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    L = _lib()
    monkeypatch.setattr(L, "_CSRC", str(tmp_path / "a" / "csrc"))
    with pytest.raises(L.GqHipError, match=re.escape(os.path.join(str(tmp_path), "include", "gqhip.h"))):
        L._read_header()


def _convert(name, **by_name):
    """_call_args of ``name`` with arguments given by parameter name -> ({parameter: converted value}, the raw result)."""
    L = _lib()
    names = [p for p in L._PARAMS[name] if p != "stream"]
    assert set(by_name) == set(names), sorted(set(names) ^ set(by_name))
    got = L._call_args(name, tuple(by_name[p] for p in names))
    assert len(got) == len(names) == len(L._PARAMS[name]) - 1      # the stream slot is _call's, not the caller's
    return dict(zip(names, got)), got


def test_conversion_lfq_train():
    x, q, idx, avg, sc = (torch.zeros(4) for _ in range(5))
    got, raw = _convert("lfq_train_f32", x=x, quantized=q, idx=idx, avg=avg, scalars=sc, B=True, L=2, C=3, nc=1, d=3, layout=False,
                        w_s=1, w_b=2.5, workspace=4096, workspace_bytes=64)
    assert [got[k] for k in ("x", "quantized", "idx", "avg", "scalars")] == [t.data_ptr() for t in (x, q, idx, avg, sc)]
    assert got["B"] == 1 and type(got["B"]) is int and got["layout"] == 0 and type(got["layout"]) is int
    assert got["w_s"] == 1.0 and type(got["w_s"]) is float and got["w_b"] == 2.5
    assert got["workspace"] == 4096 and got["workspace_bytes"] == 64          # an int address stays
    # what was converted is what ctypes accepts for the declared types
    fn = ctypes.CFUNCTYPE(*_lib()._SIGNATURES["lfq_train_f32"][:1], *_lib()._SIGNATURES["lfq_train_f32"][1])
    assert fn(lambda *a: 0)(*raw, None) == 0


def test_conversion_gq_quantize_z():
    z, cb, idx, zhat = (torch.zeros(8) for _ in range(4))
    got, _ = _convert("gq_quantize_z_f32", z=z, noise_or_null=None, cb=cb, idx=idx, zhat_or_null=zhat, zhat_noquant_or_null=None,
                      mu_out_or_null=None, sd_out_or_null=None, B=1, L=2, c=4, dim=4, n=16, layout=1, grouping=True, lv_min=-30,
                      lv_max=20, beta=1, workspace=None, workspace_bytes=0, cb_cache_or_null=None, cb_cache_bytes=0)
    assert got["z"] == z.data_ptr() and got["noise_or_null"] is None and got["workspace"] is None
    assert got["grouping"] == 1 and type(got["grouping"]) is int
    for k, v in (("lv_min", -30.0), ("lv_max", 20.0), ("beta", 1.0)):          # the quantiser entries take double
        assert got[k] == v and type(got[k]) is float


def test_conversion_lpips_head():
    f0, f1, w, out = (torch.zeros(8) for _ in range(4))
    keep = torch.zeros(8, dtype=torch.uint8)
    got, _ = _convert("lpips_head_f32", f0=f0, f1=f1, w=w, keep_or_null=keep, keep_scale=2, out=out, B=1, C=2, HW=4, layout=0,
                      workspace=None, workspace_bytes=0)
    assert got["keep_or_null"] == keep.data_ptr() and got["keep_scale"] == 2.0 and type(got["keep_scale"]) is float
    assert got["workspace"] is None and got["out"] == out.data_ptr()


@pytest.mark.parametrize("name", ["lfq_train_f32", "gq_quantize_z_f32", "lpips_head_f32"])
def test_a_wrong_argument_count_names_the_entry(name):
    L = _lib()
    n = len(L._PARAMS[name]) - 1
    for count in (n - 1, n + 1):          # n + 1: a caller that passes the stream itself
        with pytest.raises(L.GqHipError, match=name):
            L._call_args(name, (0,) * count)


def test_typed_host_pointers_pass_through():
    L = _lib()
    levels = (ctypes.c_int32 * 3)(8, 5, 5)
    z = torch.zeros(6)
    got = L._call_args("fsq_quantize_f32", (z, levels, 3, z, z, 2))
    assert got[1] is levels and got[0] == z.data_ptr() and got[2] == 3
