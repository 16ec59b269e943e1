"""CPU: host-side logic of the product package -- the C-ABI library loads and exports
every symbol include/gqhip.h declares (no compute without a GPU), config factory,
encoder/decoder parity with the seeded goldens, CPU plumbing of BASELINE config[0],
and loud failure when tensors are not on a HIP device."""
import ctypes
import hashlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import gq_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(G, "meta.json")))


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


def test_cabi_exports_every_declared_symbol():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "gqhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"^(?:int|int64_t|const char \*)\s*\**([a-z_0-9]+)\s*\(", header, flags=re.M))
    assert len(declared) >= 22
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(dll, name), f"libgqhip.so does not export {name}"
    assert declared == set(L.EXPORTED_SYMBOLS), "python binding and header disagree"
    assert L.lib().gqhip_abi_version() == L.ABI_VERSION == 8
    assert L.lib().gqhip_status_string(2) == b"workspace missing or too small"


def test_groupnorm_statistics_arithmetic_on_the_host(tmp_path):
    """csrc/gq_stats.h compiled for the host (tests/stats_host_test.cpp): the integer split of fp32 addends equals the fp64
    split bit for bit over 300 000 addends (random bit patterns, edges, denormals, +-inf / NaN), sums are independent of the
    order of the adds, the limbs hold the EXACT integer sum of the truncated addends, non-finite addends poison the record."""
    import subprocess

    exe = str(tmp_path / "stats_host_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "stats_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout + out.stderr


def test_workspace_sizing_is_host_only_and_monotone():
    L = _lib().lib()
    a = L.gqhip_workspace_bytes(1024, 65536, 16)
    b = L.gqhip_workspace_bytes(16384, 65536, 16)
    assert 0 < a < b < (1 << 28)
    assert L.gqhip_workspace_bytes(16, 65536, 65) == -1  # dim > 64 rejected
    assert L.gqhip_workspace_bytes(16, 0, 16) == -1


def test_codebook_cache_sizing_is_host_only_and_pins_the_index_layout():
    """gqhip.h:gqhip_cb_cache_bytes -- dim 4 (2^14 <= n <= 2^20): the search index of csrc/gq_grid.h:grid_layout = header 4 KiB, boxes of
    16 + 256 + 1024 nodes, leaf ranges, sub-leaf ranges, 4096 sub-leaf boxes, the codes sorted by sub-leaf, their original ids (every
    table rounded up to 256 B); dims 8 / 16 / 32: header + the filter's fp16 operand image (32 / 64 / 128 B per code); nothing else."""
    L = _lib().lib()

    def al(v):
        return (v + 255) // 256 * 256

    for n in (16384, 65536, 70001, 1 << 20):
        want = 4096 + (16 + 256 + 1024) * 32 + al((1024 + 16) * 4) + al((4096 + 16) * 4) + 4096 * 32 + al(n * 16) + al(n * 4)
        assert L.gqhip_cb_cache_bytes(n, 4) == want
        assert L.gqhip_grid_search_applies(n, 4) == 1
    assert L.gqhip_cb_cache_bytes(65536, 4) == 1508352
    assert L.gqhip_cb_cache_bytes(16383, 4) == 0 and L.gqhip_cb_cache_bytes((1 << 20) + 1, 4) == 0
    assert L.gqhip_grid_search_applies(65536, 8) == 0 and L.gqhip_grid_search_applies(65536, 16) == 0
    img = {d: L.gqhip_cb_cache_bytes(65536, d) for d in (8, 16, 32)}
    assert img[8] > 4096 and img[16] >= 4096 + 65536 * 64 and img[32] > img[16] > img[8]
    assert L.gqhip_cb_cache_bytes(65536, 5) == 0 and L.gqhip_cb_cache_bytes(65536, 64) == 0


def test_invalid_arguments_return_status_not_crash():
    L = _lib().lib()
    assert L.gq_argmax_f32(None, None, None, None, None, None, 16, 4, 1024, 1.0, None, 0, None, 0, None) == 1
    assert L.gq_scores_f32(None, None, None, None, 16, 4, 1024, 1.0, None) == 1
    assert L.lfq_pack_f32(None, None, None, 4, 16, None) == 1


_NAN = float("nan")
_GN_C = [dict(C=0), dict(C=96), dict(C=130), dict(C=2048), dict(C=512, groups=64), dict(C=512, groups=128)]
_GN_G = [dict(groups=0), dict(groups=5), dict(groups=128)]
_WINO2 = [dict(B=-1), dict(H=0), dict(H=1), dict(H=7), dict(W=1), dict(W=7), dict(C=0), dict(C=2), dict(C=6)]
_WINO4 = [dict(B=-1), dict(H=2), dict(H=6), dict(W=2), dict(W=6), dict(C=0), dict(C=2), dict(C=6)]
_TILE = [dict(tile=4), dict(tile=3), dict(tile=0), dict(tile=4, H=6), dict(tile=4, W=6), dict(tile=4, H=2)]
_SCALE = [dict(scale=0.0), dict(scale=-1.0), dict(scale=_NAN)]
_SCALE_DEV = _SCALE + [dict(scale=0.0, scales_dev=None), dict(scale=_NAN, scales_dev=None), dict(scales_dev=None)]
_GOUT = [dict(groups_out=0), dict(groups_out=5), dict(groups_out=64), dict(groups_out=1), dict(groups_out=5, stats_out=None)]
# The conv-stack entry points of csrc/gqhip_unet.hip: entry: (argument names in the order of the C signature, one
# valid set of the shape / scalar arguments, perturbations of it).  Pointer arguments are those _SIGNATURES declares void *;
# a perturbation may null some.  The first argument of _EMPTY that an entry point has is the one whose 0 means "nothing to do".
_EMPTY = ("B", "rows", "tiles", "count", "n_bg")
_CABI = {
    "gn_silu_f32": ("x gamma beta pre_bias y B C HW groups eps apply_silu layout stats_ws stream",
                    dict(B=1, C=128, HW=64, groups=32, eps=1e-6, apply_silu=1, layout=1),
                    [dict(B=-1), dict(HW=0), dict(HW=6), dict(layout=0), dict(layout=2), dict(layout=0, HW=6), dict(layout=0, C=96),
                     dict(apply_silu=0), dict(pre_bias=None)] + _GN_C + _GN_G),
    "add_bias_f32": ("a b bias y B C HW layout stream", dict(B=1, C=128, HW=64, layout=1),
                     [dict(B=-1), dict(C=0), dict(C=6), dict(HW=0), dict(HW=6), dict(layout=0), dict(layout=2), dict(layout=0, HW=6),
                      dict(layout=0, C=6), dict(bias=None)]),
    "add_bias_stats_f32": ("a b bias y B C HW groups stats_out stream", dict(B=1, C=128, HW=64, groups=32),
                           [dict(B=-1), dict(HW=0), dict(HW=6), dict(bias=None)] + _GN_C + _GN_G),
    "gn_apply_f32": ("x gamma beta y B C HW groups eps apply_silu stats stream",
                     dict(B=1, C=128, HW=64, groups=32, eps=1e-6, apply_silu=1),
                     [dict(B=-1), dict(HW=0), dict(apply_silu=0)] + _GN_C + _GN_G),
    "gn_stats_f32": ("x pre_bias B C HW groups stats_out stream", dict(B=1, C=128, HW=64, groups=32),
                     [dict(B=-1), dict(HW=0), dict(pre_bias=None)] + _GN_C + _GN_G),
    "wino_in_nhwc_f32": ("x V B H W C stream", dict(B=1, H=8, W=8, C=8), _WINO2 + [dict(H=6)]),
    "wino4_in_nhwc_f32": ("x V B H W C stream", dict(B=1, H=8, W=8, C=8), _WINO4),
    "wino_out_nhwc_f32": ("M y B H W C mscale stream", dict(B=1, H=8, W=8, C=8, mscale=1.0), _WINO2 + [dict(mscale=0.0)]),
    "wino4_out_nhwc_f32": ("M y B H W C mscale stream", dict(B=1, H=8, W=8, C=8, mscale=1.0), _WINO4 + [dict(mscale=0.0)]),
    "wino_in_nhwc_f16x3": ("x V3 B H W C tile scale stream", dict(B=1, H=8, W=8, C=8, tile=2, scale=1.0), _WINO2 + _TILE + _SCALE),
    "wino_in_nhwc_f16x2": ("x V2 B H W C tile scale stream", dict(B=1, H=8, W=8, C=8, tile=2, scale=1.0), _WINO2 + _TILE + _SCALE),
    "wino_gemm_f16x2": ("V2 Wf M P tiles Cin Cout stream", dict(P=16, tiles=256, Cin=64, Cout=256),
                        [dict(P=0), dict(P=1 << 31), dict(tiles=-256), dict(tiles=128), dict(tiles=0x40000000), dict(Cin=0), dict(Cin=16),
                         dict(Cin=32), dict(Cin=48), dict(Cin=4128), dict(Cout=0), dict(Cout=64), dict(Cout=128), dict(Cout=192),
                         dict(Cout=4224)]),
    "wino_in_gn_nhwc_f32": ("x gamma beta pre_bias stats V B H W C groups eps apply_silu stream",
                            dict(B=1, H=8, W=8, C=128, groups=32, eps=1e-6, apply_silu=1),
                            _WINO2 + [dict(groups=0), dict(groups=5), dict(groups=64), dict(apply_silu=0), dict(pre_bias=None)]),
    "wino4_in_gn_nhwc_f32": ("x gamma beta pre_bias stats V B H W C groups eps apply_silu stream",
                             dict(B=1, H=8, W=8, C=128, groups=32, eps=1e-6, apply_silu=1),
                             _WINO4 + [dict(groups=0), dict(groups=5), dict(groups=64), dict(apply_silu=0), dict(pre_bias=None)]),
    "wino_in_gn_nhwc_f16x3": ("x gamma beta pre_bias stats V3 B H W C groups eps apply_silu tile scale stream",
                              dict(B=1, H=8, W=8, C=128, groups=32, eps=1e-6, apply_silu=1, tile=2, scale=1.0),
                              _WINO2 + _TILE + _SCALE + [dict(groups=0), dict(groups=5), dict(groups=64), dict(apply_silu=0),
                                                         dict(apply_silu=0, tile=4)]),
    "wino_in_gn_nhwc_f16x2": ("x gamma beta pre_bias stats V2 B H W C groups eps apply_silu tile scale stream",
                              dict(B=1, H=8, W=8, C=128, groups=32, eps=1e-6, apply_silu=1, tile=2, scale=1.0),
                              _WINO2 + _TILE + _SCALE + [dict(groups=0), dict(groups=5), dict(groups=64), dict(apply_silu=0),
                                                         dict(apply_silu=0, tile=4)]),
    "conv3x3_gn_f16x3": ("x gamma beta pre_bias stats_in groups_in eps apply_silu scale Wf bias res y stats_out B H W Cin Cout "
                         "groups_out mscale stream",
                         dict(groups_in=32, eps=1e-6, apply_silu=1, scale=1.0, B=1, H=8, W=32, Cin=64, Cout=128, groups_out=32, mscale=1.0),
                         [dict(B=-1), dict(H=0), dict(H=4), dict(H=12), dict(H=131080), dict(W=16), dict(W=48), dict(Cin=0), dict(Cin=16),
                          dict(Cin=48), dict(Cin=544), dict(Cout=64), dict(Cout=256), dict(Cout=512), dict(groups_in=0), dict(groups_in=5),
                          dict(apply_silu=0), dict(apply_silu=0, Cout=256), dict(bias=None, res=None, pre_bias=None)] + _SCALE + _GOUT),
    "conv1x1_f16x3": ("x pre_bias Wf scales_dev scale mscale bias res y stats_out B HW Cin Cout groups_out stream",
                      dict(scale=1.0, mscale=1.0, B=1, HW=256, Cin=64, Cout=128, groups_out=32),
                      [dict(B=-1), dict(HW=0), dict(HW=64), dict(HW=128), dict(HW=384), dict(HW=512), dict(HW=(1 << 24) + 128), dict(Cin=0),
                       dict(Cin=16), dict(Cin=48), dict(Cout=64), dict(Cout=256), dict(Cout=512), dict(Cout=1024), dict(Cout=1536),
                       dict(bias=None, res=None, pre_bias=None)] + _SCALE_DEV + _GOUT),
    "conv1x1_gn_f16x3": ("x gamma beta pre_bias stats_in groups_in eps Wf scale mscale bias res y stats_out B HW Cin Cout groups_out "
                         "stream",
                         dict(groups_in=16, eps=1e-6, scale=1.0, mscale=1.0, B=1, HW=256, Cin=64, Cout=128, groups_out=32),
                         [dict(B=-1), dict(HW=0), dict(HW=64), dict(HW=128), dict(HW=384), dict(Cin=0), dict(Cin=16), dict(Cin=48),
                          dict(Cin=544), dict(Cout=64), dict(Cout=256), dict(Cout=512), dict(Cout=1024), dict(Cout=1536), dict(groups_in=0),
                          dict(groups_in=5), dict(groups_in=32)] + _SCALE + _GOUT),
    "conv1x1_qkv_split_f16x3": ("x gamma beta pre_bias stats_in groups_in eps Wf scale mscale bias Q3 K3 V3 sq sv B L C stream",
                                dict(groups_in=32, eps=1e-6, scale=1.0, mscale=1.0, sq=1.0, sv=1.0, B=1, L=256, C=128),
                                [dict(B=-1), dict(L=0), dict(L=64), dict(L=128), dict(L=384), dict(C=0), dict(C=64), dict(C=192), dict(C=512),
                                 dict(C=640), dict(groups_in=0), dict(groups_in=5), dict(groups_in=64), dict(sq=0.0), dict(sq=_NAN),
                                 dict(sv=0.0), dict(sv=_NAN), dict(gamma=None, groups_in=0), dict(gamma=None, C=640),
                                 dict(gamma=None, beta=None, stats_in=None)] + _SCALE),
    "conv3x3s2_f16x3": ("x Wf scales_dev scale mscale bias y stats_out B Hin Win Cin Cout groups_out stream",
                        dict(scale=1.0, mscale=1.0, B=1, Hin=16, Win=64, Cin=16, Cout=128, groups_out=32),
                        [dict(B=-1), dict(Hin=0), dict(Hin=8), dict(Hin=24), dict(Win=32), dict(Win=96), dict(Win=(1 << 20) + 64),
                         dict(Cin=0), dict(Cin=8), dict(Cin=24), dict(Cout=64), dict(Cout=256), dict(Cout=512), dict(Cout=1024)]
                        + _SCALE_DEV + _GOUT),
    "upconv2x_f16x3": ("x Wf scales_dev scale mscale bias y stats_out B H W Cin Cout groups_out stream",
                       dict(scale=1.0, mscale=1.0, B=1, H=8, W=32, Cin=16, Cout=128, groups_out=32),
                       [dict(B=-1), dict(H=0), dict(H=4), dict(H=12), dict(H=131080), dict(W=16), dict(W=48), dict(Cin=0), dict(Cin=8),
                        dict(Cin=24), dict(Cout=64), dict(Cout=256), dict(Cout=512), dict(Cout=1024)] + _SCALE_DEV + _GOUT),
    "conv3x3_gn_small_f32": ("x gamma beta pre_bias stats_in groups_in eps apply_silu w_ohwi bias y B H W Cin Cout stream",
                             dict(groups_in=8, eps=1e-6, apply_silu=1, B=1, H=16, W=16, Cin=32, Cout=3),
                             [dict(B=-1), dict(B=1 << 31), dict(H=8), dict(H=24), dict(W=8), dict(W=24), dict(Cin=0), dict(Cin=16),
                              dict(Cin=48), dict(Cin=544), dict(Cout=0), dict(Cout=1), dict(Cout=2), dict(Cout=4), dict(Cout=5),
                              dict(groups_in=0), dict(groups_in=5), dict(apply_silu=0)]),
    "conv3x3_cin_small_f32": ("x wk bias y stats_out B H W Cin Cout groups_out stream",
                              dict(B=1, H=8, W=32, Cin=3, Cout=128, groups_out=32),
                              [dict(B=-1), dict(B=1 << 31), dict(H=4), dict(H=12), dict(W=16), dict(W=48), dict(Cin=0), dict(Cin=1),
                               dict(Cin=2), dict(Cin=4), dict(Cin=5), dict(Cout=64), dict(Cout=256), dict(groups_out=16), dict(groups_out=0),
                               dict(groups_out=16, stats_out=None)]),
    "conv3x3_f32": ("x gamma beta pre_bias stats groups_in eps apply_silu wk bias y B H W Cin Cout stream",
                    dict(groups_in=8, eps=1e-6, apply_silu=1, B=1, H=4, W=4, Cin=64, Cout=32),
                    [dict(B=-1), dict(B=1 << 31), dict(H=0), dict(W=0), dict(Cin=4), dict(Cin=8), dict(Cin=24), dict(Cin=128),
                     dict(Cin=1088), dict(Cout=0), dict(Cout=2), dict(Cout=4), dict(Cout=6), dict(groups_in=0), dict(groups_in=5),
                     dict(apply_silu=0), dict(gamma=None), dict(beta=None), dict(stats=None), dict(stats=None, Cin=8),
                     dict(stats=None, Cin=16), dict(stats=None, Cin=32), dict(stats=None, Cin=24), dict(stats=None, Cin=1088),
                     dict(stats=None, gamma=None, beta=None, groups_in=0)]),
    "wino_out_res_nhwc_f32": ("M res bias y stats_out B H W C groups tile mscale stream",
                              dict(B=1, H=8, W=8, C=128, groups=32, tile=2, mscale=1.0),
                              _WINO2 + _TILE + _GN_C + _GN_G + [dict(C=64), dict(tile=4, C=1024), dict(tile=4, C=512), dict(res=None),
                                                                dict(res=None, bias=None)]),
    "attn_split_qkv_f16x3": ("qkv Q3 K3 V3 B L C sq sv stream", dict(B=1, L=64, C=128, sq=1.0, sv=1.0),
                             [dict(B=-1), dict(L=0), dict(C=0), dict(C=2), dict(C=6), dict(sq=0.0), dict(sq=_NAN), dict(sv=0.0),
                              dict(sv=_NAN)]),
    "attn_softmax_split_f16x3": ("S P3 rows L factor stream", dict(rows=4, L=64, factor=1.0),
                                 [dict(rows=-1), dict(L=0), dict(L=32), dict(L=96), dict(L=128), dict(L=192), dict(L=256), dict(L=1024),
                                  dict(L=2304), dict(L=4096), dict(L=4160), dict(factor=0.0), dict(factor=_NAN)]),
    "f16_scales_from_gn_stats": ("stats n_bg amp u_scale scales_out stream", dict(n_bg=32, amp=1.0, u_scale=1.0),
                                 [dict(n_bg=-1), dict(n_bg=1 << 31), dict(amp=0.0), dict(amp=_NAN), dict(u_scale=0.0), dict(u_scale=_NAN)]),
    "upsample2x_nhwc_f32": ("x y B H W C stream", dict(B=1, H=4, W=4, C=8),
                            [dict(B=-1), dict(H=0), dict(W=0), dict(C=0), dict(C=2), dict(C=6)]),
    "gqhip_checksum_tensors": ("table count sums stream", dict(count=4), [dict(count=-1), dict(count=65535), dict(count=65536)]),
}
# the switches an entry point reads per call, with every value its code tells apart (None: unset)
_CABI_ENV = {"wino_gemm_f16x2": ("GQHIP_WGEMM", (None, "128", "w8", "w4")),
             "conv1x1_f16x3": ("GQHIP_CONV1_TILE", (None, "128", "256")),
             "conv1x1_gn_f16x3": ("GQHIP_CONV1_TILE", (None, "128", "256")),
             "conv1x1_qkv_split_f16x3": ("GQHIP_CONV1_TILE", (None, "128", "256"))}


def _cabi_status_cases(L):
    """Yields (entry, case id, thunk returning the status) over the families of test_conv_stack_cabi_status_table."""
    fake = 0x10000          # never dereferenced: see the test's docstring
    for entry, (names, base, perturbations) in _CABI.items():
        names = names.split()
        argtypes = L._SIGNATURES[entry][1]
        assert len(names) == len(argtypes) and set(base) <= set(names), entry
        ptrs = [n for n, t in zip(names, argtypes) if t is ctypes.c_void_p and n != "stream"]
        empty = next(n for n in _EMPTY if n in names)
        fn = getattr(L.lib(), entry)

        def case(cid, scalars, nulls):
            vals = dict(base, **{p: (None if p in nulls else fake) for p in ptrs}, stream=None)
            vals.update(scalars)
            args = [vals[n] for n in names]
            return entry, cid, (lambda: fn(*args))

        def ident(p):
            return ",".join("%s=%r" % kv for kv in p.items()) or "base"

        some = [p for p in perturbations if empty not in p]
        yield case("empty/null", {empty: 0}, ptrs)
        for p in some:
            yield case("empty/null/" + ident(p), dict(p, **{empty: 0}), ptrs)
        for p in [{}] + some:
            yield case("empty/fake/" + ident(p), dict(p, **{empty: 0}), ())
        yield case("one/null", {}, ptrs)
        for n in ptrs:
            yield case("one/null:" + n, {}, (n,))
        for p in [{}] + perturbations:
            yield case("one/fake/" + ident(p), p, ())


def _cabi_status_table(L):
    rows = []
    for entry, cid, call in _cabi_status_cases(L):
        knob, values = _CABI_ENV.get(entry, (None, (None,)))
        for v in values:
            old = os.environ.pop(knob, None) if knob else None
            try:
                if v is not None:
                    os.environ[knob] = v
                rows.append([entry, cid if v is None else "%s/%s=%s" % (cid, knob, v), call()])
            finally:
                if knob:
                    os.environ.pop(knob, None)
                    if old is not None:
                        os.environ[knob] = old
    return rows


def test_conv_stack_cabi_status_table():
    """Every conv-stack entry point of csrc/gqhip_unet.hip returns the status tests/golden/convstack_cabi_status.json records for
    it (recorded with this generator from the library as it was before the host layer's checks were brought together): with
    nothing to do and all pointers NULL or all set, with every pointer NULL, with each pointer NULL in turn, and with each
    shape / scalar argument out of its range in turn -- once per value of the GQHIP_WGEMM / GQHIP_CONV1_TILE switches.  Without a
    device an entry point that gets past its checks returns 3 ("kernel launch failed": no device) and launches nothing, so 0 / 1 /
    3 tell "empty", "refused" and "would launch" apart -- the ORDER of the checks included.
    SAFETY: the pointers passed are made up.  They are never dereferenced only because nothing can launch, so this test must
    never run where a HIP device is present: it skips there, whatever else is asked of it."""
    if torch.cuda.is_available():
        pytest.skip("passes made-up pointers: safe only where no kernel can launch")
    got = _cabi_status_table(_lib())
    want = json.load(open(os.path.join(G, "convstack_cabi_status.json")))
    assert len(got) == len(want) > 300 and {e for e, _, _ in got} == set(_CABI) and len(_CABI) == 31
    assert {s for _, _, s in got} == {0, 1, 3}
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:20]
    # the 256-pixel tiling forced where only 128-pixel tiles fit stays an invalid argument
    assert ["conv1x1_f16x3", "one/fake/HW=384/GQHIP_CONV1_TILE=256", 1] in got
    assert ["conv1x1_f16x3", "one/fake/HW=384", 3] in got


_RECORD_ENTRIES = {          # entry point: (argument names, its size function, that function's arguments)
    "gq_step_record_f32": ("x x_rec idx rec B per_image n_idx ws ws_bytes stream", "gq_step_record_workspace_bytes", "B per_image"),
    "gq_step_record_bits_f32": ("x x_rec idx rec B per_image n_idx index_bits n_codes ws ws_bytes stream",
                                "gq_step_record_bits_workspace_bytes", "B per_image"),
    "gq_step_record_ssim_f32": ("x x_rec idx rec B C H W layout n_idx ws ws_bytes stream", "gq_step_record_ssim_workspace_bytes",
                                "B C H W"),
    "gq_step_record_ssim_bits_f32": ("x x_rec idx rec B C H W layout n_idx index_bits n_codes ws ws_bytes stream",
                                     "gq_step_record_ssim_bits_workspace_bytes", "B C H W"),
}
_RECORD_SHAPES = ((1, 3, 5, 7), (2, 3, 64, 48), (16, 3, 256, 256), (3, 3, 257, 263))
_RECORD_REFUSED = ((-1, 3, 64, 48), (0, 3, 64, 48), ((1 << 30) + 1, 3, 64, 48), (2, 0, 64, 48), (2, 3, 0, 48), (2, 3, 64, 0))


def _record_cabi_table(lib):
    """[entry or size function, case id, status or byte count] over the families of test_record_cabi_status_table; ``lib``: a
    loaded libgqhip with the signatures set."""
    fake, ample = 0x10000, 1 << 62          # the pointer is never dereferenced: see the test's docstring
    rows = []
    for entry, (names, size_name, size_args) in _RECORD_ENTRIES.items():
        names, size_args = names.split(), size_args.split()
        fn, size = getattr(lib, entry), getattr(lib, size_name)
        bits, image = "index_bits" in names, "C" in names
        ptrs = ("x", "x_rec", "idx", "rec", "ws")
        base = dict(B=2, per_image=3 * 64 * 48, C=3, H=64, W=48, layout=0, n_idx=5, index_bits=18, n_codes=1 << 18, stream=None)

        def case(cid, nulls=(), ws_bytes=ample, **scalars):
            vals = dict(base, **{p: (None if p in nulls else fake) for p in ptrs}, ws_bytes=ws_bytes)
            assert set(scalars) <= set(vals), scalars
            vals.update(scalars)
            rows.append([entry, cid, fn(*[vals[n] for n in names])])

        need = size(*[base[n] for n in size_args])
        case("base")
        case("nothing/null", ptrs, 0, B=0, n_idx=0)
        case("nothing/fake", B=0, n_idx=0)
        case("all/null", ptrs)
        for p in ptrs[:4]:
            case("null:" + p, (p,))
        case("ws/null", ("ws",), need)
        case("ws/short", (), need - 1)
        case("ws/exact", (), need)
        for B in (-1, 0, 1, (1 << 30) + 1):
            case("B=%d" % B, B=B)
        case("B=0/ws/null", ("ws",), 0, B=0)
        case("B=0/images/null", ("x", "x_rec"), B=0)
        for n in ("C", "H", "W") if image else ("per_image",):
            case(n + "=0", **{n: 0})
        if image:
            case("layout=2", layout=2)
            case("layout=1", layout=1)
        for n_idx in (-1, 0, 1):
            case("n_idx=%d" % n_idx, n_idx=n_idx)
        case("n_idx=0/idx/null", ("idx",), n_idx=0)
        case("n_idx=2^62", n_idx=1 << 62)
        if bits:
            for w in (0, 1, 16, 32, 33):
                for n_codes in (0, 1, 1 << w, (1 << w) + 1):
                    case("index_bits=%d,n_codes=%d" % (w, n_codes), index_bits=w, n_codes=n_codes)
            case("n_idx=2^33,index_bits=32", n_idx=1 << 33, index_bits=32, n_codes=1)      # the ticket field of the violations word
            case("n_idx=2^33,index_bits=32/ws/short", (), 0, n_idx=1 << 33, index_bits=32, n_codes=1)
        # B x chunks beyond 2^30: refused, but only behind the workspace check
        big = dict(B=1 << 20, C=1, H=4096, W=4096) if image else dict(B=1 << 20, per_image=1 << 24)
        case("B*chunks=2^31", **big)
        case("B*chunks=2^31/ws/short", (), 0, **big)
        for B, C, H, W in _RECORD_SHAPES + _RECORD_REFUSED:
            args = (B, C, H, W) if image else (B, C * H * W)
            rows.append([size_name, "x".join(map(str, args)), size(*args)])
    return rows


def test_record_cabi_status_table():
    """The four step-record entry points of csrc/gqhip.hip return the status, and their four size functions the byte count, that
    tests/golden/record_cabi_status.json records (recorded with this generator from the library as it was before the record's
    checks and workspace layout were brought together in one plan): nothing to do with all pointers NULL or set, each pointer NULL
    in turn, the workspace NULL / one byte short / exact, and each shape, count and index-format argument out of its range in
    turn.  Without a device an entry point that gets past its checks returns 3 ("kernel launch failed": no device) and launches
    nothing, so 0 / 1 / 2 / 3 tell "empty", "refused", "workspace" and "would launch" apart -- the ORDER of the checks included.
    SAFETY: the pointers passed are made up.  They are never dereferenced only because nothing can launch, so this test must
    never run where a HIP device is present: it skips there, whatever else is asked of it."""
    if torch.cuda.is_available():
        pytest.skip("passes made-up pointers: safe only where no kernel can launch")
    got = _record_cabi_table(_lib().lib())
    want = json.load(open(os.path.join(G, "record_cabi_status.json")))
    assert len(got) == len(want) > 150 and {e for e, _, _ in got} == set(_RECORD_ENTRIES) | {v[1] for v in _RECORD_ENTRIES.values()}
    assert {s for e, _, s in got if e in _RECORD_ENTRIES} == {0, 1, 2, 3}
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:20]
    # a few of the rules, spelled out: only gq_step_record_f32 has "nothing to do"; the bit-packed records always want the workspace
    assert ["gq_step_record_f32", "nothing/null", 0] in got and ["gq_step_record_bits_f32", "nothing/null", 1] in got
    assert ["gq_step_record_f32", "B=0/ws/null", 3] in got and ["gq_step_record_bits_f32", "B=0/ws/null", 2] in got
    assert ["gq_step_record_ssim_f32", "B=0", 1] in got and ["gq_step_record_f32", "B*chunks=2^31/ws/short", 2] in got


_NC_D = [dict(C=15), dict(nc=9, d=7, C=63), dict(nc=31, d=2, C=62), dict(nc=0, C=0)]
_VQ_N = [dict(n=0), dict(n=1), dict(n=1 << 31)]
_TRAIN_ENTRIES = {       # entry point: (argument names, valid scalars, its size function as (name, arguments) or None, perturbations)
    "gq_gauss_train_f32": ("z noise zhat sd_out kl2row scalars_out lam_state B L c dim layout grouping lv_min lv_max log2n tolerance "
                           "lam_factor lam_lo lam_hi lam_max_decreases loss_divisor stream",
                           dict(B=2, L=36, c=16, dim=8, layout=0, grouping=0, lv_min=-30.0, lv_max=20.0, log2n=12.0, tolerance=0.5,
                                lam_factor=1.01, lam_lo=1e-7, lam_hi=1e7, lam_max_decreases=0, loss_divisor=144.0), None, []),
    "gq_gauss_backward_f32": ("z noise g_zhat g_sd g_kl lam_before grad_z B L c dim layout grouping lv_min lv_max log2n tolerance "
                              "loss_divisor stream",
                              dict(B=2, L=36, c=16, dim=8, layout=0, grouping=0, lv_min=-30.0, lv_max=20.0, log2n=12.0, tolerance=0.5,
                                   loss_divisor=144.0), None, []),
    "vq_quantize_z_f32": ("z emb idx zq loss2 B L c dim n layout beta legacy workspace workspace_bytes cb_cache cb_cache_bytes stream",
                          dict(B=2, L=36, c=16, dim=8, n=1024, layout=0, beta=0.25, legacy=1, cb_cache_bytes=0),
                          ("gqhip_workspace_bytes", "rows n dim"), _VQ_N + [dict(n=1 << 30), dict(legacy=0)]),
    "vq_backward_f32": ("z emb idx g_zq g_loss grad_z grad_emb B L c dim n layout beta legacy workspace workspace_bytes stream",
                        dict(B=2, L=36, c=16, dim=8, n=1024, layout=0, beta=0.25, legacy=1),
                        ("vq_backward_workspace_bytes", "rows n dim"),
                        _VQ_N + [dict(legacy=0), dict(grad_z=None, grad_emb=None), dict(g_loss=None, grad_emb=None),
                                 dict(B=0, grad_emb=None), dict(L=0, grad_emb=None)]),
    "lfq_train_f32": ("x quantized idx avg scalars B L C nc d layout w_s w_b workspace workspace_bytes stream",
                      dict(B=2, L=36, C=16, nc=2, d=8, layout=0, w_s=1.0, w_b=1.0), ("lfq_train_workspace_bytes", "rows d"),
                      _NC_D + [dict(B=1 << 15, L=1 << 14, nc=2, d=1, C=2), dict(B=1 << 15, L=1 << 14, nc=3, d=1, C=3)]),
    "lfq_backward_f32": ("x avg g_q g_aux g_commit grad_x B L C nc d layout w_s w_b workspace workspace_bytes stream",
                         dict(B=2, L=36, C=16, nc=2, d=8, layout=0, w_s=1.0, w_b=1.0), ("lfq_train_workspace_bytes", "rows d"),
                         _NC_D + [dict(B=1 << 15, L=1 << 14, nc=2, d=1, C=2), dict(B=1 << 15, L=1 << 14, nc=3, d=1, C=3),
                                  dict(d=16, nc=1, C=16), dict(d=5, nc=1, C=5), dict(d=12, nc=1, C=12)]),
    "bsq_train_f32": ("x quantized idx avg scalars B L C d layout w_s w_b workspace workspace_bytes stream",
                      dict(B=2, L=36, C=32, d=2, layout=0, w_s=1.0, w_b=1.0), ("bsq_train_workspace_bytes", "rows d"),
                      [dict(C=31), dict(C=16), dict(C=2)]),
    "bsq_backward_f32": ("x avg g_q g_aux grad_x B L C d layout w_s w_b workspace workspace_bytes stream",
                         dict(B=2, L=36, C=32, d=2, layout=0, w_s=1.0, w_b=1.0), ("bsq_train_workspace_bytes", "rows d"),
                         [dict(C=31), dict(C=16), dict(C=2)]),
    "fsq_train_f32": ("z levels_host nlev zhat idx B L layout stream", dict(B=2, L=36, layout=0), None, []),
    "fsq_backward_f32": ("z g_zhat levels_host nlev grad_z B L layout stream", dict(B=2, L=36, layout=0), None,
                         [dict(B=1 << 14, L=1 << 14, levels=[2] * 16), dict(B=1 << 15, L=1 << 14, levels=[2] * 16)]),
}
_TRAIN_SIZES = {         # size function: four valid shapes, then refused ones
    "vq_backward_workspace_bytes": ((1, 1, 1), (4096, 1024, 8), (0, 65536, 64), (0x3fffffff, 0x7fffffff, 64),
                                    (-1, 1024, 8), (1 << 30, 1024, 8), (4096, 0, 8), (4096, 1 << 31, 8), (4096, 1024, 0), (4096, 1024, 65)),
    "lfq_train_workspace_bytes": ((1, 1), (4096, 8), (0, 16), (0x3fffffff, 16), (-1, 8), (1 << 30, 8), (4096, 0), (4096, 17)),
    "bsq_train_workspace_bytes": ((1, 1), (4096, 2), (0, 16), (0x3fffffff, 16), (-1, 2), (1 << 30, 2), (4096, 0), (4096, 17)),
}


def _train_cabi_table(lib, signatures):
    """[entry or size function, case id, status or byte count] over the families of test_train_cabi_status_table; ``lib``: a
    loaded libgqhip with the ``signatures`` (pit_hip._lib._SIGNATURES) set."""
    fake, ample = 0x10000, 1 << 62          # the pointers are never dereferenced: see the test's docstring
    rows = []
    for entry, (names, base, size, perturbations) in _TRAIN_ENTRIES.items():
        names = names.split()
        argtypes = signatures[entry][1]
        assert len(names) == len(argtypes), entry
        ptrs = [n for n, t in zip(names, argtypes) if t is ctypes.c_void_p and n != "stream"]
        has_ws, fsq = "workspace" in ptrs, "levels_host" in names
        fn = getattr(lib, entry)

        def need_of(v):
            """the workspace the call of these scalars wants, by the entry point's own size function"""
            if not size:
                return 0
            K = v["c"] // v["dim"] if "c" in v and v["dim"] > 0 else v.get("nc", 1)
            shape = dict(v, rows=v["B"] * v["L"] * K)
            return getattr(lib, size[0])(*[shape[a] for a in size[1].split()])

        def case(cid, nulls=(), off=None, ws_bytes=ample, levels=(8, 8, 8, 5, 5, 5), nlev=None, **scalars):
            vals = dict(base, **{p: (None if p in nulls else fake + (off or {}).get(p, 0)) for p in ptrs}, stream=None)
            if "cb_cache" in vals:
                vals["cb_cache"] = None
            assert set(scalars) <= set(vals), scalars
            vals.update(scalars)
            if has_ws:
                vals["workspace_bytes"] = ws_bytes(need_of(vals)) if callable(ws_bytes) else ws_bytes
            if fsq:                         # read on the host: a real array (17 elements, so that every nlev asked for is backed)
                vals["levels_host"] = None if levels is None else (ctypes.c_int32 * 17)(*(list(levels) + [2] * (17 - len(levels))))
                vals["nlev"] = len(levels or ()) if nlev is None else nlev
            rows.append([entry, cid, fn(*[vals[n] for n in names])])

        def ident(p):
            return ",".join("%s=%r" % kv for kv in p.items())

        case("base")
        case("nothing/null", ptrs, None, 0, B=0)
        case("nothing/fake", B=0)
        case("all/null", ptrs)
        for p in ptrs:
            if p not in ("workspace", "cb_cache"):
                case("null:" + p, (p,))
        for layout in (0, 1):               # the masks 3 / 7 / 15, per layout (BSQ's "blc" rows move 16 bytes at a time)
            for p in ptrs:
                if p not in ("workspace", "cb_cache"):
                    for off in (2, 4, 8):
                        case("layout=%d/%s+%d" % (layout, p, off), (), {p: off}, layout=layout)
        if has_ws:
            case("ws/null", ("workspace",), None, lambda need: need)
            case("ws/short", (), None, lambda need: need - 1)
            case("ws/exact", (), None, lambda need: need)
            case("ws/+8", (), {"workspace": 8})
            case("ws/+8/short", (), {"workspace": 8}, lambda need: need - 1)
            case("ws/null/+pointer", ("workspace",), {ptrs[0]: 2}, lambda need: need)
            case("B=0/ws/null", ("workspace",), None, 0, B=0)
            case("L=0/ws/null", ("workspace",), None, 0, L=0)
        for B in (-1, 0, 1, (1 << 30) + 1):
            case("B=%d" % B, B=B)
        for L in (-1, 0, 1, (1 << 30) + 1):
            case("L=%d" % L, L=L)
        case("B=0/L=2^30+1", B=0, L=(1 << 30) + 1)      # refused, or nothing to do: the Gaussian and VQ steps bound the rows later
        case("B=2^30+1/L=0", B=(1 << 30) + 1, L=0)
        case("B*L=2^30", B=1 << 15, L=1 << 15)
        case("B*L=2^30-2^15", B=(1 << 15) - 1, L=1 << 15)
        case("B*L=2^30/ws/short", (), None, 0, B=1 << 15, L=1 << 15)
        for layout in (0, 1, 2, -1):
            case("layout=%d" % layout, layout=layout)
        if "grouping" in names:
            for grouping in (0, 1, 2, -1):
                case("grouping=%d" % grouping, grouping=grouping)
                case("layout=1/grouping=%d" % grouping, layout=1, grouping=grouping)
        if "dim" in names:
            for dim in (0, 1, 64, 65):
                case("dim=%d" % dim, dim=dim, c=2 * max(dim, 1))
            for c in (0, 12, 17):
                case("c=%d" % c, c=c)
        if "d" in names:
            for d in (0, 1, 16, 17):
                case("d=%d" % d, d=d, C=d * (1 if "nc" in names else 16), **({"nc": 1} if "nc" in names else {}))
        if "loss_divisor" in names:
            for v in (0.0, -1.0, _NAN):
                case("loss_divisor=%r" % v, loss_divisor=v)
            case("B=0/loss_divisor=0.0", B=0, loss_divisor=0.0)
        if fsq:
            case("levels/null", levels=None, nlev=6)
            for nlev in (0, 1, 16, 17):
                case("nlev=%d" % nlev, levels=[2] * 16, nlev=nlev)
            case("level=1", levels=[8, 1, 8])
            case("product=2^31-2^16", levels=[65536, 32767])
            case("product=2^31", levels=[65536, 32768])
            case("product=2^32", levels=[4] * 16)
            case("B=0/levels/null", levels=None, nlev=6, B=0)
        for p in perturbations:
            p = dict(p)
            nulls = tuple(k for k in ptrs if k in p and p.pop(k, 0) is None)
            case(ident(dict(p, **{k: None for k in nulls})), nulls, **p)
    for size_name, shapes in _TRAIN_SIZES.items():
        for args in shapes:
            rows.append([size_name, "x".join(map(str, args)), getattr(lib, size_name)(*args)])
    return rows


def test_train_cabi_status_table():
    """The nine train-step entry points of csrc/gqhip.hip and vq_quantize_z_f32 return the status, and the three train workspace
    size functions the byte count, that tests/golden/train_cabi_status.json records (recorded with this generator from the library
    as it was before the train steps' host checks, workspace rule and launch chain were brought together): nothing to do with all
    pointers NULL or set, each pointer NULL in turn (the optional ones too), each pointer off its alignment by 2, 4 and 8 bytes in
    either layout (the masks 3, 7 and 15), the workspace NULL / one byte short / exact / misaligned, and each shape, layout,
    grouping, width, codebook-size, divisor and level argument at and past its limits in turn.  Without a device an entry point that
    gets past its checks returns 3 ("kernel launch failed": no device) and launches nothing, so 0 / 1 / 2 / 3 tell "empty",
    "refused", "workspace" and "would launch" apart -- the ORDER of the checks included.
    SAFETY: the pointers passed are made up (all but FSQ's levels, which the host reads: a real array).  They are never
    dereferenced only because nothing can launch, so this test must never run where a HIP device is present: it skips there,
    whatever else is asked of it."""
    if torch.cuda.is_available():
        pytest.skip("passes made-up pointers: safe only where no kernel can launch")
    L = _lib()
    got = _train_cabi_table(L.lib(), L._SIGNATURES)
    want = json.load(open(os.path.join(G, "train_cabi_status.json")))
    assert len(got) == len(want) > 300 and {e for e, _, _ in got} == set(_TRAIN_ENTRIES) | set(_TRAIN_SIZES)
    assert len(_TRAIN_ENTRIES) == 10 and {s for e, _, s in got if e in _TRAIN_ENTRIES} == {0, 1, 2, 3}
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:20]
    # a few of the rules, spelled out: vq_backward_f32 alone calls a misaligned workspace an invalid argument, before it looks at its
    # size; "blc" BSQ rows want 16-byte pointers; an empty batch asks for no workspace
    assert ["vq_backward_f32", "ws/+8/short", 1] in got and ["lfq_train_f32", "ws/+8/short", 2] in got
    assert ["bsq_train_f32", "layout=1/x+8", 1] in got and ["bsq_train_f32", "layout=0/x+8", 3] in got
    assert ["lfq_train_f32", "B=0/ws/null", 0] in got and ["gq_gauss_train_f32", "L=0", 1] in got and ["fsq_train_f32", "L=0", 0] in got


def test_no_cpu_fallback():
    L = _lib()
    mu = torch.zeros(4, 16)
    with pytest.raises(L.GqHipError, match="no CPU fallback"):
        L.gq_argmax(mu, mu + 1, torch.zeros(64, 16))
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    q = GaussianQuantRegularizer("bchw", 64, group=16).eval()
    with pytest.raises(L.GqHipError):
        q(torch.zeros(1, 32, 2, 2))


def test_config_factory_remaps_pit_targets_and_resolves_interpolation():
    from pit_hip.models.autoencoder import AutoencodingEngine
    from pit_hip.util import instantiate_from_config, load_config

    cfg = load_config(os.path.join(G, "tiny_config.yaml"))
    assert cfg["model"]["params"]["decoder_config"]["params"]["ch_mult"] == [1, 2, 2]
    m = instantiate_from_config(cfg["model"])
    assert isinstance(m, AutoencodingEngine)
    keys = list(m.state_dict())
    assert keys[0] == "encoder.conv_in.weight" and any(k.startswith("decoder.up.0.block.0") for k in keys)
    assert not any(k.startswith("regularization") for k in keys)  # GQ buffers are non-persistent
    assert m.regularization.prior_samples.shape == (1024, 16)
    with pytest.raises(KeyError):
        instantiate_from_config({"params": {}})


def test_regularizer_buffers_match_reference_hashes():
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    q = GaussianQuantRegularizer("bchw", 65536, group=16, backend="cuda")
    want = META["cases"]["G1"]["16"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    assert sha(q.prior_samples.numpy()) == want["cb_sha"]
    assert sha(q.normal_log_prob.numpy()) == want["nlp_sha"]
    assert len(q.state_dict()) == 0 and q.group == 16 and q.n_samples == 65536
    assert float(q.prior_samples.abs().max()) == want["absmax"]
    assert not hasattr(q, "_absmax")   # nothing derived from the codebook is cached on the host


def _sd_sha(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy()).tobytes())
    return h.hexdigest()[:16]


SMALL = dict(attn_type="vanilla", double_z=True, z_channels=16, resolution=32, in_channels=3, out_ch=3, ch=32,
             ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[8], dropout=0.0)
FULL = dict(attn_type="vanilla", double_z=True, z_channels=16, resolution=256, in_channels=3, out_ch=3, ch=128,
            ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[32], dropout=0.0)


def test_encoder_decoder_small_match_reference_outputs():
    from pit_hip.modules.unet import Decoder, Encoder

    torch.manual_seed(1234)
    enc, dec = Encoder(**SMALL).eval(), Decoder(**SMALL).eval()
    want = META["cases"]["G7"]["small"]
    assert _sd_sha(enc.state_dict()) == want["enc_sd_sha"] and _sd_sha(dec.state_dict()) == want["dec_sd_sha"]
    d = np.load(os.path.join(G, "g7_small.npz"))
    with torch.no_grad():
        ze = enc(torch.from_numpy(d["x"]))
        xr = dec(torch.from_numpy(d["z_lat"]))
    # fp32 tolerance: only the fused silu differs from the reference's x*sigmoid(x)
    np.testing.assert_allclose(ze.numpy(), d["z_enc"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(xr.numpy(), d["x_rec"], atol=2e-5, rtol=1e-5)


def test_cpu_plumbing_config0_single_image_encode_indices_decode():
    """BASELINE.json configs[0]: one 256x256 image, CPU, no GPU: encoder (torch) ->
    oracle quantiser -> decoder, against the reference's end-to-end golden."""
    from pit_hip.modules.unet import Decoder, Encoder

    torch.manual_seed(1234)
    enc, dec = Encoder(**FULL).eval(), Decoder(**FULL).eval()
    want = META["cases"]["G7"]["full"]
    assert len(enc.state_dict()) == 116 and len(dec.state_dict()) == 158
    assert _sd_sha(enc.state_dict()) == want["enc_sd_sha"] and _sd_sha(dec.state_dict()) == want["dec_sd_sha"]
    d = np.load(os.path.join(G, "g7_full_e2e.npz"))
    gx = torch.Generator().manual_seed(1000)
    x = torch.rand(1, 3, 256, 256, generator=gx) * 2 - 1
    with torch.no_grad():
        ze = enc(x)
    np.testing.assert_allclose(ze.numpy(), d["z_enc"], atol=5e-5, rtol=1e-4)
    cb = O.codebook(65536, 16, 42)
    zhat, ind = O.gq1_forward(d["z_enc"], cb, 16)  # the golden z_enc -> bit-exact indices
    assert np.array_equal(ind, d["indices"])
    with torch.no_grad():
        xr = dec(torch.from_numpy(zhat))
    assert float(np.abs(xr.numpy() - d["x_rec"].astype(np.float32)).max()) < 5e-3  # fp16-stored golden
    st = d["x_rec_stats"]
    assert abs(float(xr.mean()) - st[0]) < 1e-4 and abs(float(xr.std()) - st[1]) < 1e-4


def test_train_mode_branch_matches_reference_goldens():
    """train() branch (reparameterised sample, KL-to-log2(N) loss, adaptive
    lambda state machine, incl. GQ2's no-op lam_max decrease) -- pure torch, bit-identical on CPU."""
    import hashlib

    from pit_hip.quantization.gaussian import GaussianQuantRegularizer, GaussianQuantRegularizer2

    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    z = torch.from_numpy(np.load(os.path.join(G, "g9_train_z.npz"))["z"])
    for tag, m in (("gq1", GaussianQuantRegularizer("bchw", 1024, group=16)),
                   ("gq2", GaussianQuantRegularizer2(4, 1024))):
        m.train()
        torch.manual_seed(123)
        for it, want in enumerate(META["cases"]["G9"][tag]):
            zh, info = m(z + 0.1 * it) if tag == "gq1" else m.quant_gaussian(z + 0.1 * it)
            got = {"kl_loss": float(info["kl_loss"]), "bits_mean": float(info["bits-mean"]),
                   "bits_min": float(info["bits-min"]), "bits_max": float(info["bits-max"]),
                   "lam": float(m.lam), "lam_min": float(m.lam_min), "lam_max": float(m.lam_max),
                   "zhat_sha": sha(zh.detach().numpy())}
            assert got == want, (tag, it)
    assert set(info) >= {"kl_loss", "bits-mean", "bits-min", "bits-max", "lam"}


def test_simple_dataset_transform_semantics(tmp_path):
    """Resize(shorter edge) -> CenterCrop -> ToTensor -> Normalize(0.5)."""
    from PIL import Image

    from pit_hip.data import SimpleDataset

    rng = np.random.default_rng(0)
    (tmp_path / "sub").mkdir()
    Image.fromarray(rng.integers(0, 256, (40, 64, 3), dtype=np.uint8)).save(tmp_path / "sub" / "b.png")
    Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(rng.integers(0, 256, (50, 30, 3), dtype=np.uint8)).save(tmp_path / "c.jpg")
    ds = SimpleDataset(str(tmp_path), 32)
    assert [os.path.basename(p) for p in ds.fpaths] == ["c.jpg", "a.png", "b.png"]  # jpg glob before png
    item = ds[1]
    assert item["img"].shape == (3, 32, 32) and item["img"].dtype == torch.float32
    raw = np.asarray(Image.open(tmp_path / "a.png").convert("RGB"), dtype=np.float32)
    assert torch.equal(item["img"], (torch.from_numpy(raw).permute(2, 0, 1) / 255 - 0.5) / 0.5)  # 32x32: identity
    wide = ds[2]["img"]  # 40x64 -> resize to 32x51 -> centre crop 32x32
    assert wide.shape == (3, 32, 32) and -1.0 <= float(wide.min()) and float(wide.max()) <= 1.0
    ref = Image.open(tmp_path / "sub" / "b.png").convert("RGB").resize((51, 32), Image.BILINEAR)
    left = int(round((51 - 32) / 2.0))
    ref = np.asarray(ref, dtype=np.float32)[:, left:left + 32]
    assert torch.equal(wide, (torch.from_numpy(ref).permute(2, 0, 1) / 255 - 0.5) / 0.5)
    lst = tmp_path / "list.txt"
    lst.write_text(str(tmp_path / "a.png") + "\n")
    assert len(SimpleDataset(str(lst), 32)) == 1


def test_unet_autograd_path_on_cpu():
    """Outside no_grad (training / fine-tuning) the conv stack stays on ATen ops and is differentiable."""
    from pit_hip.modules.unet import Decoder, Encoder

    torch.manual_seed(0)
    enc, dec = Encoder(**SMALL), Decoder(**SMALL)
    x = torch.rand(1, 3, 32, 32) * 2 - 1
    z = enc(x)
    rec = dec(z[:, :16])
    rec.mean().backward()
    assert enc.conv_in.weight.grad is not None and dec.conv_out.weight.grad is not None
    with torch.no_grad():
        torch.testing.assert_close(enc(x), z.detach(), atol=1e-6, rtol=1e-6)  # same function either way


def test_graft_entry_build_runs():
    """`__graft_entry__.build()` is the driver's "does it build" check: it must compile (incrementally) and import."""
    import __graft_entry__ as ge

    ge.build()


# ---------------------------------------------------------------------------------------------- round 2
def test_get_psnr_matches_reference_golden():
    """pit/evaluations/psnr.py:17-35 via golden g12 (captured from the imported reference)."""
    from pit_hip.eval_dist import get_psnr, psnr_zero_mean

    d = np.load(os.path.join(G, "g12_psnr.npz"))
    x, xr = torch.from_numpy(d["x"]), torch.from_numpy(d["x_rec"])
    assert np.array_equal(get_psnr(x, xr, zero_mean=True).numpy(), d["psnr_zero_mean"])
    assert np.array_equal(psnr_zero_mean(x, xr).numpy(), d["psnr_zero_mean"])
    assert np.array_equal(get_psnr((x + 1) / 2, (xr + 1) / 2).numpy(), d["psnr_unit"])
    assert torch.isinf(get_psnr(x[:1], x[:1], zero_mean=True)).all()   # identical images: +inf, like the reference


def test_cal_ent_known_answers():
    """eval.py:137-141: usage = share of non-empty bins, entropy = -sum p log2(p + 1e-5)."""
    from pit_hip.eval_dist import cal_ent

    n = 65536
    usage, ent = cal_ent(torch.ones(n))
    assert float(usage) == 1.0
    assert abs(float(ent) - (-np.log2(1.0 / n + 1e-5))) < 1e-3     # 15.27 bits, not 16: the reference's 1e-5 offset
    hist = torch.zeros(n)
    hist[:4] = torch.tensor([1.0, 1.0, 2.0, 4.0])
    usage, ent = cal_ent(hist)
    assert abs(float(usage) - 4 / n) < 1e-9
    p = np.array([1, 1, 2, 4]) / 8.0
    assert abs(float(ent) - float(-(p * np.log2(p + 1e-5)).sum())) < 1e-5
    assert cal_ent(hist.to(torch.int32))[1] == ent                  # integer histograms (the HIP kernel's) are accepted


def test_checkpoint_round_trip_with_loss_keys(tmp_path):
    """autoencoder.py:313-329 / eval.py:112-113: a Lightning-style checkpoint {"state_dict": ...} whose state_dict also
    carries `loss.*` (LPIPS / discriminator) keys loads with strict=False: encoder / decoder / VQ codebook restored,
    `loss.*` reported as unexpected, GQ buffers (non-persistent) neither saved nor expected."""
    from pit_hip.models.autoencoder import AutoencodingEngine

    unet = dict(attn_type="vanilla", double_z=True, z_channels=16, resolution=32, in_channels=3, out_ch=3, ch=32,
                ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16], dropout=0.0)
    mk = lambda seed, reg: (torch.manual_seed(seed), AutoencodingEngine(
        encoder_config={"target": "pit.modules.unet.Encoder", "params": unet},
        decoder_config={"target": "pit.modules.unet.Decoder", "params": unet}, regularizer_config=reg))[1]
    gq = {"target": "pit.quantization.gaussian.GaussianQuantRegularizer", "params": {"format": "bchw", "group": 16, "n_samples": 256}}
    src = mk(1, gq)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    assert not any(k.startswith("regularization") for k in sd)
    sd["loss.perceptual_loss.net.slice1.0.weight"] = torch.zeros(4, 3, 3, 3)
    sd["loss.discriminator.main.0.weight"] = torch.ones(8)
    path = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd, "global_step": 5000}, path)
    dst = mk(2, gq)
    assert not torch.equal(dst.encoder.conv_in.weight, src.encoder.conv_in.weight)
    missing, unexpected = dst.init_from_ckpt(str(path))
    assert missing == [] and sorted(unexpected) == sorted(k for k in sd if k.startswith("loss."))
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    # ckpt_path in the constructor (the YAML route) and ignore_keys
    via_ctor = (torch.manual_seed(3), AutoencodingEngine(
        encoder_config={"target": "pit.modules.unet.Encoder", "params": unet},
        decoder_config={"target": "pit.modules.unet.Decoder", "params": unet}, regularizer_config=gq, ckpt_path=str(path)))[1]
    assert torch.equal(via_ctor.decoder.conv_out.weight, src.decoder.conv_out.weight)
    part = mk(4, gq)
    missing, _ = part.init_from_ckpt(str(path), ignore_keys=("decoder.",))
    assert missing and all(k.startswith("decoder.") for k in missing)
    assert torch.equal(part.encoder.conv_in.weight, src.encoder.conv_in.weight)
    # VQ: the codebook IS a parameter (vq.py:33) and must come back from the checkpoint
    vq = {"target": "pit.quantization.vq.VQQuantizer", "params": {"format": "bchw", "n": 64, "dim": 16}}
    unet_v = dict(unet, double_z=False)
    mkv = lambda seed: (torch.manual_seed(seed), AutoencodingEngine(
        encoder_config={"target": "pit.modules.unet.Encoder", "params": unet_v},
        decoder_config={"target": "pit.modules.unet.Decoder", "params": unet_v}, regularizer_config=vq))[1]
    a, b = mkv(5), mkv(6)
    torch.save({"state_dict": a.state_dict()}, path)
    assert "regularization.embedding.weight" in a.state_dict()
    b.init_from_ckpt(str(path))
    assert torch.equal(b.regularization.embedding.weight, a.regularization.embedding.weight)


def test_step_record_validates_shape_and_range():
    from pit_hip.eval_dist import StepRecord

    lay = StepRecord(2, 3, n_metrics=1, check_range=True)
    idx = torch.tensor([[1, 2, 65535], [0, 7, 9]])
    rec = lay.pack(idx, torch.tensor([[1.5], [2.5]]))
    got, met = lay.unpack(rec)
    assert torch.equal(got, idx) and met.reshape(-1).tolist() == [1.5, 2.5]
    with pytest.raises(ValueError, match="65536"):
        lay.pack(torch.tensor([[1, 2, 65536], [0, 7, 9]]), torch.zeros(2, 1))
    with pytest.raises(ValueError, match="layout"):
        lay.pack(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 1))


def test_operand_order_weight_layouts_and_gemm_policy():
    """Host-side repacking for libgqhip's fp16 x 3 kernels (no GPU): wino_weights_operand_order / upconv_weights_f16 put element
    (k, n) where the kernels' MFMA B operands read it (lane (c, hh) of column tile nt holds k = 16 chunk + 8 hh .. + 7 of
    column 32 nt + c), and own_gemm_fits keeps the GEMMs whose grid would leave the chip mostly idle on the library."""
    import random

    from pit_hip import _lib

    rnd = random.Random(3)
    h, l = torch.randn(3, 64, 256).half(), torch.randn(3, 64, 256).half()
    wf = _lib.wino_weights_operand_order(h, l)
    assert tuple(wf.shape) == (3, 4, 8, 2, 64, 8) and wf.dtype == torch.float16 and wf.is_contiguous()
    for _ in range(500):
        t, kc, nt, pl, hh, c, e = (rnd.randrange(n) for n in (3, 4, 8, 2, 2, 32, 8))
        assert wf[t, kc, nt, pl, hh * 32 + c, e] == (h, l)[pl][t, kc * 16 + 8 * hh + e, nt * 32 + c]
    cin, cout = 32, 128
    m = torch.randn(2, 2, cin, 2, 2, cout)                    # [u, v, ci, a, b, co] as Upsample._phase_weights builds it
    uf, us = _lib.upconv_weights_f16(m.reshape(4 * cin, 4 * cout), cin, cout)
    assert tuple(uf.shape) == (4, 4 * (cin // 16), cout // 32, 2, 64, 8) and us > 0 and math.log2(us) == int(math.log2(us))
    hi = (m * us).half()
    lo = (m * us - hi.float()).half()
    for _ in range(500):
        ph, ch, tap, nt, pl, hh, c, e = (rnd.randrange(n) for n in (4, cin // 16, 4, cout // 32, 2, 2, 32, 8))
        assert uf[ph, ch * 4 + tap, nt, pl, hh * 32 + c, e] == (hi, lo)[pl][tap >> 1, tap & 1, ch * 16 + 8 * hh + e, ph >> 1, ph & 1, nt * 32 + c]
    with pytest.raises(_lib.GqHipError):
        _lib.upconv_weights_f16(m.reshape(4 * cin, 4 * cout), cin, 96)
    # the step's Winograd GEMM shapes (positions, tiles, Cout, Cin): only the 32 x 32 levels' 36 x 1024-tile GEMMs stay on the library
    assert _lib.own_gemm_fits(36, 16384, 256, 256) and _lib.own_gemm_fits(36, 4096, 512, 512) and _lib.own_gemm_fits(16, 4096, 512, 512)
    assert _lib.own_gemm_fits(16, 16384, 512, 256) and not _lib.own_gemm_fits(36, 1024, 512, 512) and not _lib.own_gemm_fits(16, 256, 512, 512)
    assert set(_lib.FILTER_KINDS) == {"auto", "fp32", "bf16", "mixed"}
    # every weight builder's bytes and u_scale, and the operand-scale rule, as recorded before the builders shared one weight
    # split and one scale helper
    got = _weight_layout_record(_lib)
    assert got == _WEIGHT_LAYOUT_RECORD, {k: v for k, v in got.items() if _WEIGHT_LAYOUT_RECORD.get(k) != v}


def _weight_layout_record(_lib):
    def sha(t):
        assert t.dtype == torch.float16 and t.is_contiguous()
        return hashlib.sha256(t.numpy().tobytes()).hexdigest()

    def randn(seed, *shape):
        return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))

    rec = {}
    builders = {"conv3_3x3": lambda w: _lib.conv3_weights_f16(w), "conv3_1x1": lambda w: _lib.conv3_weights_f16(w[:, :, :1, :1]),
                "conv3s2": lambda w: _lib.conv3s2_weights_f16(w),
                "upconv": lambda w: _lib.upconv_weights_f16(w[:, :, :2, :2].permute(2, 3, 1, 0).reshape(4 * 32, 128)[:, None, :]
                                                            .expand(4 * 32, 4, 128).reshape(4 * 32, 4 * 128), 32, 128)}
    weights = {"randn": randn(11, 128, 32, 3, 3) * 0.07, "zero": torch.zeros(128, 32, 3, 3),
               "pow2": (randn(12, 128, 32, 3, 3) * 0.1).clamp(-0.25, 0.25)}      # amax == 0; amax an exact power of two
    assert float(weights["pow2"].abs().max()) == 0.25 and float(weights["pow2"][:, :, :1, :1].abs().max()) == 0.25
    for wname, w in weights.items():
        for bname, build in builders.items():
            wf, us = build(w)
            rec["%s/%s" % (bname, wname)] = [sha(wf), us]
    h, l = randn(13, 3, 64, 256).half(), (randn(14, 3, 64, 256) * 2.0 ** -11).half()
    rec["wino_operand_order"] = [sha(_lib.wino_weights_operand_order(h, l)), None]
    for bound in (1e-40, 1.0, 3.0, 32768.0, 1e30):
        rec["attention_scales/%r" % bound] = list(_lib.attention_scales(bound, 2.0 * bound))
    return rec


# [SHA-256 of the operand's bytes, u_scale]; attention_scales: [sq, sv] at (bound, 2 bound)
_WEIGHT_LAYOUT_RECORD = {
    "conv3_3x3/randn": ["43918aca79dada65f4b0fad5c9b448606643f7d9cbd585e1750ec7ff8734b2e2", 32768.0],
    "conv3_1x1/randn": ["4d4241106379cfafb7a60102e90247025b98059f2f1b72ea05b5dbd7b0f49215", 32768.0],
    "conv3s2/randn": ["312f60907cf0a6d4cb00f4cb905e1e97cae89cea1efa94ee59211b98e51e4cce", 32768.0],
    "upconv/randn": ["acf470e8174fa39752d94fd7d1e20e2be1a86de8759e03d163a5f5e274d66521", 32768.0],
    "conv3_3x3/zero": ["8123c216413f82bbaa0339c27a43d9822c2a043e20662b27c97874429b996e9a", 1.0],
    "conv3_1x1/zero": ["4fe7b59af6de3b665b67788cc2f99892ab827efae3a467342b3bb4e3bc8e5bfe", 1.0],
    "conv3s2/zero": ["8123c216413f82bbaa0339c27a43d9822c2a043e20662b27c97874429b996e9a", 1.0],
    "upconv/zero": ["8a39d2abd3999ab73c34db2476849cddf303ce389b35826850f9a700589b4a90", 1.0],
    "conv3_3x3/pow2": ["74899470ec9cec3d194a990fc9932afce4408499fe258d928c3c9c14983065c8", 65536.0],
    "conv3_1x1/pow2": ["c0352f2791dd6edce7d4aa473649ff903a253ee501493cf0c067fafb6df69505", 65536.0],
    "conv3s2/pow2": ["0c6a657bf8560108fa541f3630176768b6f777298cf03dfa81b3658b2d14376f", 65536.0],
    "upconv/pow2": ["85a22307a6cda80317b634d70092d0c1a17bebc48d1548ec8b24bffd37cefd1b", 65536.0],
    "wino_operand_order": ["2a1cbc5d740863c3dcd6b573c8d660108842c3b9600386b908ea60acb3f98d53", None],
    "attention_scales/1e-40": [16384.0, 16384.0],
    "attention_scales/1.0": [16384.0, 16384.0],
    "attention_scales/3.0": [8192.0, 4096.0],
    "attention_scales/32768.0": [1.0, 0.5],
    "attention_scales/1e+30": [2.5849394142282115e-26, 1.2924697071141057e-26],
}


def test_fp16_fp8_filter_representation_error_is_inside_the_charged_bound():
    """The fp16 + fp8 filter's operand arithmetic restated in numpy (per-row power-of-two normalisation,
    fp16 h parts, e4m3 corrections (s_l 2^11) x (a_h 2^-6) and s_h x (a_l 2^6), exact accumulation) on operands built to
    maximise the rounding errors -- every value just above a power of two plus the largest fp16 residual, residuals with the
    largest e4m3 error, aligned signs, coefficients spread over 30 binades, codebooks at both ends of the allowed range: the
    error of the filter value stays well inside the representation share (2450 - 256 accumulation steps) of the coefficient
    the re-rank charges (csrc/gqhip.hip: kMixedEfCoeff)."""
    rng = np.random.default_rng(1)
    u, dim, n = 2.0 ** -24, 16, 2048

    def e4m3(x):          # RNE to OCP e4m3: 3 mantissa bits, min normal 2^-6, subnormal step 2^-9, max 448
        x = np.asarray(x, dtype=np.float64)
        a = np.abs(x)
        e = np.maximum(np.floor(np.log2(np.maximum(a, 1e-300))), -6)
        step = 2.0 ** (e - 3)
        return np.sign(x) * np.minimum(np.round(a / step) * step, 448.0)

    def f16(x):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)

    def worst_error(A, B, cb):
        coef = np.concatenate([A, B], 1).astype(np.float32).astype(np.float64)
        c32 = cb.astype(np.float32)
        feat = np.concatenate([(c32 * c32).astype(np.float64), c32.astype(np.float64)], 1)
        sc = 2.0 ** (14 - (np.floor(np.log2(np.abs(coef).max(1))) + 1))      # largest coefficient into [2^13, 2^14)
        ch = coef * sc[:, None]
        chh, sh = f16(ch), f16(feat)
        chl, sl = ch - chh, feat - sh
        ft = (chh @ sh.T + (e4m3(chh / 64) @ e4m3(sl * 2048).T) * (64 / 2048) + (e4m3(chl * 64) @ e4m3(feat).T) / 64) / sc[:, None]
        N1 = np.abs(cb).max()
        assert 1.0 <= N1 <= 16.0
        T = (np.abs(coef[:, :dim]) * N1 * N1 + np.abs(coef[:, dim:]) * N1).sum(1)
        return float((np.abs(ft - coef @ feat.T).max(1) / (u * T)).max())

    def worst(shape, lo, hi):
        k = rng.integers(lo, hi, shape)
        return 2.0 ** k * (1 + 2.0 ** -11 * (1 + 2.0 ** -4 * rng.choice([1.0, 0.9375, 0.5], shape))) * rng.choice([-1, 1], shape)

    cbw = np.abs(np.clip(worst((n, dim), -1, 2), -16, 16))
    Aw, Bw = -np.abs(worst((256, dim), -2, 6)), np.abs(worst((256, dim), -2, 6))
    cases = {
        "aligned signs": (Aw, Bw, cbw),
        "mixed signs": (Aw, worst((256, dim), -2, 6), cbw * rng.choice([-1, 1], cbw.shape)),
        "30 binades in a row": (-np.abs(worst((256, dim), -20, 10)), np.abs(worst((256, dim), -20, 10)), cbw),
        "codebook up to 16": (Aw, Bw, np.clip(cbw * 4, 1, 16)),
        "codebook max 1": (Aw, Bw, cbw / cbw.max()),
    }
    for name, (A, B, cb) in cases.items():
        err = worst_error(A, B, cb)
        print(f"fp16 + fp8 representation error, {name}: {err:.0f} u T")
        assert err < 2450 - 256, (name, err)


def test_gq_cuda_package_has_the_reference_layout():
    """gq_cuda_extension/gq_cuda/__init__.py:3 does `from . import _C, ops`: both names import here too, and the op is registered
    with the reference's schema (csrc/gq_cuda.cpp:29-31)."""
    import importlib

    import torch

    gq_cuda = importlib.import_module("gq_cuda")
    assert importlib.import_module("gq_cuda._C") is gq_cuda._C and gq_cuda.ops is importlib.import_module("gq_cuda.ops")
    schema = str(torch.ops.extension_cpp.gq.default._schema)
    assert "Tensor a, Tensor b, Tensor c, Tensor(a!) out, int d, int e, int f, float g" in schema
