"""-m gpu, marker convstack: the tilings of libgqhip's own Winograd GEMM (csrc/gq_wino_gemm.h: 256 x 128 blocks, 256 x 256 blocks
of 8 waves, 128 x 256 blocks of 4 waves), forced one by one through GQHIP_WGEMM in ONE process (the knob is read per call):
every tiling and the default dispatch give the same M bit for bit (all accumulate k ascending, h U_h, h U_l, l U_h per k-step),
none writes outside its M, and each stays inside the fp64 gate of test_gpu_convstack_kernels.py."""
import functools

import pytest
import torch

from gpu_common import DEV

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]

TILINGS = ("128", "w8", "w4")          # GQHIP_WGEMM values; None = the default dispatch
SENTINEL = 12345.0

# (P, tiles, Cin, Cout):
#   Cin = 64 is a single 64-k stage (no prefetch branch, the last-k-step clamp of the weight loads), 128 uses both buffers,
#   192 is an odd stage count (buffer parity); Cout = 512 is two column blocks (Wf and M column offsets); P = 3 with 256 tiles
#   is six 128-row tiles over 8 XCD slots (the early-return path); 512 tiles reach the second to fourth 128-row tile of a position.
CASES = ((3, 256, 64, 256), (2, 512, 128, 512), (1, 256, 192, 256), (2, 256, 512, 512))


@functools.lru_cache(maxsize=None)
def _operands(case):
    """seeded operands of a case, built once and never modified: (V, U, vh, vl, uh, ul, V2, Wf)"""
    from pit_hip import _lib

    P, tiles, cin, cout = case
    g = torch.Generator().manual_seed(1000 * cin + cout + tiles + P)
    V = (torch.randn(P, tiles, cin, generator=g) * 40.0).to(DEV)
    U = (torch.randn(P, cin, cout, generator=g) * 3.0).to(DEV)
    vh = V.half(); vl = (V - vh.float()).half()
    uh = U.half(); ul = (U - uh.float()).half()
    V2 = torch.cat([vh, vl], 2).contiguous()
    Wf = _lib.wino_weights_operand_order(uh, ul)
    return V, U, vh, vl, uh, ul, V2, Wf


def _run(case, knob, monkeypatch):
    """M of one tiling, in a NaN-filled buffer between two guard positions holding a sentinel; checks guards and finiteness"""
    from pit_hip import _lib

    P, tiles, cin, cout = case
    V2, Wf = _operands(case)[6:]
    if knob is None:
        monkeypatch.delenv("GQHIP_WGEMM", raising=False)
    else:
        monkeypatch.setenv("GQHIP_WGEMM", knob)
    buf = torch.full((P + 2, tiles, cout), float("nan"), device=DEV)
    buf[0] = SENTINEL
    buf[P + 1] = SENTINEL
    M = buf[1:P + 1]
    assert M.is_contiguous()
    _lib._check(_lib.lib().wino_gemm_f16x2(V2.data_ptr(), Wf.data_ptr(), M.data_ptr(), P, tiles, cin, cout,
                                           torch.cuda.current_stream().cuda_stream), "wino_gemm_f16x2")
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[P + 1] == SENTINEL).all()), (case, knob, "guard rows overwritten")
    assert bool(torch.isfinite(M).all()), (case, knob, "M not written everywhere")
    return M.clone()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_tilings_bit_equal_and_no_stray_writes(case, monkeypatch):
    want = _run(case, TILINGS[0], monkeypatch)
    for knob in TILINGS[1:] + (None,):
        got = _run(case, knob, monkeypatch)
        assert torch.equal(got, want), (case, knob, float((got - want).abs().max()))


def test_tilings_match_fp64_of_the_split_operands(monkeypatch):
    case = (2, 256, 512, 512)
    V, U, vh, vl, uh, ul = _operands(case)[:6]
    r64 = torch.bmm(vh.double(), uh.double()) + torch.bmm(vh.double(), ul.double()) + torch.bmm(vl.double(), uh.double())
    sc = torch.bmm(V.abs().double(), U.abs().double())
    for knob in TILINGS + (None,):
        M = _run(case, knob, monkeypatch)
        e = float(((M.double() - r64).abs() / sc).max())
        print(f"wino_gemm_f16x2 GQHIP_WGEMM={knob} {case}: err {e:.2e} of sum|a||b|")
        assert e <= 3e-7, (knob, e)   # the gate of test_wino_gemm_f16x2_wider_levels_match_fp64_and_the_library_route
