"""-m gpu, marker convstack: the store phase of the five MFMA kernel families -- conv3x3_gn, conv1x1, conv3x3s2 and upconv2x
through the LDS-staged epilogue (csrc/gq_epilogue.h), the Winograd GEMMs' M store -- with and without bias, residual and
statistics, at 128 / 256 / 512 output channels where the family has them: every output element against fp64
(tests/convstack_ref.py models, the gates of test_gpu_convstack_kernels.py), the statistics records against fp64 sums of the
stored output, the stride-2 output mapping and the four upconv phases one by one, and two calls bit-equal."""
import pytest
import torch
import torch.nn.functional as F

import convstack_ref as R
from gpu_common import DEV

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _stats_match(y, st, groups):
    """the record of every (image, group) holds the fp64 sum and sum of squares of the stored y"""
    B, C = y.shape[:2]
    yd = y.double().permute(0, 2, 3, 1).reshape(B, -1, groups, C // groups)
    ref = torch.stack([yd.sum((1, 3)), (yd ** 2).sum((1, 3))], -1).flatten()
    mag = torch.stack([yd.abs().sum((1, 3)), (yd ** 2).sum((1, 3))], -1).flatten()
    from pit_hip import _lib
    got = _lib.gn_stats_values(st)
    assert torch.isfinite(got).all()
    err = float(((got - ref).abs() / (mag + 1e-30)).max())
    assert err <= 1e-10, err   # exact fixed-point sums of fp64 partial moments


def _twice(fn):
    """two calls of the same launch: outputs (and statistics records) bit-equal"""
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    return a if len(a) > 1 else a[0]


@pytest.mark.parametrize("cout", [128, 256])
def test_conv3x3_gn_epilogue(cout):
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    torch.manual_seed(100 + cout)
    cin, B, H, W = 128, 2, 16, 64
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).to(DEV).to(memory_format=torch.channels_last)
    norm = torch.nn.GroupNorm(32, cin, eps=1e-6).to(DEV)
    with torch.no_grad():
        norm.weight.normal_(); norm.bias.normal_()
        x = _cl(2 * torch.randn(B, cin, H, W, device=DEV) + 0.5)
        res = _cl(torch.randn(B, cout, H, W, device=DEV))
        wf, us = _lib.conv3_weights_f16(conv.weight)
        stats = _lib.gn_stats(x, 32)
        gn = (norm.weight, norm.bias, 32, 1e-6, True, stats, None)
        bound = U._gn_act_bound(norm, x)
        xn = _lib.gn_apply(x, norm.weight, norm.bias, 32, 1e-6, True, stats).double()
        for bias in (None, conv.bias):
            for r in (None, res):
                for groups in (0, 32):
                    ref, mag = R.conv_ref_and_mag(xn, conv.weight.double(), None if bias is None else bias.double(), 1, 1,
                                                  None if r is None else r.double())
                    out = _twice(lambda: _lib.conv3x3_direct(x, wf, us, bound, gn=gn, residual=r, bias=bias, stats_groups=groups))
                    y = out[0] if groups else out
                    tag = f"conv3x3_gn {cin}->{cout} bias {bias is not None} res {r is not None} stats {groups}"
                    R.lin_gate(y, ref, mag, 6e-7, tag)   # the gate of test_direct_conv3x3_matches_fp64_convolution
                    if groups:
                        _stats_match(y, out[1], groups)


@pytest.mark.parametrize("cout", [128, 256, 512])
def test_conv1x1_epilogue(cout):
    from pit_hip import _lib

    torch.manual_seed(200 + cout)
    cin, B, H, W = 256, 2, 16, 32
    conv = torch.nn.Conv2d(cin, cout, 1).to(DEV).to(memory_format=torch.channels_last)
    with torch.no_grad():
        x = _cl(3 * torch.randn(B, cin, H, W, device=DEV))
        res = _cl(torch.randn(B, cout, H, W, device=DEV))
        wf, us = _lib.conv3_weights_f16(conv.weight)
        bound = float(x.abs().max())
        for bias in (None, conv.bias):
            for r in (None, res):
                for groups in (0, 32):
                    ref, mag = R.conv_ref_and_mag(x.double(), conv.weight.double(), None if bias is None else bias.double(), 1, 0,
                                                  None if r is None else r.double())
                    out = _twice(lambda: _lib.conv1x1_direct(x, wf, us, bound, residual=r, bias=bias, stats_groups=groups))
                    y = out[0] if groups else out
                    R.lin_gate(y, ref, mag, 1.2e-6, f"conv1x1 {cin}->{cout} bias {bias is not None} res {r is not None} stats {groups}")
                    if groups:
                        _stats_match(y, out[1], groups)


@pytest.mark.parametrize("cout", [128, 256, 512])
def test_conv3x3s2_epilogue_and_output_mapping(cout):
    from pit_hip import _lib

    torch.manual_seed(300 + cout)
    cin, B, H, W = 128, 2, 32, 128
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 0).to(DEV).to(memory_format=torch.channels_last)
    with torch.no_grad():
        # a ramp over rows and columns: a stride-2 output written to the wrong pixel cannot pass the fp64 comparison
        ramp = (torch.arange(H, device=DEV)[:, None] * 0.37 + torch.arange(W, device=DEV)[None, :] * 0.11).sin()
        x = _cl(3 * torch.randn(B, cin, H, W, device=DEV) + 2 * ramp)
        wf, us = _lib.conv3s2_weights_f16(conv.weight)
        xp = F.pad(x.double(), (0, 1, 0, 1))
        for bias in (None, conv.bias):
            for groups in (0, 32):
                ref, mag = R.conv_ref_and_mag(xp, conv.weight.double(), None if bias is None else bias.double(), 2, 0)
                out = _twice(lambda: _lib.conv3x3s2_direct(x, wf, us, float(x.abs().max()), bias=bias, stats_groups=groups))
                y = out[0] if groups else out
                assert tuple(y.shape) == (B, cout, H // 2, W // 2)
                R.lin_gate(y, ref, mag, 8e-7, f"conv3x3s2 {cin}->{cout} bias {bias is not None} stats {groups}")
                if groups:
                    _stats_match(y, out[1], groups)


@pytest.mark.parametrize("cout", [128, 256, 512])
def test_upconv2x_epilogue_each_phase(cout):
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    torch.manual_seed(400 + cout)
    cin, B, H, W = cout, 2, 16, 32
    up = U.Upsample(cin).to(DEV).eval()
    with torch.no_grad():
        x = _cl(3.0 * torch.randn(B, cin, H, W, device=DEV))
        wf, us = _lib.upconv_weights_f16(up._phase_weights(), cin, cout)
        xu = F.interpolate(x.double(), scale_factor=2.0, mode="nearest")
        for bias in (None, up.conv.bias):
            for groups in (0, 32):
                ref, mag = R.conv_ref_and_mag(xu, up.conv.weight.double(), None if bias is None else bias.double(), 1, 1)
                out = _twice(lambda: _lib.upconv2x_direct(x, wf, us, float(x.abs().max()), bias=bias, stats_groups=groups))
                y = out[0] if groups else out
                assert tuple(y.shape) == (B, cout, 2 * H, 2 * W)
                scale = float(ref.abs().mean())
                for a in (0, 1):
                    for b in (0, 1):
                        e = float((y[:, :, a::2, b::2].double() - ref[:, :, a::2, b::2]).abs().max()) / scale
                        assert e <= 1.2e-5, (cout, a, b, e)      # the gate of test_upconv2x_direct_matches_fp64
                if groups:
                    _stats_match(y, out[1], groups)


@pytest.mark.parametrize("cin,cout", [(32, 128), (256, 256), (256, 384), (512, 512)])
def test_wino_gemm_m_store(cin, cout):
    """M of both GEMM kernels (256 x 128 tiles: cout 128, 384 or cin 32; 256 x 256 tiles otherwise) against fp64 of the same
    split operands, every row of several row tiles and positions"""
    from pit_hip import _lib

    torch.manual_seed(500 + cin + cout)
    L = _lib.lib()
    P, tiles = 2, 768
    V = torch.randn(P, tiles, cin, device=DEV) * 40.0
    Uw = torch.randn(P, cin, cout, device=DEV) * 3.0
    vh = V.half(); vl = (V - vh.float()).half()
    uh = Uw.half(); ul = (Uw - uh.float()).half()
    V2 = torch.cat([vh, vl], 2).contiguous()
    Wf = _lib.wino_weights_operand_order(uh, ul)

    def run():
        M = torch.full((P, tiles, cout), float("nan"), device=DEV)
        _lib._check(L.wino_gemm_f16x2(V2.data_ptr(), Wf.data_ptr(), M.data_ptr(), P, tiles, cin, cout,
                                      torch.cuda.current_stream().cuda_stream), "wino_gemm_f16x2")
        return M

    M = _twice(run)
    r64 = torch.bmm(vh.double(), uh.double()) + torch.bmm(vh.double(), ul.double()) + torch.bmm(vl.double(), uh.double())
    sc = torch.bmm(V.abs().double(), Uw.abs().double())
    assert torch.isfinite(M).all()
    e = float(((M.double() - r64).abs() / sc).max())
    assert e <= 3e-7, e
