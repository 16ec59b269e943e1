"""-m gpu, marker convstack: the direct 3x3 convolution's chunk loop (csrc/gq_conv3.h: run_chunk) at the shapes where a peeled last
chunk and a branch-free convert() can go wrong: the fewest chunks the entry point admits, one-tile images whose whole halo lies
outside the image, tiles whose sixth piece has lanes past the patch (all of them: 340 pixels x 4 quads over 256 threads), two
images with different statistics, both output widths, with and without the fused epilogue."""
import pytest
import torch

from gpu_common import DEV

pytestmark = pytest.mark.gpu

SIZES = ((8, 32), (16, 64), (24, 32))   # one tile (every halo pixel outside the image); 2 x 2 tiles; 3 x 1 tiles


def _case(cin, groups, cout, H, W, seed):
    """x (two images of different mean and spread), GroupNorm, conv, residual and the fp64 references, computed once per shape."""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    assert _lib.gn_nhwc_ok(cin, groups)
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).to(DEV).to(memory_format=torch.channels_last)
    norm = torch.nn.GroupNorm(groups, cin, eps=1e-6).to(DEV)
    with torch.no_grad():
        norm.weight.normal_(); norm.bias.normal_()
        x = torch.randn(2, cin, H, W, device=DEV)
        x[0] = 0.5 * x[0] - 1.0          # per-image statistics differ: a block that read the other image's records shows
        x[1] = 3.0 * x[1] + 2.0
        x = x.contiguous(memory_format=torch.channels_last)
        res = torch.randn(2, cout, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
        wf, us = _lib.conv3_weights_f16(conv.weight)
        stats = _lib.gn_stats(x, groups)
        gn = (norm.weight, norm.bias, groups, 1e-6, True, stats, None)
        bound = U._gn_act_bound(norm, x)
        xn = _lib.gn_apply(x, norm.weight, norm.bias, groups, 1e-6, True, stats).double()
        sc = torch.nn.functional.conv2d(xn.abs(), conv.weight.double().abs(), None, 1, 1)
        ref0 = torch.nn.functional.conv2d(xn, conv.weight.double(), None, 1, 1)
    return conv, x, res, wf, us, gn, bound, sc, ref0


@pytest.mark.convstack
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin,groups", [(32, 8), (64, 16)])   # nch = 2: one looped chunk + the peeled one; nch = 4: both buffers twice
def test_direct_conv3x3_few_chunks_small_images_match_fp64(cin, groups, cout):
    """conv3x3_direct against torch's fp64 convolution of gn_apply's output under test_direct_conv3x3_matches_fp64_convolution's
    bound: error <= 6e-7 of sum |x||w|; statistics rtol 2e-6 / atol 1e-3."""
    from pit_hip import _lib

    for i, (H, W) in enumerate(SIZES):
        conv, x, res, wf, us, gn, bound, sc, ref0 = _case(cin, groups, cout, H, W, 100 * cin + cout + i)
        with torch.no_grad():
            y, st = _lib.conv3x3_direct(x, wf, us, bound, gn=gn, residual=res, bias=conv.bias, stats_groups=32)
            ref = ref0 + conv.bias.double()[None, :, None, None] + res.double()
            err = float(((y.double() - ref).abs() / sc).max())
            print(f"Cin {cin} Cout {cout} {H}x{W}: fused epilogue err {err:.2e}")
            assert err <= 6e-7, (H, W, err)
            yd = y.double().permute(0, 2, 3, 1).reshape(2, H * W, 32, cout // 32)
            st_y = torch.stack([yd.sum((1, 3)), (yd ** 2).sum((1, 3))], -1).flatten()
            got = _lib.gn_stats_values(st)
            assert torch.allclose(got, st_y, rtol=2e-6, atol=1e-3), (H, W, float((got - st_y).abs().max()))
            y2 = _lib.conv3x3_direct(x, wf, us, bound, gn=gn)
            err2 = float(((y2.double() - ref0).abs() / sc).max())
            print(f"Cin {cin} Cout {cout} {H}x{W}: bare err {err2:.2e}")
            assert err2 <= 6e-7, (H, W, err2)


@pytest.mark.convstack
@pytest.mark.parametrize("cin", [16, 48])
def test_direct_conv3x3_admits_no_odd_chunk_count(cin):
    """Cin = 16 (the peeled chunk alone) and Cin = 48 (three chunks) cannot reach the kernel: the entry point takes multiples of
    32 input channels only, so the loop always runs an even number of chunks >= 2 -- and says so, rather than running."""
    from pit_hip import _lib

    conv = torch.nn.Conv2d(cin, 128, 3, 1, 1).to(DEV)
    wf, us = _lib.conv3_weights_f16(conv.weight)
    x = torch.randn(2, cin, 8, 32, device=DEV).contiguous(memory_format=torch.channels_last)
    y = torch.empty(2, 128, 8, 32, device=DEV).contiguous(memory_format=torch.channels_last)
    g = torch.ones(cin, device=DEV)
    rec = torch.zeros(2 * 4 * _lib.GNSTAT_WORDS, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.GqHipError):
        _lib.conv3x3_direct(x, wf, us, 10.0, (g, g, 4, 1e-6, True, rec, None))
    rc = _lib.lib().conv3x3_gn_f16x3(x.data_ptr(), g.data_ptr(), g.data_ptr(), None, rec.data_ptr(), 4, 1e-6, 1, 1.0, wf.data_ptr(), None,
                                     None, y.data_ptr(), None, 2, 8, 32, cin, 128, 32, 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc != 0


def _stats_of(y, cout):
    B, _, H, W = y.shape
    yd = y.double().permute(0, 2, 3, 1).reshape(B, H * W, 32, cout // 32)
    return torch.stack([yd.sum((1, 3)), (yd ** 2).sum((1, 3))], -1).flatten()


@pytest.mark.convstack
@pytest.mark.parametrize("cin", [16, 32])   # nch = 1: only the peeled chunk; nch = 2: one looped chunk + the peeled one
def test_upconv2x_direct_one_and_two_chunks_match_fp64(cin):
    """upconv2x_direct on its smallest tile (8 x 32 low-resolution pixels, every halo pixel outside the image) against the fp64
    convolution of the upsampled tensor, under test_upconv2x_direct_matches_fp64's bound: error <= 1.2e-5 of mean |y|."""
    import torch.nn.functional as F
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    torch.manual_seed(310 + cin)
    up = U.Upsample(128).to(DEV).eval()
    up.conv = torch.nn.Conv2d(cin, 128, 3, 1, 1).to(DEV)
    with torch.no_grad():
        x = (3.0 * torch.randn(2, cin, 8, 32, device=DEV)).contiguous(memory_format=torch.channels_last)
        wf, us = _lib.upconv_weights_f16(up._phase_weights(), cin, 128)
        ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), up.conv.weight.double(), up.conv.bias.double(), 1, 1)
        y, st = _lib.upconv2x_direct(x, wf, us, float(x.abs().max()), bias=up.conv.bias, stats_groups=32)
    assert tuple(y.shape) == (2, 128, 16, 64)
    err = float((y.double() - ref).abs().max()) / float(ref.abs().mean())
    print(f"upconv Cin {cin}: err {err:.2e} of mean |y|")
    assert err <= 1.2e-5, err
    assert torch.allclose(_lib.gn_stats_values(st), _stats_of(y, 128), rtol=1e-6, atol=1e-3)


@pytest.mark.convstack
@pytest.mark.parametrize("H,W", [(8, 16), (16, 16)])          # one and two 128-pixel tiles per image (the tiling small grids get)
@pytest.mark.parametrize("cin,groups", [(32, 8), (64, 16)])   # one stage: only the peeled one; two: one looped + the peeled
def test_conv1x1_one_and_two_stages_match_fp64(cin, groups, H, W):
    """conv1x1_direct, plain (with a pending bias) and with the GroupNorm fused in, under test_conv1x1_f16x3_matches_fp64's bound:
    error <= 1.2e-6 of sum |x||w|; statistics rtol 2e-6 / atol 1e-2."""
    from pit_hip import _lib

    assert _lib.gn_nhwc_ok(cin, groups)
    torch.manual_seed(410 + cin + H)
    conv = torch.nn.Conv2d(cin, 128, 1).to(DEV)
    with torch.no_grad():
        x = torch.randn(2, cin, H, W, device=DEV)
        x[0] = 0.5 * x[0] - 1.0
        x[1] = 3.0 * x[1] + 2.0
        x = x.contiguous(memory_format=torch.channels_last)
        res = torch.randn(2, 128, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
        pb = torch.randn(cin, device=DEV)
        gamma, beta = torch.randn(cin, device=DEV), torch.randn(cin, device=DEV)
        wf, us = _lib.conv3_weights_f16(conv.weight)
        w64 = conv.weight.double()
        # plain: x + pending bias, host bound; bias + residual + statistics
        xin = x.double() + pb.double()[None, :, None, None]
        ref = torch.nn.functional.conv2d(xin, w64, conv.bias.double()) + res.double()
        sc = torch.nn.functional.conv2d(xin.abs(), w64.abs())
        y, st = _lib.conv1x1_direct(x, wf, us, float(xin.abs().max()), residual=res, bias=conv.bias, stats_groups=32, pre_bias=pb)
        err = float(((y.double() - ref).abs() / sc).max())
        print(f"1x1 Cin {cin} {H}x{W}: plain err {err:.2e}")
        assert err <= 1.2e-6, err
        assert torch.allclose(_lib.gn_stats_values(st), _stats_of(y, 128), rtol=2e-6, atol=1e-2)
        # GroupNorm (no SiLU) fused in
        stats = _lib.gn_stats(x, groups)
        xn = _lib.gn_apply(x, gamma, beta, groups, 1e-6, False, stats).double()
        ref = torch.nn.functional.conv2d(xn, w64)
        sc = torch.nn.functional.conv2d(xn.abs(), w64.abs())
        y = _lib.conv1x1_direct(x, wf, us, float(xn.abs().max()), gn=(gamma, beta, groups, 1e-6, False, stats, None))
        err = float(((y.double() - ref).abs() / sc).max())
        print(f"1x1 Cin {cin} {H}x{W}: GroupNorm err {err:.2e}")
        assert err <= 1.2e-6, err
