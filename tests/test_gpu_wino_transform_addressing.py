"""-m gpu, marker convstack: where the Winograd transform kernels read and write.  The kernels form their addresses from a base
and per-item row / column / plane offsets (csrc/gq_unet_aux.h: "Addressing of the transform kernels"); an index that went wrong
would read or write another pixel, tile, plane or image.  Inputs are small integers (|x| <= 8) and every transform coefficient is an
integer <= 8, so all fp32 arithmetic is exact and the result is compared with torch.equal against a plain torch evaluation of
B^T d B / A^T M A.  With the power-of-two scale 1 the fp16 split of an integer below 2048 is h = v, l = 0.

Shapes: B = 3 (image bases), H != W (row / column strides), 8 x 12 (every tile touches a border), 16 x 20 (interior tiles), and a C
on each side of the host's channels-per-thread branch: wino_out_res at F(4x4,3x3) runs two channels per thread unless C = 1024
(gqhip_unet.hip: 256 % (C / 2)); the input transforms have no branch on C (C = 8: a block spans many tiles, 128: the step's).

Every case runs twice: with the kernels the host picks at these sizes (32-bit offsets, "u32") and with GQHIP_WINO_WIDE=1, which
sends the same calls to the *_wide_kernel twins (64-bit offsets) that otherwise only tensors beyond 4 GiB reach."""
import pytest
import torch

from gpu_common import DEV

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]

BT = {2: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64),
      4: torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                       [0, 4, 0, -5, 0, 1]], dtype=torch.float64)}
AT = {2: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
      4: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)}
SHAPES = ((8, 12), (16, 20))
B = 3


@pytest.fixture(params=(False, True), ids=("u32", "wide"))
def offsets(request, monkeypatch):
    """the library reads GQHIP_WINO_WIDE on every call"""
    if request.param:
        monkeypatch.setenv("GQHIP_WINO_WIDE", "1")
    else:
        monkeypatch.delenv("GQHIP_WINO_WIDE", raising=False)
    return request.param


def ints(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).float()


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def ref_input_transform(x, t):
    """V [N * N, tiles, C] fp64 = B^T d B of every (t + 2)^2 input tile d of the zero-padded x [B, C, H, W], tiles in (b, th, tw) order"""
    n = t + 2
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    d = xp.unfold(2, n, t).unfold(3, n, t)                       # [B, C, H/t, W/t, n, n]
    bt = BT[t].to(x.device)
    v = bt @ d @ bt.T
    return v.permute(4, 5, 0, 2, 3, 1).reshape(n * n, -1, x.shape[1])


def ref_output_transform(M, t, H, W):
    """y [B, C, H, W] fp64 = A^T m A of every tile of M [N * N, tiles, C]"""
    n, C = t + 2, M.shape[2]
    m = M.double().reshape(n, n, B, H // t, W // t, C).permute(2, 5, 3, 4, 0, 1)      # [B, C, th, tw, n, n]
    at = AT[t].to(M.device)
    y = at @ m @ at.T                                                           # [B, C, th, tw, t, t]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)


@pytest.mark.parametrize("t", (2, 4))
@pytest.mark.parametrize("C", (8, 128))
def test_input_transforms_read_and_write_the_right_elements(t, C, offsets):
    """wino_in / wino4_in at fp32, f16x2 ([h | l]) and f16x3 ([h | h | l]) operands"""
    from pit_hip import _lib

    L = _lib.lib()
    for H, W in SHAPES:
        x = ints(B, C, H, W, seed=100 * t + H)
        ref = ref_input_transform(x, t).to(DEV)
        assert float(ref.abs().max()) < 2048
        xd, tiles, taps = nhwc(x), B * (H // t) * (W // t), (t + 2) ** 2
        for planes in (0, 2, 3):
            V = torch.full((taps, tiles, (planes or 1) * C), 7.0, dtype=torch.float16 if planes else torch.float32, device=DEV)
            _lib._wino_in(L, xd, V, None, t, planes, 1.0)
            parts = V.double().reshape(taps, tiles, planes or 1, C)
            want = {0: (ref,), 2: (ref, 0 * ref), 3: (ref, ref, 0 * ref)}[planes]
            for p, w in enumerate(want):
                assert torch.equal(parts[:, :, p], w), (t, C, H, W, planes, p)


@pytest.mark.parametrize("t", (2, 4))
def test_fused_input_transforms_write_what_gn_apply_and_the_plain_transform_write(t, offsets):
    """The GroupNorm-fused input transforms at the fp16 operands the step runs (f16x2, f16x3), B = 3, borders and interior: the
    bits of gn_apply followed by the plain transform (the fp32 operand is tied the same way in test_gpu_convstack_kernels.py)."""
    from pit_hip import _lib

    L, C, eps = _lib.lib(), 128, 1e-6
    torch.manual_seed(20)
    gamma, beta = torch.randn(C).to(DEV), torch.randn(C).to(DEV)
    for H, W in SHAPES:
        x = nhwc(3 * torch.randn(B, C, H, W))
        stats = _lib.gn_stats(x, 32)
        tiles, taps = B * (H // t) * (W // t), (t + 2) ** 2
        for silu in (True, False):
            xn = _lib.gn_apply(x, gamma, beta, 32, eps, silu, stats)
            for planes in (2, 3):
                fused = torch.zeros((taps, tiles, planes * C), dtype=torch.float16, device=DEV)
                plain = torch.zeros_like(fused)
                _lib._wino_in(L, x, fused, (gamma, beta, 32, eps, silu, stats, None), t, planes, 8.0)
                _lib._wino_in(L, xn, plain, None, t, planes, 8.0)
                assert torch.equal(fused, plain), (t, H, W, silu, planes)


@pytest.mark.parametrize("t", (2, 4))
def test_plain_output_transforms_read_and_write_the_right_elements(t, offsets):
    from pit_hip import _lib

    L, C = _lib.lib(), 128
    for H, W in SHAPES:
        tiles, taps = B * (H // t) * (W // t), (t + 2) ** 2
        M = ints(taps, tiles, C, seed=200 * t + H).to(DEV)
        y = torch.full((B, C, H, W), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
        fn = L.wino4_out_nhwc_f32 if t == 4 else L.wino_out_nhwc_f32
        _lib._check(fn(M.data_ptr(), y.data_ptr(), B, H, W, C, 0.25, _lib._stream()), "wino_out_nhwc_f32")
        assert torch.equal(y.double(), 0.25 * ref_output_transform(M, t, H, W)), (t, H, W)


@pytest.mark.parametrize("t,C", ((2, 128), (4, 128), (4, 1024)))
def test_wino_out_res_reads_and_writes_the_right_elements_and_sums_them_exactly(t, C, offsets):
    """y = A^T M A + bias (+ res) with and without residual and bias, and the statistics records of y against exact integer sums"""
    from pit_hip import _lib

    L, groups = _lib.lib(), 32
    for H, W in SHAPES:
        tiles, taps = B * (H // t) * (W // t), (t + 2) ** 2
        M = ints(taps, tiles, C, seed=300 * t + H + C).to(DEV)
        res, bias = nhwc(ints(B, C, H, W, seed=7 * t + W + C)), ints(C, seed=11 * t + C).to(DEV)
        base = ref_output_transform(M, t, H, W)
        for r, b in ((None, None), (res, None), (None, bias), (res, bias)):
            y, stats = _lib._out_and_stats(res, C, H, W, groups)
            y.fill_(7.0)
            _lib._check(L.wino_out_res_nhwc_f32(M.data_ptr(), _lib._ptr(r), _lib._ptr(b), y.data_ptr(), stats.data_ptr(), B, H, W, C,
                                                groups, t, 1.0, _lib._stream()), "wino_out_res_nhwc_f32")
            want = base + (0 if r is None else r.double()) + (0 if b is None else b.double().view(1, C, 1, 1))
            assert torch.equal(y.double(), want), (t, C, H, W, r is not None, b is not None)
            g = want.reshape(B, groups, -1)
            sums = torch.stack([g.sum(2), (g * g).sum(2)], 2).flatten()
            assert torch.equal(_lib.gn_stats_values(stats), sums), (t, C, H, W, r is not None, b is not None)


def test_the_fp32_twin_test_holds_on_the_wide_kernels(monkeypatch):
    """test_gpu_convstack_kernels.py's bit-equality of the fused fp32 input transforms with gn_apply + their plain twins, with every
    transform of it on the wide kernels"""
    import test_gpu_convstack_kernels as K

    monkeypatch.setenv("GQHIP_WINO_WIDE", "1")
    K.test_fused_groupnorm_consumers_equal_gn_apply_then_their_plain_twins()
