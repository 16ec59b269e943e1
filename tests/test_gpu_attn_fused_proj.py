"""-m gpu: the attention block's 1x1 GEMM with GroupNorm in its staging, the attention operands in its epilogue, and its
128-pixel tiling (csrc/gq_conv3.h: conv1x1_f16x3_kernel<COUT, RR, GN, SPLIT>).

Every variant does the arithmetic of the route it replaces on the same values, so every comparison here is torch.equal / byte
equality -- no tolerance:

* GN      against gn_silu(silu=False) followed by conv1x1_direct, on groups whose |mean| / std is ~100 (the manner of
          test_gpu_groupnorm_offsets.py: a wrong shift cannot hide behind a zero-mean input);
* SPLIT   against the fp32 projection followed by attn_split_qkv_f16x3, with guard rows around Q3 / K3 / V3;
* tilings forced by GQHIP_CONV1_TILE against each other, output and statistics records;
* AttnBlock with the route on and off (and, as a gross check only, under the propagated fp64 model of
  test_gpu_convstack_routes.py).

Shapes are the smallest that reach every path: 16 x 16 pixels = one 256-pixel tile or two 128-pixel tiles per image, two images,
Cin = 128 / 256 (4 / 8 stages: the LDS double buffer wraps two / four times), 24 x 16 pixels for the 128-pixel tail.
"""
import pytest
import torch

import convstack_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]
DEV = "cuda:0"
EPS = 1e-6
TILINGS = ("128", "256")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _offset_input(B, C, H, W, seed, pending):
    """(x, pre_bias or None): per group v = +-100 s + s randn, s in {2^-6, 1, 2^6}; with ``pending`` the offset sits in the
    pending bias (per channel) and x carries the spread."""
    g = torch.Generator().manual_seed(seed)
    grp = torch.arange(C) // (C // 32)
    s = 2.0 ** (6.0 * ((grp % 3).double() - 1.0))
    off = torch.where(grp % 2 == 0, 100.0, -100.0) * s
    x = s[None, :, None, None] * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    if pending:
        return _cl(x.float().to(DEV)), off.float().to(DEV)
    return _cl((x + off[None, :, None, None]).float().to(DEV)), None


def _norm(C, seed):
    norm = torch.nn.GroupNorm(32, C, eps=EPS).to(DEV)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        norm.weight.copy_((torch.rand(C, generator=g) * 2 + 0.25).to(DEV))
        norm.bias.copy_(torch.randn(C, generator=g).to(DEV))
    return norm


def _gn_tuple(norm, x, pb):
    from pit_hip import _lib

    return (norm.weight, norm.bias, 32, EPS, False, _lib.gn_stats(x, 32, pb), pb)


# ------------------------------------------------------------------------------------------ 1. GroupNorm in the staging
@pytest.mark.parametrize("tile", TILINGS)
@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("cin", [128, 256])
def test_groupnorm_variant_equals_the_two_pass_route(cin, pending, tile, monkeypatch):
    """Cin = 128: 4 channels per group, the smallest the NHWC GroupNorm kernels take (Cin = 64, 2 per group, is rejected)."""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    monkeypatch.setenv("GQHIP_CONV1_TILE", tile)
    B, H, W = 2, 16, 16
    x, pb = _offset_input(B, cin, H, W, cin + pending, pending)
    norm = _norm(cin, 3)
    torch.manual_seed(cin)
    conv = torch.nn.Conv2d(cin, 128, 1).to(DEV)
    wf, us = _lib.conv3_weights_f16(conv.weight)
    bound = U._gn_act_bound(norm, x)
    y = _lib.gn_silu(x, norm.weight, norm.bias, 32, EPS, silu=False, pre_bias=pb)
    want = _lib.conv1x1_direct(y, wf, us, bound, bias=conv.bias)
    got = _lib.conv1x1_direct(x, wf, us, bound, bias=conv.bias, gn=_gn_tuple(norm, x, pb))
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0.1
    assert torch.equal(got, want)


def test_two_channels_per_group_is_rejected():
    """Cin = 64 with 32 groups: the NHWC GroupNorm kernels need 4 | channels per group, and so does the variant."""
    from pit_hip import _lib

    x = _cl(torch.randn(2, 64, 16, 16, device=DEV))
    norm = _norm(64, 3)
    wf, us = _lib.conv3_weights_f16(torch.randn(128, 64, 1, 1, device=DEV))
    stats = torch.zeros(_lib.GNSTAT_WORDS * 2 * 32, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.GqHipError):
        _lib.conv1x1_direct(x, wf, us, 8.0, gn=(norm.weight, norm.bias, 32, EPS, False, stats, None))
    rc = _lib.lib().conv1x1_gn_f16x3(x.data_ptr(), norm.weight.data_ptr(), norm.bias.data_ptr(), None, stats.data_ptr(), 32, EPS,
                                     wf.data_ptr(), 1.0, 1.0, None, None, x.data_ptr(), None, 2, 256, 64, 128, 1, _lib._stream())
    assert rc != 0      # refused before any launch: y is never written


# ------------------------------------------------------------------------------------------ 2. the split epilogue
GUARD = 4            # rows before and after each operand buffer
SENTINEL = 0x5A3C    # fp16 bit pattern of the guards (and of the buffers before the call)


def _guarded(rows, width):
    buf = torch.full(((rows + 2 * GUARD) * width,), SENTINEL, dtype=torch.int16, device=DEV)
    return buf, buf[GUARD * width: (GUARD + rows) * width].view(torch.float16)


def _guards_intact(buf, rows, width):
    return bool((buf[: GUARD * width] == SENTINEL).all()) and bool((buf[(GUARD + rows) * width:] == SENTINEL).all())


def _projection(x, wf, us, bound, bias, gn):
    """The fp32 q | k | v projection [B, L, 3C] the existing route stores: one conv1x1_direct where the kernel is instantiated
    for 3C columns, else one per third on slices of the SAME operand-order weights (same u_scale: same bits per column)."""
    from pit_hip import _lib

    cout = wf.shape[2] * 32
    if cout in (128, 256, 512, 1536):
        y = _lib.conv1x1_direct(x, wf, us, bound, bias=bias, gn=gn)
    else:
        n = wf.shape[2] // 3
        y = torch.cat([_lib.conv1x1_direct(x, wf[:, :, n * t: n * (t + 1)].contiguous(), us, bound,
                                           bias=bias[32 * n * t: 32 * n * (t + 1)].contiguous(), gn=gn) for t in range(3)], 1)
    return y.permute(0, 2, 3, 1).reshape(x.shape[0], x.shape[2] * x.shape[3], cout).contiguous()


@pytest.mark.parametrize("tile", TILINGS)
@pytest.mark.parametrize("with_gn", [False, True])
@pytest.mark.parametrize("C,H,W,B", [(128, 16, 16, 2), (512, 16, 16, 1)])
def test_split_epilogue_equals_projection_plus_attn_split_qkv(C, H, W, B, with_gn, tile, monkeypatch):
    """C = 128, L = 256, B = 2: three column blocks, one each of q, k, v.  C = 512, one 256-pixel tile per image (L = 256): four
    blocks per third; with GQHIP_CONV1_TILE = 128 the same as two tiles.  (A 64-token image has no whole tile of either
    tiling: test_tokens_below_a_tile_are_rejected.)"""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    monkeypatch.setenv("GQHIP_CONV1_TILE", tile)
    L = H * W
    x, _ = _offset_input(B, C, H, W, C + B, False)
    if not with_gn:
        x = _cl(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C)).to(DEV))
    norm = _norm(C, 5)
    torch.manual_seed(C + 1)
    w = torch.randn(3 * C, C, 1, 1, device=DEV) * C ** -0.5
    bias = torch.randn(3 * C, device=DEV)
    wf, us = _lib.conv3_weights_f16(w)
    bound = U._gn_act_bound(norm, x) if with_gn else float(x.abs().max())
    gn = _gn_tuple(norm, x, None) if with_gn else None
    qkv = _projection(x, wf, us, bound, bias, gn)
    sq, sv = _lib.attention_scales(float(qkv[..., : 2 * C].abs().max()), float(qkv[..., 2 * C:].abs().max()))
    want = _lib.attention_operands(B, L, C, DEV)
    _lib._check(_lib.lib().attn_split_qkv_f16x3(qkv.data_ptr(), want[0].data_ptr(), want[1].data_ptr(), want[2].data_ptr(), B, L,
                                                C, sq, sv, _lib._stream()), "attn_split_qkv_f16x3")
    shapes = ((B * L, 3 * C), (B * L, 3 * C), (B * 3 * L, C))
    bufs = [_guarded(*s) for s in shapes]
    out = tuple(v.view(sh) for (_, v), sh in zip(bufs, ((B, L, 3 * C), (B, L, 3 * C), (B, 3 * L, C))))
    got = _lib.qkv_split_direct(x, wf, us, bound, sq, sv, bias=bias, gn=gn, out=out)
    torch.cuda.synchronize()
    for name, g, wnt, (buf, _), s in zip("QKV", got, want, bufs, shapes):
        assert torch.equal(g.view(torch.int16), wnt.view(torch.int16)), name + "3 differs"
        assert _guards_intact(buf, *s), name + "3: guard rows written"
    assert float(want[0].float().abs().max()) > 1.0


def test_tokens_below_a_tile_are_rejected():
    """C = 512, L = 64, B = 1: 64 tokens hold no whole tile (tiles never span images), so the split projection refuses the shape
    as conv1x1_direct does, and AttnBlock keeps the unfused route there."""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    x = _cl(torch.randn(1, 512, 8, 8, device=DEV))
    w = torch.randn(1536, 512, 1, 1, device=DEV) * 0.05
    wf, us = _lib.conv3_weights_f16(w)
    with pytest.raises(_lib.GqHipError):
        _lib.qkv_split_direct(x, wf, us, 4.0, 1.0, 1.0)
    with pytest.raises(_lib.GqHipError):
        _lib.conv1x1_direct(x, wf, us, 4.0)
    blk = U.AttnBlock(512).eval().to(DEV).to(memory_format=torch.channels_last)
    with torch.no_grad():
        assert blk._fused_proj_attention(x) is None


# ------------------------------------------------------------------------------------------ 3. tilings
@pytest.mark.parametrize("full", [True, False])
def test_tilings_give_the_same_output_and_statistics(full, monkeypatch):
    """16 x 16 pixels: both tilings, output and statistics records equal.  24 x 16 pixels (HW = 384 = 256 + a 128-pixel tail): the
    automatic choice routes it to 128-pixel tiles, a forced 256 is rejected; its output equals rows 0..23 of the 256-pixel
    tiling on the image padded to 32 x 16 (a pixel's result depends on that pixel alone), its records those of gn_stats."""
    from pit_hip import _lib

    B, cin, cout = 2, 256, 256
    torch.manual_seed(31 + full)
    conv = torch.nn.Conv2d(cin, cout, 1).to(DEV)
    wf, us = _lib.conv3_weights_f16(conv.weight)

    def run(x, res, tile):
        if tile is None:
            monkeypatch.delenv("GQHIP_CONV1_TILE", raising=False)
        else:
            monkeypatch.setenv("GQHIP_CONV1_TILE", tile)
        if full:
            return _lib.conv1x1_direct(x, wf, us, float(x.abs().max()), residual=res, bias=conv.bias, stats_groups=32)
        return _lib.conv1x1_direct(x, wf, us, float(x.abs().max())), None

    x = _cl(torch.randn(B, cin, 16, 16, device=DEV) + 3.0)
    res = _cl(torch.randn(B, cout, 16, 16, device=DEV) * 5 - 20.0)
    y128, st128 = run(x, res, "128")
    y256, st256 = run(x, res, "256")
    assert torch.equal(y128, y256) and float(y256.abs().max()) > 0.1
    if full:
        assert torch.equal(st128, st256)
        assert not torch.equal(st256, torch.zeros_like(st256))

    xt = _cl(torch.randn(B, cin, 24, 16, device=DEV) + 3.0)
    rt = _cl(torch.randn(B, cout, 24, 16, device=DEV) * 5 - 20.0)
    with pytest.raises(_lib.GqHipError):
        run(xt, rt, "256")
    ya, sta = run(xt, rt, None)
    yf, stf = run(xt, rt, "128")
    pad = lambda t: _cl(torch.cat([t, torch.zeros_like(t[:, :, :8])], 2))
    yp, _ = run(pad(xt), pad(rt), "256")
    assert torch.equal(ya, yf) and torch.equal(ya, yp[:, :, :24])
    if full:
        assert torch.equal(sta, stf)
        got, want = _lib.gn_stats_values(sta), _lib.gn_stats_values(_lib.gn_stats(ya, 32))
        # both are exact sums of per-thread fp64 partials of the same fp32 values: they differ by the partials' roundings only
        assert float(((got - want).abs() / (want.abs() + 1e-30)).max()) <= 2.0 ** -40


# ------------------------------------------------------------------------------------------ 4. AttnBlock end to end
def test_attn_block_fused_projection_route_on_and_off():
    """c = 512, B = 2, 16 x 16, no_grad, channels_last: the route on and off are torch.equal (output and the statistics left for
    the next GroupNorm) -- that comparison carries this test.  The propagated fp64 model of test_gpu_convstack_routes.py (the
    tolerance the suite has for this block) is applied as well, but the route uses a vanishing fraction of it on this input: it
    guards against a gross error only, the unfused route being gated there."""
    from pit_hip.modules import unet as U

    torch.manual_seed(7)
    att = U.AttnBlock(512).eval().to(DEV).to(memory_format=torch.channels_last)
    x = _cl(torch.randn(2, 512, 16, 16, device=DEV) * 1.5 + 0.5)
    assert U.ATTN_FUSED_PROJ
    with torch.no_grad():
        assert att._fused_proj_attention(x) is not None      # the route is taken at this shape
        y_on = att(x)
        U.ATTN_FUSED_PROJ = False
        try:
            y_off = att(x)
        finally:
            U.ATTN_FUSED_PROJ = True
        ref, bound = R.attn_ref_and_bound(R.twin64(att), R.d64(x), c_proj=R.C_F16X3)
    assert torch.equal(y_on, y_off)
    assert torch.equal(U._left_stats(y_on, 32), U._left_stats(y_off, 32))
    R.bound_gate(y_on, ref, bound, "AttnBlock 512 at 16 x 16, fused projection")
