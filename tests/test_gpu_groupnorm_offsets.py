"""-m gpu: the conv stack's GroupNorm statistics on groups whose mean is large against their spread (mean / std up to 1000).

Every GroupNorm of the channels_last stack reads a statistics record (csrc/gq_stats.h) that the kernel which produced its input
left behind, and forms var = SS / n - mean^2 from it.  The relative error of that difference grows like (mean / std)^2 times
the relative error of SS, so a record that is accurate relative to sum v^2 can still be useless for the variance of an
offset-dominated group: flat images, letterboxed frames, large biases.  The other GroupNorm tests draw zero-mean-ish data and
cannot see this.

Inputs: each (image, group) gets its own offset c_g and spread s_g, x = c_g + s_g randn, c / s in {0, 1, 10, 100, 1000},
s in {2^-10, 1, 2^10}, signs alternating, plus an exactly constant group, a group of constant but different channels and
groups with one outlier pixel (at the first pixel of the image -- the first value some thread sees -- and inside it).

Gates (u = 2^-24, eps = 1e-6, every GroupNorm of this UNet), fixed by the error model and not read off a run:

* producers -- the record decoded with _lib.gn_stats_values and the readers' formula, against fp64 statistics of the fp32
  tensor the kernel wrote (with a pending bias: of the fp32 sum x + pre_bias the kernel forms):
      |mean - mean64| <= 8 u (|mean64| + std64)
      |var - var64|   <= 8 u (var64 + eps) + 2^-50 mean64^2
  8 u is what tests/convstack_ref.py:gn_own_error charges the statistics.  u eps: below that the record cannot move
  rstd = (var + eps)^-1/2 by more than 8 u relative.  2^-50 mean^2: the readers' own fp64 evaluation of SS / n - mean^2
  (three roundings of ~mean^2 at 2^-53), 2^26 times below u -- needed only where var64 is 0 or nearly so.
  Neither constant depends on mean / std: that is the property under test.
* consumers -- output against fp64 F.group_norm (+ SiLU) of the same fp32 input (+ pending bias), gated by the unchanged
  convstack_ref.gn_own_error; fused into a convolution, the convolution's charge plus gn_own_error propagated through |w|
  (the pattern of test_gpu_convstack_routes.py).  torch's fp32 F.group_norm is printed next to each case as a yardstick.
* modules -- the full-size Encoder / Decoder on flat inputs against the fp64 twin under the product contract.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import convstack_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]
DEV = "cuda:0"
U24 = R.U24
EPS = 1e-6
K_MEAN = 8.0
K_VAR = 8.0
RATIOS = (0.0, 1.0, 10.0, 100.0, 1000.0)
SIGMAS = (2.0 ** -10, 1.0, 2.0 ** 10)
FULL = dict(attn_type="vanilla", double_z=True, z_channels=16, resolution=256, in_channels=3, out_ch=3, ch=128,
            ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[32], dropout=0.0)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@contextlib.contextmanager
def switch(**flags):
    from pit_hip.modules import unet as U

    old = {k: getattr(U, k) for k in flags}
    try:
        for k, v in flags.items():
            setattr(U, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(U, k, v)


def offset_groups(B, C, H, W, groups=32, seed=0):
    """fp32 [B, C, H, W] (CPU, NCHW): per (image, group) x = c + s randn over the sweep, then the special groups."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    cases = [(r, s) for r in RATIOS for s in SIGMAS] + ["const", "channels", "outlier0", "outlier"]
    x = torch.empty(B, groups, cpg, H, W, dtype=torch.float64)
    for k in range(B * groups):
        b, gi = divmod(k, groups)
        case = cases[k % len(cases)]
        sign = -1.0 if (k // len(cases) + k) % 2 else 1.0
        noise = torch.randn(cpg, H, W, generator=g, dtype=torch.float64)
        if case == "const":
            x[b, gi] = sign * 1.7
        elif case == "channels":
            x[b, gi] = sign * 100.0 + torch.arange(cpg, dtype=torch.float64)[:, None, None]
        elif case in ("outlier0", "outlier"):
            x[b, gi] = sign * 100.0 + noise
            if case == "outlier0":
                x[b, gi, 0, 0, 0] += 1000.0
            else:
                x[b, gi, cpg // 2, H // 3, W // 2] += 1000.0
        else:
            r, s = case
            x[b, gi] = sign * r * s + s * noise
    return x.reshape(B, C, H, W).float()


def pending_bias_groups(B, C, H, W, groups=32, seed=0):
    """The pending-bias form of the sweep: (x, pre_bias), fp32 on the device, x channels_last.  A pending bias is a convolution's
    bias not yet added, so it carries each group's offset (per channel, the same for every image) and x the spread."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    cases = [(r, s) for r in RATIOS for s in SIGMAS] + ["const", "channels", "outlier0", "outlier"]
    x = torch.zeros(B, groups, cpg, H, W, dtype=torch.float64)
    pb = torch.empty(groups, cpg, dtype=torch.float64)
    for gi in range(groups):
        case = cases[gi % len(cases)]
        sign = -1.0 if gi % 2 else 1.0
        noise = torch.randn(B, cpg, H, W, generator=g, dtype=torch.float64)
        if case == "const":
            pb[gi] = sign * 1.7
        elif case == "channels":
            pb[gi] = sign * 100.0 + torch.arange(cpg, dtype=torch.float64)
        elif case in ("outlier0", "outlier"):
            pb[gi], x[:, gi] = sign * 100.0, noise
            if case == "outlier0":
                x[:, gi, 0, 0, 0] += 1000.0
            else:
                x[:, gi, cpg // 2, H // 3, W // 2] += 1000.0
        else:
            r, s = case
            pb[gi], x[:, gi] = sign * r * s, s * noise
    return _cl(x.reshape(B, C, H, W).float().to(DEV)), pb.reshape(C).float().to(DEV)


def _readers_view(st, B, groups, n):
    """(mean, var) per (image, group) from a record, by the consumers' formula (gq_unet_aux.h:gn_apply_*)."""
    from pit_hip import _lib

    v = _lib.gn_stats_values(st).view(B * groups, 2)
    mean = v[:, 0] / n
    var = (v[:, 1] / n - mean * mean).clamp_min(0.0)
    return mean, var


def check_record(st, y, groups, what):
    """Producer gate (module docstring); prints the fraction of each gate used per decade of |mean| / std."""
    y64 = R.d64(y)
    B, C = y64.shape[0], y64.shape[1]
    g = y64.reshape(B * groups, -1)
    n = g.shape[1]
    m64 = g.mean(1)
    v64 = ((g - m64[:, None]) ** 2).mean(1)
    sd64 = v64.sqrt()
    mean, var = _readers_view(st, B, groups, n)
    assert torch.isfinite(mean).all() and torch.isfinite(var).all(), what
    fm = (mean - m64).abs() / (K_MEAN * U24 * (m64.abs() + sd64) + 1e-300)
    fv = (var - v64).abs() / (K_VAR * U24 * (v64 + EPS) + 2.0 ** -50 * m64 * m64)
    ratio = m64.abs() / sd64.clamp_min(1e-300)
    dec = torch.where(sd64 > 0, ratio.clamp(1e-1, 1e5).log10().round(), torch.full_like(ratio, float("inf")))
    parts = []
    for d in sorted(set(dec.tolist())):
        sel = dec == d
        lab = "std 0" if d == float("inf") else f"~1e{int(d)}"
        parts.append(f"{lab}: mean {float(fm[sel].max()):.3f} var {float(fv[sel].max()):.3f}")
    print(f"[stats] {what}: fraction of gate by |mean|/std -- " + "; ".join(parts))
    assert float(fm.max()) <= 1.0 and float(fv.max()) <= 1.0, (what, float(fm.max()), float(fv.max()))
    return float(fm.max()), float(fv.max())


def _norm(C, seed):
    norm = torch.nn.GroupNorm(32, C, eps=EPS).to(DEV)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        norm.weight.copy_((torch.rand(C, generator=g) * 2 + 0.25).to(DEV))
        norm.bias.copy_((torch.randn(C, generator=g)).to(DEV))
    return norm


def check_consumer(got, xin64, norm, act, what, xin32=None):
    """|got - GN64| <= gn_own_error; torch's fp32 GroupNorm of the same input printed as a yardstick."""
    ref = F.group_norm(xin64, norm.num_groups, norm.weight.double(), norm.bias.double(), norm.eps)
    if act:
        ref = F.silu(ref)
    bound = R.gn_own_error(norm, xin64, act)
    extra = ""
    if xin32 is not None:
        t32 = F.group_norm(xin32.contiguous(), norm.num_groups, norm.weight, norm.bias, norm.eps)
        t32 = F.silu(t32) if act else t32
        extra = f" (torch fp32 GroupNorm: {float(((t32.double() - ref).abs() / bound).max()):.3f})"
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    used = float(((got.double() - ref).abs() / bound).max())
    print(f"[gn] {what}: {used:.3f} of gn_own_error{extra}")
    assert used <= 1.0, (what, used)
    return used


# ------------------------------------------------------------------------------------------ producers
@pytest.mark.parametrize("C,H,W", [(128, 24, 40), (256, 20, 22), (512, 8, 12), (128, 64, 64)])
def test_statistics_kernels_on_offset_groups(C, H, W):
    """gn_stats (NHWC, with and without a pending bias), the NCHW statistics pass of gn_silu, add_bias_stats."""
    from pit_hip import _lib

    B = 2
    x = offset_groups(B, C, H, W, seed=C + H).to(DEV)
    xl = _cl(x)
    n_words = _lib.GNSTAT_WORDS * B * 32
    check_record(_lib.gn_stats(xl, 32), xl, 32, f"gn_stats NHWC C{C} {H}x{W}")
    xm, pb = pending_bias_groups(B, C, H, W, seed=C + H + 1)
    check_record(_lib.gn_stats(xm, 32, pb), xm + pb[None, :, None, None], 32, f"gn_stats NHWC + pending bias C{C} {H}x{W}")
    norm = _norm(C, 1)
    for layout, xx in (("NCHW", x.contiguous()), ("NHWC", xl)):
        arena = _lib.StatsArena()
        arena.want = n_words
        with _lib.stats_arena(arena, x.device):
            _lib.gn_silu(xx, norm.weight, norm.bias, 32, EPS, silu=True)
            rec = arena.buf[:n_words].clone()
        check_record(rec, xx, 32, f"gn_silu's statistics pass {layout} C{C} {H}x{W}")
    a = _cl(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(4)).to(DEV))
    bias = torch.randn(C, generator=torch.Generator().manual_seed(5)).to(DEV)
    y, st = _lib.add_bias_stats(a, _cl(xl - a), bias, 32)
    check_record(st, y, 32, f"add_bias_stats C{C} {H}x{W}")


def _conv_out_offsets(cout, seed):
    """Per-output-channel bias that puts each output group at its own offset (sign alternating, 1 .. 1e3 x the conv's spread)."""
    g = torch.Generator().manual_seed(seed)
    grp = torch.arange(cout) // (cout // 32)
    return (torch.where(grp % 2 == 0, 1.0, -1.0) * 10.0 ** (grp % 4).double() * 0.5 * (1 + 0.1 * torch.rand(cout, generator=g, dtype=torch.float64))).float()


def _res_offsets(B, cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    off = (torch.rand(B, 32, generator=g) * 2 - 1) * 300.0
    return _cl((off.repeat_interleave(cout // 32, 1)[:, :, None, None] + 0.05 * torch.randn(B, cout, H, W, generator=g)).to(DEV))


def test_winograd_output_transform_statistics_on_offset_groups():
    """wino_out_res_nhwc_kernel through wino_conv3x3(stats_groups=32): fp32 and f16 x 3 GEMMs, F(2,3) and F(4,3), with and
    without a residual; the output's groups sit at offsets of 0.5 .. 500 x their spread (bias) and +-300 (residual)."""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    torch.manual_seed(8)
    for cin, cout, B, H, W in ((256, 256, 2, 16, 24), (128, 512, 1, 8, 12)):
        conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).to(DEV)
        with torch.no_grad():
            conv.weight.mul_(0.2)
            conv.bias.copy_(_conv_out_offsets(cout, cin).to(DEV))
        x = _cl(torch.randn(B, cin, H, W).to(DEV))
        res = _res_offsets(B, cout, H, W, cout)
        for f4 in (False, True):
            Uw = U._wino_weights(conv, f4)
            u3, us, wf2 = U._wino_weights_f16(conv, f4)
            for route, f16 in (("fp32", None), ("f16x3", (u3, us, float(x.abs().max()), None))):
                for r in (None, res):
                    y, st = _lib.wino_conv3x3(x, Uw, residual=r, bias=conv.bias, stats_groups=32, f16=f16)
                    check_record(st, y, 32, f"Winograd F({4 if f4 else 2},3) {route} {cin}->{cout} residual {r is not None}")


def test_direct_conv_epilogue_statistics_on_offset_groups():
    """conv3_epilogue (conv3x3_direct, conv1x1_direct, conv3x3s2_direct) and upconv2x_f16x3_kernel (the decoder's Upsample)."""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    torch.manual_seed(9)
    # 3x3 with GroupNorm + SiLU of an offset input fused in, bias + offset residual
    for cin, cout, (B, H, W) in ((128, 128, (2, 16, 64)), (256, 256, (1, 8, 32)), (512, 128, (1, 8, 32))):
        conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).to(DEV)
        with torch.no_grad():
            conv.weight.mul_(0.2)
            conv.bias.copy_(_conv_out_offsets(cout, cin).to(DEV))
        norm = _norm(cin, 2)
        x = _cl(offset_groups(B, cin, H, W, seed=11).to(DEV))
        wf, us = _lib.conv3_weights_f16(conv.weight)
        gn = (norm.weight, norm.bias, 32, EPS, True, _lib.gn_stats(x, 32), None)
        for r in (None, _res_offsets(B, cout, H, W, 12)):
            y, st = _lib.conv3x3_direct(x, wf, us, U._gn_act_bound(norm, x), gn=gn, residual=r, bias=conv.bias, stats_groups=32)
            check_record(st, y, 32, f"conv3x3_direct {cin}->{cout} residual {r is not None}")
    # 1x1 (offset input, pending bias, offset output)
    for cin, cout, (B, H, W) in ((256, 128, (2, 16, 32)), (512, 512, (1, 16, 16))):
        conv = torch.nn.Conv2d(cin, cout, 1).to(DEV)
        with torch.no_grad():
            conv.weight.mul_(0.2)
            conv.bias.copy_(_conv_out_offsets(cout, cin + 1).to(DEV))
        x = _cl(offset_groups(B, cin, H, W, seed=13).to(DEV) * 1e-3)
        pb = torch.randn(cin, device=DEV) * 0.01
        wf, us = _lib.conv3_weights_f16(conv.weight)
        scales = _lib.f16_scales(_lib.gn_stats(x, 32, pb), 1.0, us)
        y, st = _lib.conv1x1_direct(x, wf, us, scales, residual=_res_offsets(B, cout, H, W, 14), bias=conv.bias, stats_groups=32,
                                    pre_bias=pb)
        check_record(st, y, 32, f"conv1x1_direct {cin}->{cout}")
    # stride 2 (Downsample)
    for cin, cout, (B, H, W) in ((128, 128, (2, 32, 128)), (256, 512, (1, 16, 64))):
        conv = torch.nn.Conv2d(cin, cout, 3, 2, 0).to(DEV)
        with torch.no_grad():
            conv.weight.mul_(0.2)
            conv.bias.copy_(_conv_out_offsets(cout, cin + 2).to(DEV))
        x = _cl(torch.randn(B, cin, H, W, device=DEV))
        wf, us = _lib.conv3s2_weights_f16(conv.weight)
        y, st = _lib.conv3x3s2_direct(x, wf, us, float(x.abs().max()), bias=conv.bias, stats_groups=32)
        check_record(st, y, 32, f"conv3x3s2_direct {cin}->{cout}")
    # sub-pixel upsample + conv
    for ch, B, H, W in ((512, 1, 8, 32), (256, 2, 24, 64)):
        up = U.Upsample(ch).to(DEV).eval().to(memory_format=torch.channels_last)
        with torch.no_grad():
            up.conv.weight.mul_(0.2)
            up.conv.bias.copy_(_conv_out_offsets(ch, ch + 3).to(DEV))
        x = _cl(torch.randn(B, ch, H, W, device=DEV))
        U._leave_stats(x, _lib.gn_stats(x, 32), 32)
        with torch.no_grad(), switch(DIRECT_UPCONV=True):
            y, pb = up(x)
        assert pb is None
        st, groups = U._left_stats(y, 32), 32
        check_record(st, y, groups, f"upconv2x_direct {ch} ch {H}x{W}")


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 24, 96)])
def test_conv_in_small_statistics_on_flat_images(B, H, W):
    """conv3x3_cin_small: the encoder's first conv, the first producer a flat image reaches.  Images: constant gray levels, a
    letterboxed frame, a low-contrast frame; conv_in's bias puts the output groups at offsets of ~1 .. 1e3 x their spread."""
    from pit_hip import _lib

    g = torch.Generator().manual_seed(21)
    conv = torch.nn.Conv2d(3, 128, 3, 1, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.3)
        conv.bias.copy_(_conv_out_offsets(128, 22).to(DEV))
    wk = _lib.conv_cin_small_weights(conv.weight)
    imgs = [torch.full((B, 3, H, W), v) for v in (-1.0, 0.25, 1.0)]
    lb = torch.full((B, 3, H, W), -1.0)
    lb[:, :, H // 4: H - H // 4] = torch.rand(B, 3, H - 2 * (H // 4), W, generator=g) * 2 - 1
    imgs += [lb, 0.3 + 1e-3 * torch.randn(B, 3, H, W, generator=g)]
    for k, img in enumerate(imgs):
        y, st = _lib.conv3x3_cin_small(_cl(img.to(DEV)), wk, conv.bias, stats_groups=32)
        check_record(st, y, 32, f"conv3x3_cin_small image {k} {B}x{H}x{W}")


# ------------------------------------------------------------------------------------------ consumers
@pytest.mark.parametrize("C,H,W", [(128, 24, 40), (256, 20, 22), (512, 8, 12)])
def test_groupnorm_consumers_on_offset_groups(C, H, W):
    """gn_apply (NHWC: record from gn_stats, with and without a pending bias; from add_bias_stats), gn_silu (NCHW and NHWC, its
    own statistics pass), against fp64 GroupNorm (+ SiLU) under gn_own_error."""
    from pit_hip import _lib

    B = 2
    x = offset_groups(B, C, H, W, seed=C + 7).to(DEV)
    xl = _cl(x)
    x64 = R.d64(x)
    norm = _norm(C, 3)
    for act in (False, True):
        y = _lib.gn_apply(xl, norm.weight, norm.bias, 32, EPS, act, _lib.gn_stats(xl, 32))
        check_consumer(y, x64, norm, act, f"gn_apply(gn_stats) C{C} {H}x{W} silu {act}", x)
        for layout, xx in (("NCHW", x.contiguous()), ("NHWC", xl)):
            y = _lib.gn_silu(xx, norm.weight, norm.bias, 32, EPS, silu=act)
            check_consumer(y, x64, norm, act, f"gn_silu {layout} C{C} {H}x{W} silu {act}", x)
    # pending bias: the GroupNorm is of x + pb (in fp64), the kernels fold pb into the shift
    xm, pb = pending_bias_groups(B, C, H, W, seed=C + 8)
    xin64 = R.d64(xm) + R.d64(pb)[None, :, None, None]
    for act in (False, True):
        for layout, xx in (("NCHW", xm.contiguous()), ("NHWC", xm)):
            y = _lib.gn_silu(xx, norm.weight, norm.bias, 32, EPS, silu=act, pre_bias=pb)
            check_consumer(y, xin64, norm, act, f"gn_silu + pending bias {layout} C{C} {H}x{W} silu {act}",
                           xm + pb[None, :, None, None])
    a = _cl(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(4)).to(DEV))
    bias = torch.randn(C, generator=torch.Generator().manual_seed(5)).to(DEV)
    s, st = _lib.add_bias_stats(a, _cl(xl - a), bias, 32)
    y = _lib.gn_apply(s, norm.weight, norm.bias, 32, EPS, True, st)
    check_consumer(y, R.d64(s), norm, True, f"gn_apply(add_bias_stats) C{C} {H}x{W}", s)


def test_fused_groupnorm_convolutions_on_offset_groups():
    """The consumers that fuse GroupNorm (+ SiLU) into a convolution's input: conv3x3_gn_small (decoder conv_out),
    conv3x3_f32(gn=...) (encoder conv_out), conv3x3_direct(gn=...) and the Winograd input transforms (wino_conv3x3(gn=...),
    F(2,3) and F(4,3)) -- each against an fp64 convolution of the fp64 GroupNorm of the same input: the convolution's charge
    of sum |act||w| plus gn_own_error propagated through |w|, x 1.25 for the second order (convstack_ref)."""
    from pit_hip import _lib
    from pit_hip.modules import unet as U

    torch.manual_seed(10)

    def gate(y, xin64, norm, conv_w, c, padding, what):
        a64 = F.silu(F.group_norm(xin64, 32, norm.weight.double(), norm.bias.double(), EPS))
        ref, mag = R.conv_ref_and_mag(a64, conv_w.double(), None, 1, padding)
        gnerr = F.conv2d(R.gn_own_error(norm, xin64, True), conv_w.double().abs(), None, 1, padding)
        R.bound_gate(y, ref, R.SECOND_ORDER * (c * mag + gnerr), what)

    for cin, (B, H, W) in ((128, (2, 16, 32)), (256, (1, 16, 32))):
        x = _cl(offset_groups(B, cin, H, W, seed=cin + 1).to(DEV))
        xm, pb = pending_bias_groups(B, cin, H, W, seed=cin + 2)
        norm = _norm(cin, 4)
        for pre in (None, pb):
            xx = x if pre is None else xm
            xin64 = R.d64(x) if pre is None else R.d64(xm) + R.d64(pre)[None, :, None, None]
            st = _lib.gn_stats(xx, 32, pre)
            gn = (norm.weight, norm.bias, 32, EPS, True, st, pre)
            tag = f"{cin} ch {H}x{W}, pending bias {pre is not None}"
            w3 = torch.randn(3, cin, 3, 3, device=DEV) * 0.05
            y = _lib.conv3x3_gn_small(xx, w3.permute(0, 2, 3, 1).contiguous(), None, gn)
            gate(y, xin64, norm, w3, R.C_FP32, 1, "conv3x3_gn_small, " + tag)
            w32 = torch.randn(32, cin, 3, 3, device=DEV) * 0.05
            y = _lib.conv3x3_f32(xx, _lib.conv_f32_weights(w32), 32, gn=gn)
            gate(y, xin64, norm, w32, R.C_FP32, 1, "conv3x3_f32(gn), " + tag)
            conv = torch.nn.Conv2d(cin, 128, 3, 1, 1).to(DEV)
            wf, us = _lib.conv3_weights_f16(conv.weight)
            y = _lib.conv3x3_direct(xx, wf, us, U._gn_act_bound(norm, xx), gn=gn)
            gate(y, xin64, norm, conv.weight, R.C_F16X3, 1, "conv3x3_direct(gn), " + tag)
            for f4 in (False, True):
                y = _lib.wino_conv3x3(xx, U._wino_weights(conv, f4), gn=gn)
                gate(y, xin64, norm, conv.weight, R.C_WINO_F4 if f4 else R.C_WINO_F2, 1,
                     f"Winograd F({4 if f4 else 2},3) fused GroupNorm, " + tag)


# ------------------------------------------------------------------------------------------ modules on flat inputs
STATS_SWITCHES = ["FUSED_GN", "FUSED_ADD_STATS", "FUSED_WINO_GN", "CONV_IN_SMALL"]


def _runs():
    """(tag, switches off, layout): NCHW, channels_last, then channels_last with each statistics-related switch off."""
    cl = torch.channels_last
    return ([("NCHW", {}, torch.contiguous_format), ("channels_last", {}, cl)]
            + [(f"channels_last, {s} off", {s: False}, cl) for s in STATS_SWITCHES])


def _flat_images():
    """[6, 3, 256, 256] in [-1, 1]: constant -1, +1, 0.25, -0.6; letterboxed (content in the middle 50 %); low contrast."""
    g = torch.Generator().manual_seed(31)
    imgs = [torch.full((3, 256, 256), v) for v in (-1.0, 1.0, 0.25, -0.6)]
    lb = torch.full((3, 256, 256), -1.0)
    lb[:, 64:192, 64:192] = torch.rand(3, 128, 128, generator=g) * 2 - 1
    imgs += [lb, 0.4 + 1e-3 * torch.randn(3, 256, 256, generator=g)]
    return torch.stack(imgs)


@pytest.mark.parametrize("weights", ["default", "checkpoint-like"])
def test_encoder_on_flat_images_meets_the_contract(weights):
    """The full-size Encoder (bench shape 256 x 256, batch 2) on constant, letterboxed and low-contrast images, both layouts, and
    channels_last with each statistics-related switch off: z against the fp64 twin under contract_z."""
    from ckpt_like import checkpoint_like_
    from pit_hip.modules import unet as U

    torch.manual_seed(1234)
    enc = U.Encoder(**FULL).eval()
    if weights != "default":
        checkpoint_like_(enc, 5)
    enc = enc.to(DEV)
    imgs = _flat_images().to(DEV)
    twin = R.twin64(enc)
    for i in range(0, imgs.shape[0], 2):
        x = imgs[i: i + 2].contiguous()
        with torch.no_grad():
            z64 = twin(R.d64(x))
            for tag, flags, fmt in _runs():
                with switch(**flags):
                    z = enc.to(memory_format=fmt)(x.contiguous(memory_format=fmt))
                R.contract_z(z, z64, f"encoder, {weights} weights, images {i}-{i + 1}, {tag}")


@pytest.mark.parametrize("weights", ["default", "checkpoint-like"])
def test_decoder_on_a_near_constant_latent_meets_the_contract(weights):
    """The full-size Decoder on z = c + 1e-3 noise (every level's activations offset-dominated), both layouts, and channels_last
    with each statistics-related switch off: the reconstruction against the fp64 twin under contract_x."""
    from ckpt_like import checkpoint_like_
    from pit_hip.modules import unet as U

    torch.manual_seed(1234)
    dec = U.Decoder(**FULL).eval()
    if weights != "default":
        checkpoint_like_(dec, 6)
    dec = dec.to(DEV)
    g = torch.Generator().manual_seed(41)
    z = (torch.tensor([0.5, -1.5])[:, None, None, None] + 1e-3 * torch.randn(2, 16, 32, 32, generator=g)).to(DEV)
    with torch.no_grad():
        x64 = R.twin64(dec)(R.d64(z))
        for tag, flags, fmt in _runs():
            with switch(**flags):
                xr = dec.to(memory_format=fmt)(z.contiguous(memory_format=fmt))
            R.contract_x(xr, x64, f"decoder, {weights} weights, near-constant z, {tag}")
