"""SD3-style conv encoder / decoder as ``torch.nn`` modules over libgqhip's conv-stack kernels.

Mirror of the reference's ``pit/modules/unet.py`` interface for the hot path:
``Encoder(**params)(x) -> [B, 2*z, H/8, W/8]`` (unet.py:317-436) and
``Decoder(**params)(z) -> [B, 3, H, W]`` (unet.py:439-587).  The module tree is
laid out so that ``state_dict()`` keys equal the reference's (``conv_in``,
``down.{i}.block.{j}.norm1`` ... ``up.{i}.upsample.conv``), so a reference
checkpoint's ``encoder.*`` / ``decoder.*`` tensors load unchanged.

Two execution paths.  A module left in NCHW runs ATen / MIOpen convolutions with libgqhip's fused GroupNorm and residual
kernels (the drop-in default).  A module converted with ``.to(memory_format=torch.channels_last)`` -- the bench
configuration -- runs every convolution but ``conv_in`` in libgqhip (direct fp16 x 3 implicit GEMMs, Winograd transforms
around fp16 GEMMs, fp32 matrix-core convolutions for the layers next to z) and is bit-reproducible run to run; which kernel
serves which layer: tests/golden/convstack_routes.json (the recorded call list of tools/convstack/route_trace.py; every 3x3
convolution's route is picked in ``_conv3x3``).  Training / autograd / CPU tensors always take the ATen ops.

Only what the shipped SD3-UNet configs use is built: ``attn_type`` "vanilla"
(single-head SDPA, unet.py:166-206) or "none"; ``temb_channels`` is always 0 on
this path (unet.py:342, :473) so the time-embedding projection is not created.
"""
from __future__ import annotations

import math
import os
import threading
from typing import Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib


# ---- switches: module-level, read at call time (tests, tools/convstack/route_trace.py and A/B timing turn them off one at a
# time).  Which library calls each setting leaves: tests/golden/convstack_routes.json.
GN_GROUPS = 32             # unet.py:54-57: every Normalize is GroupNorm(32, C, eps=1e-6); the groups of every statistics record left
# libgqhip's GroupNorm(+ swish) (gn_silu / gn_apply, either layout) and, on channels_last tensors, every own convolution below
# (_own_ok); off: ATen ops, except in the residual adds (_add) and the q | k | v projection (AttnBlock._own_qkv_ok)
FUSED_GN = True
DEFER_BIAS = True          # convolutions run bias-free; the consumer (next GroupNorm, residual add, kernel epilogue) folds the bias in
FUSED_ADD_STATS = True     # residual add (and attention proj_out tail) also leaves the next GroupNorm's statistics (channels_last)
STATS_ARENA = True         # the statistics records of a forward from one arena zeroed by one fill (not ~60 memset launches per step)
_MAX_STATS_ARENAS = 8      # ... one arena per (thread, stream) that ran the module, the least recently used one goes
# every inference forward of Encoder / Decoder on a HIP device checks its weight-derived caches against a content hash of the
# parameters (catches ``param.data`` writes, which bump no version counter); see _WeightGuard
WEIGHT_GUARD = os.environ.get("GQHIP_WEIGHT_GUARD", "1") != "0"   # (the env switch: A/B timing)
# marked 3x3 convolutions (mark_winograd: decoder and, with WINOGRAD_ENCODER, encoder) of >= WINOGRAD_MIN_CH channels that the
# direct kernel does not take: libgqhip's Winograd transforms around 16 (F(2x2,3x3)) or 36 (F(4x4,3x3)) GEMMs
WINOGRAD = True
WINOGRAD_MIN_CH = 128
WINOGRAD_F4 = True         # convolutions marked f4 (the decoder's), H % 4 == W % 4 == 0: F(4x4,3x3) on 6x6 tiles instead of F(2x2,3x3)
# in the encoder too (read when an Encoder is built): measured perturbation of z 4.2e-6 vs the CPU reference (direct MIOpen convs:
# 3.4e-6), no index change on the CPU golden nor on 16 384 rows against the direct-conv encoder (tools/encoder_winograd_check.py)
WINOGRAD_ENCODER = True
FUSED_WINO_TAIL = True     # Winograd output transform / direct-kernel epilogue + bias + residual + next GroupNorm's statistics: one pass
# The 16 / 36 Winograd GEMMs as ONE fp16 batched GEMM with fp32 accumulation whose K axis carries the three products of
# two-term fp16 splits of both operands (22-bit significands): measured error 2.5-2.9e-7 of sum|a||b| against 2.6-3.5e-7
# for hipBLASLt's fp32 GEMM (itself a split-bf16 emulation on gfx950), at 1.2x (128 channels) to 2.5x (512) its speed
# (tools/bmm_bf16x3.py).  False: the library's fp32 GEMM.
WINOGRAD_F16X3 = True
# the 256- / 512-channel Winograd GEMMs through libgqhip's wino_gemm_f16x2 on the [h | l] operand (weights in MFMA
# operand order, three products in the kernel) where its grid fills the chip (_lib.own_gemm_fits: everything but the
# 32 x 32 levels' 36 x 1024-tile GEMMs); else the library GEMM over [h | h | l]
WINOGRAD_OWN_GEMM = True
# GroupNorm+SiLU applied inside the Winograd input transforms (F(2x2,3x3) / F(4x4,3x3)): the normalised tensor is never written or
# re-read.  Bit-identical V to gn_apply + plain transform (same folded scale / shift, same silu_f32): 53.4 -> 50.8 ms / step.
FUSED_WINO_GN = True
FUSED_WINO_GN_F4 = True
# 3x3 convolutions into 128 channels (256 x 256 level) -- and, where the alternative is F(2x2,3x3) (the encoder), into 256
# channels (128 x 128 level) -- as a direct fp16 x 3 implicit GEMM instead of Winograd: reads the activation once and
# writes the result once where Winograd moves 6.4 / 10.7 GB of transformed tensors per convolution at 256 x 256
DIRECT_CONV = True
DIRECT_CONV_S2 = True      # Downsample (pad + 3x3 stride 2) as an fp16 x 3 convolution on the four phase images of x
DIRECT_CONV_1X1 = True     # 1x1 shortcut / proj_out / q | k | v convolutions as an fp16 x 3 GEMM, the split of x inside the kernel
# Upsample: nearest x2 + conv3x3 as four 2x2 phase convolutions of the low-resolution input (2.25x fewer flops), computed directly by
# libgqhip's upconv2x_f16x3 (one kernel); shapes it does not tile: NHWC upsample copy + the ordinary convolution routes
DIRECT_UPCONV = True
CONV_IN_SMALL = True       # the encoder's conv_in (3 -> 128) on libgqhip's fixed-order fp32 kernel (+ bias + statistics), not MIOpen
FUSED_CONV_OUT = True      # decoder conv_out (128 -> 3) with norm_out + swish fused in: one VALU kernel
# encoder conv_out (512 -> 2 z, norm_out + swish fused in) and decoder conv_in (z -> 512) on the fp32 matrix cores with a fixed
# summation order (bit-reproducible; MIOpen's pick for the former combines split-K partial sums with atomics)
CONV_F32 = True
FUSED_QKV = True           # q, k, v as one GEMM with fused biases (channels_last): libgqhip's 1x1 kernel at 512 channels, else addmm
ATTN_FUSED_PROJ = True     # GroupNorm inside the q | k | v projection's staging, the GEMM operands written by its epilogue
ATTN_F16X3 = True          # both attention GEMMs as fp16 x 3 library GEMMs (split of q, k, v and softmax + split: libgqhip kernels)
ATTN_MATH = "auto"         # explicit matmul/softmax/matmul instead of the fused SDPA kernel: "auto" = on HIP devices


def _gn(ch: int) -> nn.GroupNorm:
    # unet.py:54-57
    return nn.GroupNorm(32, ch, eps=1e-6, affine=True)


def _infer_ok(x: torch.Tensor) -> bool:
    """Inference on a HIP device, fp32, 4-D: what every libgqhip route asks of its input.  (Whatever FUSED_GN says: _own_ok
    adds that switch and the layout; _add and AttnBlock._own_qkv_ok deliberately ask this much only.)"""
    return x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.dim() == 4


def _nhwc(x: torch.Tensor) -> bool:
    """Dense channels_last (and not NCHW-contiguous as well)."""
    return _lib.image_layout(x) == 1


def _own_ok(x: torch.Tensor) -> bool:
    """libgqhip's own convolutions apply: FUSED_GN, inference on a HIP device, fp32, 4-D, dense channels_last."""
    return FUSED_GN and _infer_ok(x) and _nhwc(x)


def _plain3x3(conv: nn.Module) -> bool:
    """A Conv2d with kernel 3x3, stride 1, padding 1, dilation 1, groups 1 and zero padding."""
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros")


# ---- what a producer leaves on its output for the consumer: tensor attributes (ResnetBlock / AttnBlock return plain tensors; an
# attribute does not follow a view or a copy, so its carrier is the very tensor the producer wrote).  Only these four touch them.
def _leave_stats(y: torch.Tensor, records, groups: int, pre_bias=None, memo: bool = False) -> torch.Tensor:
    """Tag y with the GroupNorm statistics records (``groups`` groups) its producer computed with it; returns y.  ``memo``: the
    records were computed afterwards, for y + ``pre_bias`` (this very object, or None) -- kept apart from the producer's."""
    if memo:
        y._gn_stats_pb = (records, groups, pre_bias)
    else:
        y._gn_stats = (records, groups)
    return y


def _left_stats(x: torch.Tensor, groups: int, pre_bias=None, memo: bool = False):
    """The statistics records the producer of x left, or None.  They serve only a GroupNorm of the same ``groups``, with no bias
    pending on x, and x dense channels_last (the only layout the records' consumers take).  ``memo``: failing that, the
    records memoised for x + this very ``pre_bias`` object."""
    st = getattr(x, "_gn_stats", None)
    if st is not None and pre_bias is None and st[1] == groups and _nhwc(x):
        return st[0]
    st = getattr(x, "_gn_stats_pb", None) if memo else None
    return st[0] if st is not None and st[1] == groups and st[2] is pre_bias else None


def _leave_bound(y: torch.Tensor, bound: float) -> None:
    y._act_bound = bound   # a rigorous bound on |y| for y = swish(GroupNorm(.)) (_gn_act_bound); _left_bound: that, or None


def _left_bound(x: torch.Tensor):
    return getattr(x, "_act_bound", None)


def _tagged(out):
    """A library call's (y, statistics records of y in GN_GROUPS groups) as the modules' (y, pending_bias): y tagged, no bias."""
    return _leave_stats(*out, GN_GROUPS), None


def _stats_of(x: torch.Tensor, pre_bias, groups: int):
    """GroupNorm statistics of x + pre_bias: left by the producer of x, computed earlier for the same pending bias, or
    computed (and remembered on x) here."""
    stats = _left_stats(x, groups, pre_bias, memo=True)
    if stats is None:
        stats = _lib.gn_stats(x, groups, pre_bias)
        _leave_stats(x, stats, groups, pre_bias, memo=True)
    return stats


def _gn_tuple(norm: nn.GroupNorm, x: torch.Tensor, pre_bias, silu: bool = True) -> _lib.GnFold:
    """The ``gn`` argument of the kernels that apply ``norm`` (+ swish) while they stage x + pre_bias (statistics: _stats_of)."""
    return _lib.GnFold(norm.weight, norm.bias, norm.num_groups, norm.eps, silu, _stats_of(x, pre_bias, norm.num_groups), pre_bias)


def _use_fused(x: torch.Tensor, norm: nn.GroupNorm) -> bool:
    """HIP fused GroupNorm(+SiLU) applies to inference on HIP devices, NCHW fp32, HW % 4 == 0;
    training / autograd / CPU tensors stay on the ATen ops (this stack is PyTorch by design)."""
    if not (FUSED_GN and _infer_ok(x) and norm.affine):
        return False
    layout = _lib.image_layout(x)
    if layout == 0:
        return (x.shape[2] * x.shape[3]) % 4 == 0
    return layout == 1 and _lib.gn_nhwc_ok(x.shape[1], norm.num_groups)


def _materialize(x: torch.Tensor, pre_bias) -> torch.Tensor:
    return x if pre_bias is None else x + pre_bias[None, :, None, None]


def _norm_act(norm: nn.GroupNorm, x: torch.Tensor, act: bool = True, pre_bias=None) -> torch.Tensor:
    """GroupNorm followed by swish (unet.py:140-141, :146-147, :432-433) -- one fused HIP pass pair.
    ``pre_bias``: per-channel bias still pending on ``x`` (see ``_conv3x3``)."""
    if _use_fused(x, norm):
        stats = _left_stats(x, norm.num_groups, pre_bias)   # of the producer (e.g. _add); never the memo of _stats_of
        if stats is not None:
            y = _lib.gn_apply(x, norm.weight, norm.bias, norm.num_groups, norm.eps, act, stats)
        else:
            y = _lib.gn_silu(x, norm.weight, norm.bias, norm.num_groups, norm.eps, silu=act, pre_bias=pre_bias)
        if WINOGRAD_F16X3:
            _leave_bound(y, _gn_act_bound(norm, x))   # lets the Winograd GEMMs that consume y run as fp16 x 3 (see _f16_args)
        return y
    y = norm(_materialize(x, pre_bias))
    return F.silu(y) if act else y   # unet.py:49-51 (x * sigmoid(x)): the same function, one kernel


def _defer_ok(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """Deferred-bias path: inference on HIP, fp32, zero padding."""
    return FUSED_GN and DEFER_BIAS and _infer_ok(x) and conv.bias is not None and conv.padding_mode == "zeros"


def _f16_args(conv: nn.Conv2d, x: torch.Tensor, f4: bool, norm=None):
    """The ``f16`` argument of _lib.wino_conv3x3's fp16 x 3 route, or None.  The route needs a rigorous bound on the tensor the
    input transform sees: with ``norm`` (GroupNorm + swish run inside the transform, the activated tensor is never materialised)
    it is computed here, else it is the one _norm_act left on x (there only when it ran with WINOGRAD_F16X3 set)."""
    bound = None if not WINOGRAD_F16X3 else _left_bound(x) if norm is None else _gn_act_bound(norm, x)
    if bound is None or not _lib.bmm_out_dtype_ok(x.device):   # (bmm(out_dtype=fp32): recent PyTorch-ROCm, probed once)
        return None
    u3, u_scale, wf2 = _wino_weights_f16(conv, f4)
    return _lib.F16Gemm(u3, u_scale, bound, wf2 if WINOGRAD_OWN_GEMM else None)


def _conv3x3(conv: nn.Conv2d, x: torch.Tensor, norm=None, pre_bias=None, residual=None, residual_bias=None,
             want_stats: bool = False):
    """[residual + residual_bias +] conv(swish(norm(x + pre_bias))) -> (y, pending_bias): the one place that picks a
    convolution's route.  ATen's MIOpen path adds the bias in a separate elementwise pass over the whole output; on the
    deferred path the conv runs bias-free and the bias is handed to the consumer (the next fused GroupNorm or residual add),
    which folds it in.
    Input: libgqhip's direct fp16 x 3 kernel and the Winograd input transforms (FUSED_WINO_GN / FUSED_WINO_GN_F4) apply
    ``norm`` + swish while they stage x, so the normalised tensor is never written; where neither takes the layer it is
    materialised by ``_norm_act`` and the route is picked for that tensor: Winograd (fp16 x 3 or fp32 GEMMs) or the library.
    Tail: with ``want_stats`` (the consumer is a GroupNorm(32)) or a ``residual`` (conv2 of a ResnetBlock) the kernel's
    epilogue adds the bias (+ residual + residual_bias) and leaves the next GroupNorm's statistics with the output; a
    residual it cannot take is added by ``_add``.  ``norm`` None runs any convolution (1x1, stride 2): only marked 3x3
    stride-1 ones leave the library."""
    cout = conv.out_channels
    fuse_in = norm is not None and _defer_ok(x, conv) and _use_fused(x, norm)
    tail = FUSED_WINO_TAIL and (want_stats or residual is not None) and _lib.gn_nhwc_ok(cout, GN_GROUPS)
    if residual is not None:
        # the fused conv2 tail exists only with norm2 handled here, and is gated on _wino_ok for the direct kernel too
        if not (tail and fuse_in and _wino_ok(conv, x) and residual.shape[1] == cout and _nhwc(residual)):
            h, bias = _conv3x3(conv, x if norm is None else _norm_act(norm, x, pre_bias=pre_bias))
            if residual_bias is not None:
                bias = residual_bias if bias is None else bias + residual_bias
            return _add(residual, h, bias), None
    f4 = WINOGRAD_F4 and getattr(conv, "_gq_wino4", False) and x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0
    direct = fuse_in and _direct_ok(conv, x)    # (conv1 takes the direct kernel whatever _wino_ok says)
    if norm is not None and not direct and not (fuse_in and _wino_ok(conv, x) and (FUSED_WINO_GN_F4 if f4 else FUSED_WINO_GN)):
        x, norm = _norm_act(norm, x, pre_bias=pre_bias), None
    if norm is None and residual is None:       # (a fused residual tail has passed both tests on the tensor norm2 read)
        if not _defer_ok(x, conv):
            return conv(x), None
        if not _wino_ok(conv, x):
            return F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups), conv.bias
    epilogue = {}
    if tail:
        epilogue = dict(residual=residual, bias=conv.bias if residual_bias is None else conv.bias + residual_bias,
                        stats_groups=GN_GROUPS)
    if direct:
        wf, us = _direct_weights(conv)
        out = _lib.conv3x3_direct(x, wf, us, _gn_act_bound(norm, x), gn=_gn_tuple(norm, x, pre_bias), **epilogue)
    else:
        gn = None if norm is None else _gn_tuple(norm, x, pre_bias)
        out = _lib.wino_conv3x3(x, _wino_weights(conv, f4), gn=gn, f16=_f16_args(conv, x, f4, norm), **epilogue)
    return _tagged(out) if tail else (out, conv.bias)


def _match_layout(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """A module converted with ``.to(memory_format=torch.channels_last)`` gets its input in NHWC too (the fast conv
    stack -- Winograd, sub-pixel upsample, NHWC GroupNorm kernels -- is the channels_last one)."""
    if x.is_cuda and x.dim() == 4 and _nhwc(conv.weight) and not x.is_contiguous(memory_format=torch.channels_last):
        return x.contiguous(memory_format=torch.channels_last)
    return x


# ---- route predicates, one per libgqhip route: the switch, what the module layer adds (markers, biases, layouts) and exactly the
# divisibility the route's _lib wrapper enforces (_pointwise_ok excepted: see there); _wino_ok / _direct_ok are combined in _conv3x3
def _wino_ok(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """_lib.wino_conv3x3: a marked convolution of >= WINOGRAD_MIN_CH channels, Cout % 4, even H and W, channels_last."""
    return (WINOGRAD and getattr(conv, "_gq_wino", False) and min(conv.in_channels, conv.out_channels) >= WINOGRAD_MIN_CH
            and conv.out_channels % 4 == 0 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and _nhwc(x))


def _direct_ok(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """3x3 stride-1 padding-1 convolutions of the widest levels run as libgqhip's direct fp16 x 3 convolution: into 128
    channels (the 256 x 256 level), where every Winograd route is HBM-bound on its transformed tensors, and -- for modules
    marked F(2x2,3x3)-only (the encoder) -- into 256 channels too (gq_conv3.h)."""
    if not (DIRECT_CONV and getattr(conv, "_gq_wino", False) and conv.in_channels % 16 == 0 and x.shape[2] % 8 == 0
            and x.shape[3] % 32 == 0 and _nhwc(x)):
        return False
    if conv.out_channels == 128:
        return True
    # 256 output channels only where F(4x4,3x3) would not be used
    return conv.out_channels == 256 and not (WINOGRAD_F4 and getattr(conv, "_gq_wino4", False))


def _pointwise_ok(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """1x1 convolutions into 128 / 256 / 512 channels (ResnetBlock shortcuts, attention proj_out) as libgqhip's fp16 x 3
    GEMM over the pixels (gq_conv3.h: conv1x1_f16x3) instead of MIOpen's fp32 implicit GEMM (~100 TFLOP/s)."""
    # (HW % 256 and Cin % 128 are asked here although the library takes HW % 128 and Cin % 32)
    return (DIRECT_CONV_1X1 and _own_ok(x) and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.out_channels in (128, 256, 512)
            and conv.in_channels % 128 == 0 and (x.shape[2] * x.shape[3]) % 256 == 0)


def _proj_tail_ok(conv: nn.Conv2d, x: torch.Tensor, a: torch.Tensor) -> bool:
    """_lib.conv1x1_direct with its tail for the attention block: x + conv(a) + bias and the next GroupNorm's statistics."""
    return (_pointwise_ok(conv, a) and FUSED_ADD_STATS and _nhwc(x) and conv.bias is not None
            and _lib.gn_nhwc_ok(x.shape[1], GN_GROUPS))


def _stride2_ok(conv: nn.Conv2d, x: torch.Tensor, mode: str) -> bool:
    """_lib.conv3x3s2_direct for Downsample's convolution (always 3x3, stride 2, padding 0) behind a zero pad; needs the bias."""
    return (DIRECT_CONV_S2 and mode == "constant" and _own_ok(x) and conv.out_channels in (128, 256, 512)
            and conv.in_channels % 16 == 0 and conv.bias is not None and x.shape[2] % 16 == 0 and x.shape[3] % 64 == 0
            and _lib.gn_nhwc_ok(x.shape[1], GN_GROUPS) and _lib.gn_nhwc_ok(conv.out_channels, GN_GROUPS))


def _upconv_ok(up: "Upsample", x: torch.Tensor) -> bool:
    """_lib.upconv2x_direct for Upsample with a deferrable bias (the caller adds: statistics left by the producer of x)."""
    return (DIRECT_UPCONV and DEFER_BIAS and up.with_conv and _own_ok(x) and _plain3x3(up.conv) and up.conv.bias is not None
            and up.conv.out_channels in (128, 256, 512) and x.shape[1] % 16 == 0 and x.shape[2] % 8 == 0
            and x.shape[3] % 32 == 0 and _lib.gn_nhwc_ok(up.conv.out_channels, GN_GROUPS))


def _conv_f32_ok(conv: nn.Conv2d, x: torch.Tensor, gn: bool) -> bool:
    """_lib.conv3x3_f32 for the narrow ends of the stack (encoder conv_out with ``gn``, decoder conv_in without): a fixed
    summation order, hence bit-reproducible -- MIOpen's pick for 512 -> 32 channels is a split-K kernel with atomics."""
    return (CONV_F32 and _own_ok(x) and _plain3x3(conv)
            and _lib.conv_f32_ok(conv.in_channels, conv.out_channels, x.shape[2], x.shape[3], gn))


def _direct_weights(conv: nn.Conv2d):
    """(Wf, u_scale) of conv3x3_direct / conv1x1_direct, cached until the weight changes."""
    return _cached(conv, "direct_wf", _wkey(conv.weight), lambda: _lib.conv3_weights_f16(conv.weight))


def _norm_act_conv_small(norm: nn.GroupNorm, conv: nn.Conv2d, x: torch.Tensor, pre_bias=None) -> torch.Tensor:
    """conv(swish(norm(x + pre_bias))) for a 3x3 convolution into <= 4 channels (the decoder's conv_out, unet.py:585-587):
    one libgqhip kernel -- GroupNorm + swish applied while staging, fp32 FMAs -- instead of a normalisation pass and
    MIOpen's implicit GEMM (0.2 + 0.96 ms at 16 x 256 x 256 x 128)."""
    if (FUSED_CONV_OUT and _own_ok(x) and _use_fused(x, norm) and _plain3x3(conv) and conv.out_channels <= 4
            and x.shape[1] % 32 == 0 and x.shape[1] <= 512 and x.shape[2] % 16 == 0 and x.shape[3] % 16 == 0):
        ohwi = _cached(conv, "ohwi", _wkey(conv.weight), lambda: conv.weight.detach().permute(0, 2, 3, 1).contiguous())
        return _lib.conv3x3_gn_small(x, ohwi, conv.bias, _gn_tuple(norm, x, pre_bias))
    return conv(_norm_act(norm, x, pre_bias=pre_bias))


def _wkey(*params):
    return tuple((p.data_ptr(), p._version, p.device) for p in params)


def _cached(module: nn.Module, name: str, key, build):
    """Weight-derived data of ``module`` (operand-order copies, fp16 splits, bounds): one dict per module, entries keyed on
    the parameters' (data_ptr, _version, device), dropped together by ``invalidate_caches``."""
    cache = module.__dict__.setdefault("_gq_cache", {})
    ent = cache.get(name)
    if ent is None or ent[0] != key:
        ent = (key, build())
        cache[name] = ent
    return ent[1]


def _conv_f32(conv: nn.Conv2d, x: torch.Tensor, gn=None) -> torch.Tensor:
    wk = _cached(conv, "f32_wk", _wkey(conv.weight), lambda: _lib.conv_f32_weights(conv.weight))
    return _lib.conv3x3_f32(x, wk, conv.out_channels, bias=conv.bias, gn=gn)


def _conv_in_small(conv: nn.Conv2d, x: torch.Tensor):
    """The encoder's conv_in (unet.py:411-413, 3 -> 128 channels) -> (y, pending_bias).  On the channels_last path: libgqhip's
    fixed-order fp32 kernel with the bias and the first GroupNorm's statistics in its epilogue (MIOpen: 0.24 ms per call once
    its CK solver runs, 4 ms for each of a process's first eight calls).  Other shapes / layouts: ``_conv3x3``."""
    if (CONV_IN_SMALL and _own_ok(x) and _plain3x3(conv) and GN_GROUPS == 32   # (the kernel's statistics epilogue: 32 groups)
            and _lib.conv_cin_small_ok(conv.in_channels, conv.out_channels, x.shape[2], x.shape[3])):
        wk = _cached(conv, "cin_small_wk", _wkey(conv.weight), lambda: _lib.conv_cin_small_weights(conv.weight))
        return _tagged(_lib.conv3x3_cin_small(x, wk, conv.bias, stats_groups=GN_GROUPS))
    return _conv3x3(conv, x)


def _norm_act_conv_f32(norm: nn.GroupNorm, conv: nn.Conv2d, x: torch.Tensor, pre_bias=None) -> torch.Tensor:
    """conv(swish(norm(x + pre_bias))) for the encoder's conv_out (unet.py:432-436): GroupNorm + swish applied while the
    patch is staged, fp32 matrix cores, fixed summation order."""
    if _conv_f32_ok(conv, x, True) and _use_fused(x, norm):   # (_conv_f32_ok: channels_last)
        return _conv_f32(conv, x, gn=_gn_tuple(norm, x, pre_bias))
    return conv(_norm_act(norm, x, pre_bias=pre_bias))


_WINO_G2 = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
_WINO_G4 = [[1 / 4, 0.0, 0.0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
            [1 / 24, -1 / 12, 1 / 6], [0.0, 0.0, 1.0]]


def _wino_weights(conv: nn.Conv2d, f4: bool = False) -> torch.Tensor:
    """U = G g G^T of a 3x3 kernel, [16, Cin, Cout] for F(2x2,3x3) or [36, Cin, Cout] for F(4x4,3x3) (formed in
    fp64, rounded once); cached until the weight changes."""
    def build():
        w = conv.weight
        G = torch.tensor(_WINO_G4 if f4 else _WINO_G2, dtype=torch.float64, device=w.device)
        u = torch.einsum("ik,ockl,jl->ijco", G, w.double(), G).float()
        return u.reshape(-1, w.shape[1], w.shape[0]).contiguous()

    return _cached(conv, "wino_u", _wkey(conv.weight) + (f4,), build)


def _wino_weights_f16(conv: nn.Conv2d, f4: bool = False):
    """(U3, u_scale, Wf2): U = G g G^T scaled by a power of two into fp16's comfortable range and split into two fp16 terms,
    stacked along K as [U_h; U_l; U_h] ([T, 3 Cin, Cout] fp16) -- the weight side of the f16x3 GEMM (gqhip.h:
    wino_in_nhwc_f16x3) -- and, where libgqhip's own GEMM applies (Cin % 32 == 0, Cout % 128 == 0), (U_h, U_l) in MFMA operand
    order for wino_gemm_f16x2 (the [h | l] route).  Cached like (and keyed like) the fp32 U."""
    def build():
        h, l, u_scale = _lib._split_f16(_wino_weights(conv, f4))
        own = WINOGRAD_OWN_GEMM and h.shape[1] % 32 == 0 and h.shape[2] % 128 == 0
        return torch.cat([h, l, h], 1).contiguous(), u_scale, (_lib.wino_weights_operand_order(h, l) if own else None)

    return _cached(conv, "wino_u3", _wkey(conv.weight) + (f4, WINOGRAD_OWN_GEMM), build)


def _gn_act_bound(norm: nn.GroupNorm, x: torch.Tensor) -> float:
    """A rigorous bound on |SiLU(GroupNorm(x))|: a group of n elements has |(x - mean) / sqrt(var + eps)| <= sqrt(n - 1),
    so |y| <= sqrt(n - 1) max|gamma| + max|beta| and |SiLU(y)| <= |y|.  (max|gamma|, max|beta| cached per weight.)"""
    gb = _cached(norm, "gb_max", _wkey(norm.weight, norm.bias),
                 lambda: (float(norm.weight.detach().abs().max()), float(norm.bias.detach().abs().max())))
    n = (x.shape[1] // norm.num_groups) * x.shape[2] * x.shape[3]
    return math.sqrt(max(n - 1, 1)) * gb[0] + gb[1]


class _WeightGuard:
    """Notices parameter writes that bump no version counter (``param.data.mul_()``, EMA swaps through ``.data``): the
    weight-derived caches below are keyed on (data_ptr, _version), which such writes leave unchanged.  One libgqhip launch per
    forward hashes the bytes of every parameter of the module (gqhip.h:gqhip_checksum_tensors, ~0.1-0.2 GB read); the forward
    runs speculatively on the cached data while the sums travel to pinned host memory; before the result is returned they are
    compared with the sums the caches were built from, and on a difference the caches are dropped and the forward runs again.
    The wait is for a copy queued at the START of this forward, so the host stays at most one forward ahead of the device
    and the device never idles."""

    def __init__(self) -> None:
        self.key = None

    def begin(self, module: nn.Module) -> bool:
        params = [p for p in module.parameters()]
        # the checksum kernel reads numel() words from data_ptr(): only DENSE parameters (contiguous, or a dense channels_last
        # layout) -- an expanded or strided view would be read past its own storage, so such a module runs unguarded
        dense = lambda p: p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))
        if not params or not all(p.is_cuda and p.dtype == torch.float32 and dense(p) for p in params):
            return False
        key = tuple(p.data_ptr() for p in params)
        if key != self.key:
            try:
                self.table = _lib.checksum_table([p.detach() for p in params])
            except _lib.GqHipError:
                return False
            self.sums = torch.empty(len(params), dtype=torch.int64, device=params[0].device)
            self.host = torch.empty(len(params), dtype=torch.int64).pin_memory()
            self.event = torch.cuda.Event()
            self.baseline = None
            self.key = key
        self.versions = tuple(p._version for p in params)
        _lib.checksum_tensors(self.table, self.sums)
        self.host.copy_(self.sums, non_blocking=True)
        self.event.record()
        return True

    def changed(self) -> bool:
        """True when some parameter's bytes changed WITHOUT its version counter moving (the only case the caches cannot see by
        themselves: an update that bumps ``_version`` -- load_state_dict, an optimizer step -- already changed the cache keys, so the
        speculative run rebuilt what it needed and is not repeated)."""
        self.event.synchronize()
        cur = self.host.clone()
        base, base_v = self.baseline, getattr(self, "baseline_versions", None)
        self.baseline, self.baseline_versions = cur, self.versions
        if base is None or torch.equal(cur, base):
            return False
        moved = (cur != base).tolist()
        return any(m and v == bv for m, v, bv in zip(moved, self.versions, base_v))


def _with_stats_arena(module: nn.Module, run, x: torch.Tensor):
    """run(x) with every GroupNorm statistics record of the forward carved out of an arena of the module (one fill per forward
    instead of one small memset launch per producing kernel: _lib.StatsArena).  One arena per (thread, stream): the buffer is
    re-zeroed and reused in stream order, so two streams (or threads) running the same module must not share it.  Never under a
    graph capture: a captured graph would bake in the arena's address, and a later eager forward with a bigger batch reallocates
    the buffer -- the replay would then zero and accumulate into memory the allocator may have handed to someone else; captured
    forwards take per-call records from the caching allocator, which the capture keeps alive."""
    if not (STATS_ARENA and FUSED_GN and x.is_cuda and not torch.is_grad_enabled()) or torch.cuda.is_current_stream_capturing():
        return run(x)
    key = (threading.get_ident(), torch.cuda.current_stream(x.device).cuda_stream)
    arenas = module.__dict__.setdefault("_gq_stats_arenas", {})
    arena = arenas.pop(key, None)
    if arena is None:
        arena = _lib.StatsArena()
        module.__dict__.setdefault("_gq_stats_arena", arena)      # (the first one: what tests / tools look at)
        # bounded: workloads that churn threads or streams would otherwise keep one device arena per (thread, stream)
        # they ever used; the least recently used one goes (dicts keep insertion order; a hit re-inserts below).  The device
        # memory of an evicted arena is released stream-ordered by the caching allocator, so a forward still in flight on it is safe.
        while len(arenas) >= _MAX_STATS_ARENAS:
            arenas.pop(next(iter(arenas)))
    arenas[key] = arena
    with _lib.stats_arena(arena, x.device):
        return run(x)


def _guarded(module: nn.Module, run0, x: torch.Tensor):
    """run(x) with the module's weight caches verified against the parameters' bytes (see _WeightGuard).  Costs one host wait per
    forward (for a copy queued at the forward's start: the host stays at most one module ahead of the device).  A caller that
    never writes parameters through ``.data`` and wants a fully asynchronous forward opts out per module:
    ``encoder.weight_guard = False`` (or process-wide: GQHIP_WEIGHT_GUARD=0)."""
    run = lambda t: _with_stats_arena(module, run0, t)
    if not (WEIGHT_GUARD and getattr(module, "weight_guard", True) and x.is_cuda and not torch.is_grad_enabled()
            and not torch.cuda.is_current_stream_capturing()):
        return run(x)
    guard = module.__dict__.get("_gq_guard")
    if guard is None:
        guard = module.__dict__["_gq_guard"] = _WeightGuard()
    if not guard.begin(module):
        return run(x)
    y = run(x)
    if guard.changed():
        invalidate_caches(module)
        y = run(x)
    return y


def invalidate_caches(module: nn.Module) -> None:
    """Drop every weight-derived cache under ``module`` (Winograd U matrices, operand-order fp16 splits, the sub-pixel phase
    matrices, the fused q/k/v matrix, operand bounds): every one of them lives in the owning module's ``_gq_cache`` dict
    (see ``_cached``), keyed on the parameters' (data_ptr, _version, device) -- which follows ``load_state_dict``, optimizer
    steps, ``.to()`` and any in-place op on the parameter.  Writes through ``param.data`` bump no version counter: those are
    caught by the content-hash guard of every inference forward (``_WeightGuard``), which calls this function itself, so
    nobody has to remember to."""
    for m in module.modules():
        m.__dict__.pop("_gq_cache", None)


def _drop_caches_after_load(module, incompatible_keys) -> None:
    invalidate_caches(module)


def mark_winograd(module: nn.Module, f4: bool = False) -> None:
    """Flag the stride-1, padding-1 3x3 convolutions of ``module`` for the Winograd path (see ``_conv3x3``);
    ``f4``: F(4x4,3x3) where the spatial size allows it (decoder only: larger rounding error)."""
    for m in module.modules():
        if _plain3x3(m):
            m._gq_wino = True
            m._gq_wino4 = f4


def _add(a: torch.Tensor, b: torch.Tensor, bias=None) -> torch.Tensor:
    """a + b (+ bias[c]) -- the residual add with the pending biases folded in."""
    if bias is not None and _infer_ok(a) and a.shape == b.shape:    # (whatever FUSED_GN says)
        la, lb = _lib.image_layout(a), _lib.image_layout(b)
        if FUSED_ADD_STATS and la == 1 and lb == 1 and _lib.gn_nhwc_ok(a.shape[1], GN_GROUPS):
            # every residual add of this UNet feeds a GroupNorm(32): leave its statistics with the sum, the
            # consumer (_norm_act) then skips its own statistics pass over the tensor
            return _leave_stats(*_lib.add_bias_stats(a, b, bias, GN_GROUPS), GN_GROUPS)
        if la is not None and la == lb and ((la == 0 and (a.shape[2] * a.shape[3]) % 4 == 0) or
                                            (la == 1 and a.shape[1] % 4 == 0)):
            return _lib.add_bias(a, b, bias)
    return _materialize(a + b, bias)


def _sdpa(q, k, v):
    # single head, head_dim = C = 512, fp32: two hipBLASLt GEMMs + a softmax beat the fused attn_fwd kernel
    # (3.3 -> 1.9 ms per step at bs 16; A/B-timed, +2 % end to end); same function, fp32 rounding-level differences
    if ATTN_MATH is True or (ATTN_MATH == "auto" and q.is_cuda):
        w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * (q.shape[-1] ** -0.5), dim=-1)
        return torch.matmul(w, v)
    return F.scaled_dot_product_attention(q, k, v)  # scale c**-0.5


def _conv3(cin: int, cout: int, padding_mode: str = "zeros", stride: int = 1, padding: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, 3, stride, padding, padding_mode=padding_mode)


class ResnetBlock(nn.Module):
    """GN -> swish -> conv3 -> GN -> swish -> conv3 (+ 1x1 shortcut); unet.py:100-153."""

    def __init__(self, cin: int, cout: int, dropout: float = 0.0, padding_mode: str = "zeros") -> None:
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.norm1 = _gn(cin)
        self.conv1 = _conv3(cin, cout, padding_mode)
        self.norm2 = _gn(cout)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = _conv3(cout, cout, padding_mode)
        if cin != cout:
            self.nin_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x: torch.Tensor, pre_bias=None) -> torch.Tensor:
        """``pre_bias``: bias of the conv that produced ``x``, not yet added (deferred path)."""
        h, b1 = _conv3x3(self.conv1, x, self.norm1, pre_bias, want_stats=True)   # norm2 follows
        xs, bs = self._shortcut(x, pre_bias)
        if self.dropout.p > 0.0 and self.training:   # active dropout: norm2 is materialised, which leaves conv2's tail unfused
            return _conv3x3(self.conv2, self.dropout(_norm_act(self.norm2, h, pre_bias=b1)), residual=xs, residual_bias=bs)[0]
        # dropout is the identity (unet.py:148 with p = 0 / eval)
        return _conv3x3(self.conv2, h, self.norm2, b1, residual=xs, residual_bias=bs)[0]

    def _shortcut(self, x: torch.Tensor, pre_bias):
        """(xs, bs) with xs + bs = nin_shortcut(x + pre_bias), or x + pre_bias where the width does not change."""
        if self.in_channels == self.out_channels:
            return x, pre_bias
        nin = self.nin_shortcut
        if _pointwise_ok(nin, x) and _use_fused(x, self.norm1):
            # nin(x + pb) as one fp16 x 3 GEMM over the pixels; x + pb is split inside the kernel, its power-of-two scale
            # comes (on the device) from the statistics norm1 needed anyway: |x + pb| <= sqrt(group sum of squares)
            wf, us = _direct_weights(nin)
            scales = _lib.f16_scales(_stats_of(x, pre_bias, GN_GROUPS), 1.0, us)
            return _lib.conv1x1_direct(x, wf, us, scales, pre_bias=pre_bias), nin.bias
        # nin(x + pb) = nin_nobias(x) + W.pb + nin.bias : every constant goes into the fused add
        xs, bs = _conv3x3(nin, x)
        if pre_bias is not None:
            wpb = nin.weight.reshape(self.out_channels, self.in_channels) @ pre_bias
            bs = wpb if bs is None else bs + wpb
        return xs, bs


class AttnBlock(nn.Module):
    """Single-head self attention over the h*w positions; unet.py:166-206."""

    def __init__(self, ch: int) -> None:
        super().__init__()
        self.norm = _gn(ch)
        self.q = nn.Conv2d(ch, ch, 1)
        self.k = nn.Conv2d(ch, ch, 1)
        self.v = nn.Conv2d(ch, ch, 1)
        self.proj_out = nn.Conv2d(ch, ch, 1)

    def _qkv_weights(self):
        """([c, 3c] GEMM matrix, [3c] bias) of the q / k / v 1x1 convolutions; cached until a weight changes."""
        ps = (self.q.weight, self.k.weight, self.v.weight, self.q.bias, self.k.bias, self.v.bias)

        def build():
            c = self.q.weight.shape[0]
            return (torch.cat([p.detach().reshape(c, c) for p in ps[:3]], 0).t().contiguous(),
                    torch.cat([p.detach() for p in ps[3:]], 0).contiguous())

        return _cached(self, "qkv", _wkey(*ps), build)

    def _qkv_weights_f16(self):
        """(qkv_wf, qkv_us): that matrix as the weight operand of libgqhip's fp16 x 3 GEMM over the pixels; cached likewise."""
        def build():
            wqkv = self._qkv_weights()[0]
            return _lib.conv3_weights_f16(wqkv.t().reshape(wqkv.shape[1], wqkv.shape[0], 1, 1))

        return _cached(self, "qkv_wf", _wkey(self.q.weight, self.k.weight, self.v.weight), build)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        b, c, h, w = x.shape
        fused = self._fused_proj_attention(x) if ATTN_FUSED_PROJ else None
        if fused is not None:
            a, a_scale = fused[0].reshape(b, h, w, c).permute(0, 3, 1, 2), fused[1]
        else:
            a, a_scale = self._attention(x)
        return self._proj_out(x, a, a_scale)

    def _attention(self, x: torch.Tensor):
        """(attention output [b, c, h, w], power of two still pending on it) of norm -> q, k, v -> softmax(q k^T) v."""
        b, c, h, w = x.shape
        a_scale = 1.0      # power of two still pending on the attention output (fp16 x 3 route)
        y = _norm_act(self.norm, x, act=False)
        # [b, c, h, w] -> [b, 1, hw, c]
        if _nhwc(y):
            # channels_last: [b, hw, c] is a free view of the conv output and of the result
            if FUSED_QKV and _infer_ok(y):
                # q, k, v = three 1x1 convolutions of the same tensor = ONE GEMM [b*hw, c] x [c, 3c] with the biases in
                # its epilogue (instead of 3 MIOpen launches + 3 bias-add passes); the thirds are strided views
                wqkv, bqkv = self._qkv_weights()
                if self._own_qkv_ok(y):
                    # ... as libgqhip's fp16 x 3 GEMM over the pixels (the fp32 library GEMM runs at ~130 TFLOP/s)
                    qkv_wf, qkv_us = self._qkv_weights_f16()
                    qkv = _lib.conv1x1_direct(y, qkv_wf, qkv_us, _gn_act_bound(self.norm, x), bias=bqkv)
                    qkv = qkv.permute(0, 2, 3, 1).reshape(b, 1, h * w, 3 * c)
                else:
                    qkv = torch.addmm(bqkv, y.permute(0, 2, 3, 1).reshape(b * h * w, c), wqkv).view(b, 1, h * w, 3 * c)
                q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
            else:
                qkv = None
                q, k, v = (f(y).permute(0, 2, 3, 1).reshape(b, 1, h * w, c) for f in (self.q, self.k, self.v))
            if qkv is not None and qkv.is_contiguous():
                if self._f16x3_attention_ok(y):
                    # both attention GEMMs as fp16 GEMMs over K axes of two-term fp16 splits (fp32 accumulation): the fp32
                    # GEMMs are a split-bf16 emulation at ~120 TFLOP/s; operand scales from rigorous bounds (GroupNorm bound x
                    # weight row sums), the softmax writes the split operand of the second GEMM directly
                    yb = _gn_act_bound(self.norm, x)
                    a, a_scale = _lib.attention_f16x3(qkv.view(b, h * w, 3 * c), self._qk_bound(yb), self._v_bound(yb))
            if a_scale == 1.0:
                a = _sdpa(q, k, v)
            a = a.reshape(b, h, w, c).permute(0, 3, 1, 2)   # (times a_scale: folded into proj_out's scale below)
        else:
            q, k, v = (f(y).reshape(b, 1, c, h * w).transpose(2, 3).contiguous() for f in (self.q, self.k, self.v))
            a = _sdpa(q, k, v)
            a = a.transpose(2, 3).reshape(b, c, h, w)
        return a, a_scale

    def _proj_out(self, x: torch.Tensor, a: torch.Tensor, a_scale: float) -> torch.Tensor:
        """x + proj_out(a * a_scale)."""
        if _proj_tail_ok(self.proj_out, x, a):
            # proj_out + bias + residual add + the next GroupNorm's statistics in one fp16 x 3 GEMM over the pixels.  Scale:
            # the attention output is a convex combination of the rows of v, so |a| <= max|v| <= max|y| max_j ||W_v[j]||_1 +
            # max|b_v|, with |y| bounded by the GroupNorm bound
            wf, us = _direct_weights(self.proj_out)
            return _tagged(_lib.conv1x1_direct(a, wf, us, self._v_bound(_gn_act_bound(self.norm, x)) / a_scale, residual=x,
                                               bias=self.proj_out.bias, stats_groups=GN_GROUPS, post_scale=a_scale))[0]
        if a_scale != 1.0:
            a = a * a_scale
        p, pb = _conv3x3(self.proj_out, a)
        return _add(x, p, pb)

    @staticmethod
    def _own_qkv_ok(y: torch.Tensor) -> bool:
        """The q | k | v projection of y (the normalised tensor, or x where the GroupNorm runs inside the projection: same shape,
        layout and dtype) as ONE libgqhip fp16 x 3 GEMM over the pixels.  c = 512: the plain kernel's 3c = 1536 columns."""
        return (FUSED_QKV and DIRECT_CONV_1X1 and _infer_ok(y) and y.shape[1] == 512 and (y.shape[2] * y.shape[3]) % 256 == 0
                and _nhwc(y))    # (whatever FUSED_GN says)

    @staticmethod
    def _f16x3_attention_ok(y: torch.Tensor) -> bool:
        """Both attention GEMMs as fp16 x 3 library GEMMs (_lib.attention_f16x3 / attention_from_operands)."""
        return ATTN_F16X3 and y.shape[1] % 4 == 0 and _lib.bmm_out_dtype_ok(y.device) and (y.shape[2] * y.shape[3]) in _lib.ATTN_L_OK

    def _fused_proj_attention(self, x: torch.Tensor):
        """The fp16 x 3 attention route below with its two reformatting passes folded into the q | k | v projection
        (gq_conv3.h: conv1x1_f16x3_kernel, GN + SPLIT): the GroupNorm is applied while x is staged -- the normalised tensor is
        never written -- and the epilogue stores the operands of the two attention GEMMs, so neither the fp32 q | k | v nor
        attn_split_qkv's pass over it exists.  Bit for bit the unfused route's result.  Returns (O_raw, scale) or None where
        that route's own conditions (_own_qkv_ok, _f16x3_attention_ok: shared with _attention, so the two cannot drift apart) or
        the variant's (a GroupNorm the NHWC kernels take) do not hold.  c = 512 like the route it replaces: at other widths the
        unfused projection is a library GEMM and "bit for bit" would have nothing to hold against."""
        b, c, h, w = x.shape
        if not (self._own_qkv_ok(x) and self._f16x3_attention_ok(x) and _use_fused(x, self.norm)):
            return None
        if not _lib.gn_nhwc_ok(c, self.norm.num_groups):
            return None
        bqkv = self._qkv_weights()[1]
        qkv_wf, qkv_us = self._qkv_weights_f16()
        yb = _gn_act_bound(self.norm, x)
        sq, sv = _lib.attention_scales(self._qk_bound(yb), self._v_bound(yb))
        gn = _gn_tuple(self.norm, x, None, silu=False)
        q3, k3, v3 = _lib.qkv_split_direct(x, qkv_wf, qkv_us, yb, sq, sv, bias=bqkv, gn=gn)
        return _lib.attention_from_operands(q3, k3, v3, sq, sv)

    def _qk_bound(self, y_bound: float) -> float:
        """max(|q|, |k|) for |y| <= y_bound: q = W_q y + b_q, k = W_k y + b_k."""
        ps = (self.q.weight, self.k.weight, self.q.bias, self.k.bias)

        def build():
            c = self.q.weight.shape[0]
            rs = max(float(self.q.weight.detach().reshape(c, -1).abs().sum(1).max()),
                     float(self.k.weight.detach().reshape(c, -1).abs().sum(1).max()))
            return rs, max(float(self.q.bias.detach().abs().max()), float(self.k.bias.detach().abs().max()))

        qkb = _cached(self, "qk_bound", _wkey(*ps), build)
        return y_bound * qkb[0] + qkb[1]

    def _v_bound(self, y_bound: float) -> float:
        """max|v| for |y| <= y_bound: v = W_v y + b_v."""
        def build():
            wv = self.v.weight.detach().reshape(self.v.weight.shape[0], -1)
            return float(wv.abs().sum(1).max()), float(self.v.bias.detach().abs().max())

        vb = _cached(self, "v_bound", _wkey(self.v.weight, self.v.bias), build)
        return y_bound * vb[0] + vb[1]


class Downsample(nn.Module):
    """Asymmetric (0,1,0,1) pad + stride-2 conv3; unet.py:76-97."""

    def __init__(self, ch: int, with_conv: bool = True, padding_mode: str = "zeros") -> None:
        super().__init__()
        self.with_conv = with_conv
        self.mode = "constant" if padding_mode == "zeros" else padding_mode
        if with_conv:
            self.conv = _conv3(ch, ch, stride=2, padding=0)

    def forward(self, x: torch.Tensor):
        """Returns (y, pending_bias) -- see ``_conv3x3``."""
        if not self.with_conv:
            return F.avg_pool2d(x, 2, 2), None
        conv = self.conv
        if _stride2_ok(conv, x, self.mode):
            # pad + stride-2 convolution + bias + the next GroupNorm's statistics as ONE fp16 x 3 kernel on the four phase
            # images of x (MIOpen: a padding pass + an fp32 implicit GEMM, 0.7-1.0 ms); the scale of x comes, on the device,
            # from the statistics its producer left behind (or computed here): |x| <= sqrt(group sum of squares)
            s2_wf, s2_us = _cached(conv, "s2_wf", _wkey(conv.weight), lambda: _lib.conv3s2_weights_f16(conv.weight))
            scales = _lib.f16_scales(_stats_of(x, None, GN_GROUPS), 1.0, s2_us)
            return _tagged(_lib.conv3x3s2_direct(x, s2_wf, s2_us, scales, bias=conv.bias, stats_groups=GN_GROUPS))
        if self.mode == "constant":
            x = F.pad(x, (0, 1, 0, 1), mode="constant", value=0)
        else:
            x = F.pad(x, (0, 1, 0, 1), mode=self.mode)
        return _conv3x3(self.conv, x)


class Upsample(nn.Module):
    """Nearest x2 + conv3; unet.py:60-73."""

    def __init__(self, ch: int, with_conv: bool = True, padding_mode: str = "zeros") -> None:
        super().__init__()
        self.with_conv = with_conv
        if with_conv:
            self.conv = _conv3(ch, ch, padding_mode)

    def _phase_weights(self) -> torch.Tensor:
        """[4*Cin, 4*Cout] matrix of the 3x3 kernel folded onto the low-resolution grid: one 2x2 kernel per output phase
        (a, b); tap u of phase a collects the kernel rows that land on source row i-1+a+u: a=0: {0}, {1,2};  a=1: {0,1}, {2}
        (same for columns).  Row index (2u+v)*Cin + ci, column (2a+b)*Cout + co.  Cached until the weight changes."""
        def build():
            w = self.conv.weight.detach()
            rows = (((0,), (1, 2)), ((0, 1), (2,)))
            cout, cin = w.shape[0], w.shape[1]
            m = w.new_zeros(2, 2, cin, 2, 2, cout)          # [u, v, ci, a, b, co]
            for a in range(2):
                for b in range(2):
                    for u in range(2):
                        for v in range(2):
                            for kh in rows[a][u]:
                                for kw in rows[b][v]:
                                    m[u, v, :, a, b, :] += w[:, :, kh, kw].t()
            return m.reshape(4 * cin, 4 * cout).contiguous()

        return _cached(self, "phase_w", _wkey(self.conv.weight), build)

    def forward(self, x: torch.Tensor):
        """Returns (y, pending_bias) -- see ``_conv3x3``."""
        # nearest x2 then conv3x3 == four 2x2 convolutions of the low-resolution input (one per output phase): 16 instead of 36
        # tap evaluations per source pixel, no upsampled tensor -- one libgqhip kernel, with the bias added and the statistics of
        # the next ResnetBlock's norm1 left behind.  The scale of x comes, on the device, from the statistics its producer left (sqrt
        # of a group's sum of squares bounds its largest element): without those (a memo of _stats_of does not count), not taken
        stats = _left_stats(x, GN_GROUPS) if _upconv_ok(self, x) else None
        if stats is not None:
            c, cout = x.shape[1], self.conv.out_channels
            wf, wf_us = _cached(self, "phase_wf", _wkey(self.conv.weight),
                                lambda: _lib.upconv_weights_f16(self._phase_weights(), c, cout))
            scales = _lib.f16_scales(stats, 1.0, wf_us)
            return _tagged(_lib.upconv2x_direct(x, wf, wf_us, scales, bias=self.conv.bias, stats_groups=GN_GROUPS))
        if _own_ok(x) and x.shape[1] % 4 == 0:   # what the direct kernel does not take: a plain NHWC copy kernel, then the convolution
            x = _lib.upsample2x_nhwc(x)   # ATen's NHWC nearest kernel runs at ~1.6 TB/s; this one is a plain copy
        else:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        return _conv3x3(self.conv, x) if self.with_conv else (x, None)


def _make_attn(ch: int, attn_type: str) -> nn.Module:
    if attn_type == "vanilla":
        return AttnBlock(ch)
    if attn_type == "none":
        return nn.Identity()
    raise NotImplementedError(f"attn_type={attn_type!r} is not on the SD3-UNet hot path (reference unet.py:291-314)")


class _Level(nn.Module):
    """One resolution level: res blocks (+ per-block attention) and the optional resampler."""

    def __init__(self) -> None:
        super().__init__()
        self.block = nn.ModuleList()
        self.attn = nn.ModuleList()

    def run(self, h: torch.Tensor, pre_bias=None) -> torch.Tensor:
        has_attn = len(self.attn) > 0
        for i, blk in enumerate(self.block):
            h = blk(h, pre_bias if i == 0 else None)
            if has_attn:
                h = self.attn[i](h)
        return h


class _Mid(nn.Module):
    def __init__(self, ch: int, dropout: float, padding_mode: str) -> None:
        super().__init__()
        self.block_1 = ResnetBlock(ch, ch, dropout, padding_mode)
        self.block_2 = ResnetBlock(ch, ch, dropout, padding_mode)  # no mid attention (unet.py:391, :500)

    def forward(self, h: torch.Tensor, pre_bias=None) -> torch.Tensor:
        return self.block_2(self.block_1(h, pre_bias))


class Encoder(nn.Module):
    def __init__(self, *, ch: int, out_ch: int = 3, ch_mult: Sequence[int] = (1, 2, 4, 8), num_res_blocks: int,
                 attn_resolutions: Sequence[int], dropout: float = 0.0, resamp_with_conv: bool = True,
                 in_channels: int, resolution: int, z_channels: int, double_z: bool = True,
                 use_linear_attn: bool = False, attn_type: str = "vanilla", padding_mode: str = "zeros",
                 **ignore_kwargs) -> None:
        super().__init__()
        self.register_load_state_dict_post_hook(_drop_caches_after_load)
        if use_linear_attn:
            attn_type = "linear"
        self.ch, self.resolution, self.in_channels = ch, resolution, in_channels
        self.num_resolutions, self.num_res_blocks = len(ch_mult), num_res_blocks
        self.conv_in = _conv3(in_channels, ch, padding_mode)
        widths = [ch] + [ch * m for m in ch_mult]
        res = resolution
        self.down = nn.ModuleList()
        for lvl in range(self.num_resolutions):
            level = _Level()
            cin = widths[lvl]
            for _ in range(num_res_blocks):
                level.block.append(ResnetBlock(cin, widths[lvl + 1], dropout, padding_mode))
                cin = widths[lvl + 1]
                if res in attn_resolutions:
                    level.attn.append(_make_attn(cin, attn_type))
            if lvl != self.num_resolutions - 1:
                level.downsample = Downsample(cin, resamp_with_conv, padding_mode)
                res //= 2
            self.down.append(level)
        top = widths[-1]
        self.mid = _Mid(top, dropout, padding_mode)
        self.norm_out = _gn(top)
        self.conv_out = _conv3(top, 2 * z_channels if double_z else z_channels, padding_mode)
        if WINOGRAD_ENCODER:
            mark_winograd(self)   # F(2x2,3x3) only: the encoder's rounding decides indices

    def invalidate_caches(self) -> None:
        invalidate_caches(self)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _guarded(self, self._forward, x)

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        x = _match_layout(x, self.conv_in)
        h, pb = _conv_in_small(self.conv_in, x)
        for lvl, level in enumerate(self.down):
            h, pb = level.run(h, pb), None
            if lvl != self.num_resolutions - 1:
                h, pb = level.downsample(h)
        h = self.mid(h, pb)
        return _norm_act_conv_f32(self.norm_out, self.conv_out, h)


class Decoder(nn.Module):
    def __init__(self, *, ch: int, out_ch: int, ch_mult: Sequence[int] = (1, 2, 4, 8), num_res_blocks: int,
                 attn_resolutions: Sequence[int], dropout: float = 0.0, resamp_with_conv: bool = True,
                 in_channels: int, resolution: int, z_channels: int, give_pre_end: bool = False,
                 tanh_out: bool = False, use_linear_attn: bool = False, attn_type: str = "vanilla",
                 padding_mode: str = "zeros", **ignore_kwargs) -> None:
        super().__init__()
        self.register_load_state_dict_post_hook(_drop_caches_after_load)
        if use_linear_attn:
            attn_type = "linear"
        self.ch, self.resolution, self.in_channels = ch, resolution, in_channels
        self.num_resolutions, self.num_res_blocks = len(ch_mult), num_res_blocks
        self.give_pre_end, self.tanh_out = give_pre_end, tanh_out
        top = ch * ch_mult[-1]
        res = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, res, res)
        self.conv_in = _conv3(z_channels, top, padding_mode)
        self.mid = _Mid(top, dropout, padding_mode)
        levels = []
        cin = top
        for lvl in reversed(range(self.num_resolutions)):
            level = _Level()
            cout = ch * ch_mult[lvl]
            for _ in range(num_res_blocks + 1):
                level.block.append(ResnetBlock(cin, cout, dropout, padding_mode))
                cin = cout
                if res in attn_resolutions:
                    level.attn.append(_make_attn(cin, attn_type))
            if lvl != 0:
                level.upsample = Upsample(cin, resamp_with_conv, padding_mode)
                res *= 2
            levels.append(level)
        self.up = nn.ModuleList(reversed(levels))  # index = resolution level, like the reference
        self.norm_out = _gn(cin)
        self.conv_out = _conv3(cin, out_ch, padding_mode)
        mark_winograd(self, f4=True)

    def get_last_layer(self, **kwargs) -> torch.Tensor:
        return self.conv_out.weight

    def invalidate_caches(self) -> None:
        invalidate_caches(self)

    def forward(self, z: torch.Tensor, **kwargs) -> torch.Tensor:
        self.last_z_shape = z.shape
        return _guarded(self, self._forward, z)

    def _forward(self, z: torch.Tensor) -> torch.Tensor:
        z = _match_layout(z, self.conv_in)
        h, pb = (_conv_f32(self.conv_in, z), None) if _conv_f32_ok(self.conv_in, z, False) else _conv3x3(self.conv_in, z)
        h, pb = self.mid(h, pb), None
        for lvl in reversed(range(self.num_resolutions)):
            h, pb = self.up[lvl].run(h, pb), None
            if lvl != 0:
                h, pb = self.up[lvl].upsample(h)
        if self.give_pre_end:
            return h
        h = _norm_act_conv_small(self.norm_out, self.conv_out, h, pb)
        return torch.tanh(h) if self.tanh_out else h
