"""What the quantiser modules share on their way into libgqhip.so: the one train switch and the one library view.

The library reads a module tensor in one of two layouts (gqhip.h): "bchw" = [B, C, positions...] and "blc" = [B, L, C], both
contiguous.  A view here is ``(tensor in such a layout, its layout name, restore)``; ``restore`` maps any library output of that
layout (whatever its channel count: indices, std, zhat) back to the module's logical shape without a copy.
"""
from __future__ import annotations

import math
import os

import torch


def train_fused() -> bool:
    """False when GQHIP_TRAIN_FUSED=0 asks for the op-by-op torch path of a train step (read per call)."""
    return os.environ.get("GQHIP_TRAIN_FUSED", "1") != "0"


_OPT_IN = {"bsq": "GQHIP_BSQ_TRAIN_FUSED", "fsq": "GQHIP_FSQ_TRAIN_FUSED"}


def train_fused_opt_in(family: str) -> bool:
    """True when the fused train step of ``family`` ("bsq", "fsq") is asked for: ``train_fused()`` and the family's own variable
    (GQHIP_BSQ_TRAIN_FUSED / GQHIP_FSQ_TRAIN_FUSED) set to 1.  Read per call; unset, these modules keep their torch routes."""
    return train_fused() and os.environ.get(_OPT_IN[family], "0") == "1"


def _same(t):
    return t


def positions_view(t, d: int, keep_batch: bool = False):
    """Channel axis ``d`` last: a view of the same storage when the memory already is position-major (a channels_last
    [B, C, h, w] with d = 1: NHWC memory IS the "blc" layout with L = h * w), one copy otherwise."""
    tl = torch.movedim(t, d, -1)
    if not tl.is_contiguous():
        tl = tl.contiguous()
    lead = tl.shape[:-1]
    tv = tl.reshape(lead[0] if keep_batch else 1, -1, tl.shape[-1])
    return tv, "blc", lambda o: torch.movedim(o.reshape(*lead, -1), -1, d)


def format_view(t, fmt: str):
    """The view of a module with a ``format`` ("bchw": [b, C, h, w], "blc": [b, l, C]); the leading axis stays the batch.  A dense
    channels_last tensor is read, and its outputs come back, in that memory; any other non-contiguous one is copied."""
    if fmt == "blc" or t.is_contiguous():
        return t.contiguous(), fmt, _same
    if t.is_contiguous(memory_format=torch.channels_last):
        return positions_view(t, 1, keep_batch=True)
    return t.contiguous(), "bchw", _same


def axis_view(t, dim_idx: int):
    """The view of a module with a free channel axis ``dim_idx``: a contiguous tensor is [outer, C, inner] = "bchw" for any axis,
    everything else (the last axis, a channels_last 4-d tensor with dim_idx 1, a copy of the rest) is ONE "blc" image of all
    positions.

    Why two folds of the leading axes (B = b in format_view, B = 1 here): the "blc" kernels address rows by b * L + l only, so
    either fold would very likely give the same bits, but B and L are arguments of every launch and decide the empty-tensor
    edge (L >= 1 is required, B = 0 is allowed).  Each family keeps the fold it has always had."""
    d = dim_idx % t.dim()
    shape = t.shape
    inner = int(math.prod(shape[d + 1:]))
    if t.is_contiguous() and inner != 1:
        tv = t.reshape(int(math.prod(shape[:d])), shape[d], inner)
        return tv, "bchw", lambda o: o.reshape(*shape[:d], -1, *shape[d + 1:])
    return positions_view(t, d, keep_batch=False)


def mu_shape(tv, layout: str):
    """The shape of mu (and of the noise, zhat, std) for a view ``tv`` whose channel axis holds [mu | logvar]."""
    shape = list(tv.shape)
    shape[1 if layout == "bchw" else 2] //= 2
    return tuple(shape)
