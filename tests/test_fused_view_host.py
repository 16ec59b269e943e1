"""The one library view and the one train switch of the quantiser modules (pit_hip/quantization/_fused.py), on CPU tensors.

Every row of the two view tables: the layout name, the view's shape, whether the view shares the input's storage, that it is
contiguous, and the round trip -- a library output with fewer channels (half of them, as zhat has; one, as an index tensor has)
comes back through ``restore`` as the matching slice of the module tensor, in the module's logical shape."""
import importlib
import math

import pytest
import torch

from pit_hip.quantization import _fused


def _arange(*shape):
    return torch.arange(math.prod(shape), dtype=torch.float32).reshape(*shape)


def _check(t, view, channel_axis, want_layout, want_shape, shares_storage):
    tv, layout, restore = view
    assert layout == want_layout
    assert tuple(tv.shape) == tuple(want_shape)
    assert tv.is_contiguous()
    if shares_storage:
        assert tv.data_ptr() == t.data_ptr()
    assert torch.equal(restore(tv), t) and restore(tv).shape == t.shape
    lib_axis = 1 if layout == "bchw" else 2
    C = t.shape[channel_axis]
    assert tv.shape[lib_axis] == C
    for channels in (C // 2, 1):
        out = tv.narrow(lib_axis, 0, channels).contiguous()         # what a library call returns: its own contiguous tensor
        back = restore(out)
        want = t.narrow(channel_axis, 0, channels)
        assert back.shape == want.shape and torch.equal(back, want)
        assert back.data_ptr() == out.data_ptr()                     # restore never copies


# ---- modules with a format: GQ1 eval and train, VQ, LFQ ------------------------------------------------------------------
def test_format_bchw_contiguous_is_passed_as_is():
    t = _arange(2, 8, 3, 5)
    tv, layout, _ = view = _fused.format_view(t, "bchw")
    assert tv is t
    _check(t, view, 1, "bchw", (2, 8, 3, 5), True)


def test_format_bchw_channels_last_is_blc_on_the_same_storage():
    t = _arange(2, 8, 3, 5).contiguous(memory_format=torch.channels_last)
    assert not t.is_contiguous()
    view = _fused.format_view(t, "bchw")
    _check(t, view, 1, "blc", (2, 15, 8), True)
    back = view[2](view[0].narrow(2, 0, 4).contiguous())
    assert back.is_contiguous(memory_format=torch.channels_last)     # logical [b, X, h, w] in channels_last strides


def test_format_bchw_neither_is_copied():
    base = _arange(2, 8, 3, 10)
    t = base[..., ::2]
    assert not t.is_contiguous() and not t.is_contiguous(memory_format=torch.channels_last)
    view = _fused.format_view(t, "bchw")
    _check(t, view, 1, "bchw", (2, 8, 3, 5), False)
    assert view[0].data_ptr() != t.data_ptr()
    tt = _arange(2, 3, 8, 5).transpose(1, 2)                          # a transpose
    _check(tt, _fused.format_view(tt, "bchw"), 1, "bchw", (2, 8, 3, 5), False)


def test_format_bchw_contiguous_wins_when_both():
    t = _arange(2, 8, 1, 1)
    assert t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)
    _check(t, _fused.format_view(t, "bchw"), 1, "bchw", (2, 8, 1, 1), True)
    t = t.contiguous(memory_format=torch.channels_last)
    _check(t, _fused.format_view(t, "bchw"), 1, "bchw", (2, 8, 1, 1), True)


def test_format_blc():
    t = _arange(2, 15, 8)
    tv, _, _ = view = _fused.format_view(t, "blc")
    assert tv is t
    _check(t, view, 2, "blc", (2, 15, 8), True)
    ts = _arange(2, 15, 16)[..., ::2]                                 # not contiguous: the one copy
    _check(ts, _fused.format_view(ts, "blc"), 2, "blc", (2, 15, 8), False)


# ---- the module with a free channel axis: GQ2 ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim_idx", [1, -4])
def test_axis_contiguous_inner_axes_is_bchw(dim_idx):
    t = _arange(2, 8, 2, 3, 5)
    _check(t, _fused.axis_view(t, dim_idx), 1, "bchw", (2, 8, 30), True)


def test_axis_contiguous_middle_axis_folds_outer():
    t = _arange(2, 3, 8, 5)
    _check(t, _fused.axis_view(t, 2), 2, "bchw", (6, 8, 5), True)


@pytest.mark.parametrize("shape, want", [((2, 8, 2, 3, 5), (1, 96, 5)), ((2, 3, 5, 8), (1, 30, 8)), ((2, 2, 3, 5, 8), (1, 60, 8)), ((15, 8), (1, 15, 8))])
def test_axis_contiguous_last_axis_is_one_blc_image(shape, want):
    t = _arange(*shape)
    _check(t, _fused.axis_view(t, -1), len(shape) - 1, "blc", want, True)


def test_axis_channels_last_4d_is_not_copied():
    t = _arange(2, 8, 3, 5).contiguous(memory_format=torch.channels_last)
    _check(t, _fused.axis_view(t, 1), 1, "blc", (1, 30, 8), True)
    _check(t, _fused.axis_view(t, -3), 1, "blc", (1, 30, 8), True)


def test_axis_not_contiguous_is_copied_once():
    t = _arange(2, 8, 2, 3, 10)[..., ::2]
    _check(t, _fused.axis_view(t, 1), 1, "blc", (1, 60, 8), False)
    _check(t, _fused.axis_view(t, -1), 4, "blc", (1, 96, 5), False)
    tl = _arange(2, 8, 3, 5).contiguous(memory_format=torch.channels_last)
    _check(tl, _fused.axis_view(tl, -1), 3, "blc", (1, 48, 5), False)    # channels_last, but the channel axis asked for is w


def test_positions_view_is_always_one_blc_image():
    """What GaussianQuantRegularizer2.dequant hands over: the indices with their channel axis last, contiguous or not."""
    t = _arange(2, 4, 3, 5)
    _check(t, _fused.positions_view(t, 1), 1, "blc", (1, 30, 4), False)
    tl = _arange(2, 3, 5, 4)
    _check(tl, _fused.positions_view(tl, 3), 3, "blc", (1, 30, 4), True)


def test_the_two_families_fold_the_batch_differently():
    t = _arange(2, 8, 3, 5).contiguous(memory_format=torch.channels_last)
    assert _fused.format_view(t, "bchw")[0].shape == (2, 15, 8) and _fused.axis_view(t, 1)[0].shape == (1, 30, 8)
    assert _fused.format_view(t, "bchw")[0].data_ptr() == _fused.axis_view(t, 1)[0].data_ptr()


def test_mu_shape_halves_the_channel_axis():
    assert _fused.mu_shape(torch.empty(2, 8, 3, 5), "bchw") == (2, 4, 3, 5)
    assert _fused.mu_shape(torch.empty(6, 8, 5), "bchw") == (6, 4, 5)
    assert _fused.mu_shape(torch.empty(2, 15, 8), "blc") == (2, 15, 4)


# ---- the switch ----------------------------------------------------------------------------------------------------------
def test_train_fused_follows_the_environment_per_call(monkeypatch):
    monkeypatch.delenv("GQHIP_TRAIN_FUSED", raising=False)
    assert _fused.train_fused() is True
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "0")
    assert _fused.train_fused() is False
    monkeypatch.setenv("GQHIP_TRAIN_FUSED", "1")
    assert _fused.train_fused() is True


@pytest.mark.parametrize("name", ["gaussian", "vq", "lfq"])
def test_modules_share_the_one_switch(name):
    mod = importlib.import_module(f"pit_hip.quantization.{name}")
    assert not hasattr(mod, "_train_fused")
    assert mod.train_fused is _fused.train_fused


# ---- the scratch owner of pit_hip._lib (its capture rule needs a GPU: tests/test_gpu_scratch_capture.py) --------------------
def test_scratch_classes_are_freed_by_reference_count():
    """A module's workspaces hold device memory: dropping the module must free them at once, not at the next cyclic collection."""
    import gc
    import weakref

    from pit_hip import _lib

    gc.collect()
    gc.disable()
    try:
        for cls in (_lib.Workspace, _lib.VqBackwardWorkspace, _lib.LfqTrainWorkspace):
            ws = cls()
            refs = [weakref.ref(ws)] + ([weakref.ref(ws._cache)] if cls is _lib.Workspace else [])
            del ws
            assert all(r() is None for r in refs), cls.__name__
    finally:
        gc.enable()
