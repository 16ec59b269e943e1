"""The module layer's host-side vocabulary (pit_hip/modules/unet.py, the conv-stack half of pit_hip/_lib.py), on CPU tensors: the
two accessors of what a producer leaves on its output, the plain-3x3 predicate behind mark_winograd, the two named tuples of the
_lib boundary."""
import torch
import torch.nn as nn

from pit_hip import _lib
from pit_hip.modules import unet as U

TOY = dict(ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[8], resolution=64, z_channels=16, double_z=True,
           in_channels=3, out_ch=3, dropout=0.0, attn_type="vanilla")


def test_left_statistics_serve_matching_groups_no_pending_bias_and_the_very_tensor():
    records, memo = torch.arange(8), torch.arange(8) + 100     # (stand-ins: the accessors never look inside)
    x = torch.randn(2, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    pb, pb_twin = torch.randn(64), torch.randn(64)
    assert U._left_stats(x, 32) is None and U._left_stats(x, 32, memo=True) is None
    assert U._leave_stats(x, records, 32) is x
    # 1. matching groups, no pending bias, dense channels_last: the producer's records
    assert U._left_stats(x, 32) is records
    # 2. other groups
    assert U._left_stats(x, 16) is None
    # 3. a pending bias
    assert U._left_stats(x, 32, pb) is None
    # 4. the memo: kept apart from the producer's records, found only when asked for, for the identical bias object and groups
    assert U._left_stats(x, 32, pb, memo=True) is None
    U._leave_stats(x, memo, 32, pb, memo=True)
    assert U._left_stats(x, 32, pb, memo=True) is memo
    assert U._left_stats(x, 32, pb) is None
    assert U._left_stats(x, 32, pb_twin, memo=True) is None and U._left_stats(x, 32, pb.clone(), memo=True) is None
    assert U._left_stats(x, 16, pb, memo=True) is None
    assert U._left_stats(x, 32) is records and U._left_stats(x, 32, memo=True) is records   # (the producer's come first)
    m = torch.randn(2, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    U._leave_stats(m, memo, 32, None, memo=True)               # a memo for "no pending bias" is a memo all the same
    assert U._left_stats(m, 32) is None and U._left_stats(m, 32, memo=True) is memo
    # 5. a view of a tagged tensor, a copy and another layout of it carry nothing
    assert U._left_stats(x[:1], 32) is None and U._left_stats(x.view(2, 64, 4, 4), 32) is None
    assert U._left_stats(x.clone(), 32) is None and U._left_stats(x.contiguous(), 32) is None
    nchw = U._leave_stats(torch.randn(2, 64, 4, 4), records, 32)
    assert U._left_stats(nchw, 32) is None                     # records on a tensor that is not dense channels_last do not serve
    # the companion for the activation bound
    assert U._left_bound(x) is None
    U._leave_bound(x, 3.5)
    assert U._left_bound(x) == 3.5 and U._left_bound(x[:1]) is None


def _spelled_out(m) -> bool:
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1)
            and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


def test_mark_winograd_marks_exactly_the_plain_3x3_convolutions():
    for module, n_conv, n_marked, f4 in ((U.Encoder(**TOY), 35, 22, False), (U.Decoder(**TOY), 47, 33, True),
                                         (U.Decoder(**dict(TOY, padding_mode="reflect")), 47, 0, None)):
        convs = [m for m in module.modules() if isinstance(m, nn.Conv2d)]
        marked = [m for m in convs if getattr(m, "_gq_wino", False)]
        assert len(convs) == n_conv and len(marked) == n_marked
        assert [m for m in module.modules() if _spelled_out(m)] == marked
        assert all(U._plain3x3(m) == _spelled_out(m) for m in module.modules())
        assert all(m._gq_wino4 is f4 for m in marked)
        assert not any(hasattr(m, "_gq_wino4") for m in convs if m not in marked)


def test_named_tuples_take_plain_tuples_and_compare_equal_to_them():
    g, b, st, pb, u3, wf2 = (torch.zeros(1) for _ in range(6))
    gn = (g, b, 32, 1e-6, True, st, pb)
    fold = _lib.GnFold(*gn)
    assert isinstance(fold, tuple) and fold == gn and tuple(fold) == gn and len(fold) == 7
    assert (fold.gamma is g and fold.beta is b and fold.groups == 32 and fold.eps == 1e-6 and fold.silu is True
            and fold.stats is st and fold.pre_bias is pb)
    assert _lib.GnFold(*fold) == fold
    f3, f4 = (u3, 2.0, 7.5), (u3, 2.0, 7.5, wf2)
    assert _lib.F16Gemm(*f3) == f3 + (None,) and _lib.F16Gemm(*f3).wf2 is None
    gemm = _lib.F16Gemm(*f4)
    assert isinstance(gemm, tuple) and gemm == f4 and gemm.U3 is u3 and gemm.u_scale == 2.0 and gemm.bound == 7.5 and gemm.wf2 is wf2
    # what unet.py builds is the same tuple
    norm = nn.GroupNorm(32, 64, eps=1e-6)
    x = U._leave_stats(torch.randn(1, 64, 4, 4).contiguous(memory_format=torch.channels_last), st, 32)
    assert U._gn_tuple(norm, x, None, silu=False) == (norm.weight, norm.bias, 32, 1e-6, False, st, None)
