#!/usr/bin/env python3
"""SHA-256 of what every conv-stack entry point with a GroupNorm fold or a Winograd transform in its kernel writes, on seeded
inputs: one line `<case> <digest>` per output (V, y, statistics records).  Run it once per library build and compare the lines:

    GQHIP_LIB=vq-vae-from-gaussian-vae_amd/csrc/libgqhip_parent.so python tools/convstack/fold_hashes.py > parent.txt
    python tools/convstack/fold_hashes.py > tree.txt && cmp parent.txt tree.txt

None of these kernels uses a floating-point atomic (the statistics are integer limb sums), so a build must agree with itself
between two runs before two builds are compared.  Shapes: 3 x 12 x 20 pixels for the transforms (border and interior tiles of
F(2x2,3x3) and F(4x4,3x3)), C = 128 and 256, 32 groups; the direct and fp32 convolutions at the smallest shapes of
tests/test_gpu_convstack_kernels.py."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd")]
from pit_hip import _lib  # noqa: E402

DEV = torch.device("cuda:0")
EPS = 1e-6


def out(case, *tensors):
    for i, t in enumerate(tensors):
        torch.cuda.synchronize()
        raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
        print(f"{case}{'/' + str(i) if len(tensors) > 1 else ''} {hashlib.sha256(raw).hexdigest()}")


def cl(*shape, scale=1.0, shift=0.0):
    return (scale * torch.randn(*shape) + shift).to(DEV).contiguous(memory_format=torch.channels_last)


def main():
    torch.manual_seed(1717)
    L = _lib.lib()
    for C in (128, 256):
        gamma, beta, pb = torch.randn(C).to(DEV), torch.randn(C).to(DEV), torch.randn(C).to(DEV)
        x = cl(3, C, 12, 20, scale=3.0, shift=0.5)
        # GroupNorm as its own pass: channels_last from given statistics, and gn_silu (its own statistics) in both layouts with a
        # pending bias; the NCHW kernel at H * W % 4 == 0
        for silu in (True, False):
            out(f"gn_apply C{C} silu{int(silu)}", _lib.gn_apply(x, gamma, beta, 32, EPS, silu, _lib.gn_stats(x, 32)))
            for pre in (None, pb):
                tag = f"C{C} silu{int(silu)} pre{int(pre is not None)}"
                out(f"gn_silu nhwc {tag}", _lib.gn_silu(x, gamma, beta, 32, EPS, silu=silu, pre_bias=pre))
                out(f"gn_silu nchw {tag}", _lib.gn_silu(x.contiguous(), gamma, beta, 32, EPS, silu=silu, pre_bias=pre))
        # the input transforms: plain and with the GroupNorm in front, fp32 / 3-plane / 2-plane operands
        for t in (2, 4):
            tiles, T = 3 * (12 // t) * (20 // t), (t + 2) ** 2
            for planes in (0, 3, 2):
                V = torch.zeros((T, tiles, (planes or 1) * C), dtype=torch.float16 if planes else torch.float32, device=DEV)
                _lib._wino_in(L, x, V, None, t, planes, 8.0)
                out(f"wino_in C{C} F{t} planes{planes}", V)
                for silu in (True, False):
                    for pre in (None, pb):
                        stats = _lib.gn_stats(x, 32, pre)
                        V.zero_()
                        _lib._wino_in(L, x, V, (gamma, beta, 32, EPS, silu, stats, pre), t, planes, 8.0)
                        out(f"wino_in_gn C{C} F{t} planes{planes} silu{int(silu)} pre{int(pre is not None)}", V)
            # the output transforms: plain, and with bias / residual / statistics of the result
            M = torch.randn(T, tiles, C).to(DEV)
            res, bias = cl(3, C, 12, 20), torch.randn(C).to(DEV)
            y = _lib._out_nhwc(x, C, 12, 20)
            _lib._check((L.wino4_out_nhwc_f32 if t == 4 else L.wino_out_nhwc_f32)(M.data_ptr(), y.data_ptr(), 3, 12, 20, C, 0.25,
                                                                                 _lib._stream()), "wino_out_nhwc_f32")
            out(f"wino_out C{C} F{t}", y)
            for r, b in ((None, None), (res, None), (None, bias), (res, bias)):
                y, stats = _lib._out_and_stats(x, C, 12, 20, 32)
                _lib._check(L.wino_out_res_nhwc_f32(M.data_ptr(), _lib._ptr(r), _lib._ptr(b), y.data_ptr(), stats.data_ptr(), 3, 12,
                                                    20, C, 32, t, 0.25, _lib._stream()), "wino_out_res_nhwc_f32")
                out(f"wino_out_res C{C} F{t} res{int(r is not None)} bias{int(b is not None)}", y, stats)
    # the direct convolutions with the fold in their prologue
    for cin, cout, shape in ((256, 128, (1, 8, 32)), (128, 256, (2, 16, 32))):
        gamma, beta, pb = torch.randn(cin).to(DEV), torch.randn(cin).to(DEV), torch.randn(cin).to(DEV)
        x = cl(shape[0], cin, *shape[1:], scale=2.0)
        w3, w1 = 0.05 * torch.randn(cout, cin, 3, 3).to(DEV), 0.05 * torch.randn(cout, cin, 1, 1).to(DEV)
        wf3, us3 = _lib.conv3_weights_f16(w3)
        wf1, us1 = _lib.conv3_weights_f16(w1)
        res, bias = cl(shape[0], cout, *shape[1:]), torch.randn(cout).to(DEV)
        for pre in (None, pb):
            stats = _lib.gn_stats(x, 32, pre)
            for silu in (True, False):
                gn = (gamma, beta, 32, EPS, silu, stats, pre)
                tag = f"{cin}->{cout} silu{int(silu)} pre{int(pre is not None)}"
                out(f"conv3x3_gn_f16x3 {tag}", *_lib.conv3x3_direct(x, wf3, us3, 64.0, gn, residual=res, bias=bias, stats_groups=32))
            gn = (gamma, beta, 32, EPS, False, stats, pre)
            out(f"conv1x1_gn_f16x3 {cin}->{cout} pre{int(pre is not None)}",
                *_lib.conv1x1_direct(x, wf1, us1, 64.0, residual=res, bias=bias, stats_groups=32, gn=gn))
            if cin == 128:
                wq, uq = _lib.conv3_weights_f16(0.05 * torch.randn(3 * cin, cin, 1, 1).to(DEV))
                out(f"conv1x1_qkv_split_f16x3 gn {cin} pre{int(pre is not None)}", *_lib.qkv_split_direct(x, wq, uq, 64.0, 4.0, 2.0, gn=gn))
    for cin, cout, shape, silu in ((128, 4, (1, 16, 16), False), (256, 1, (1, 16, 32), True)):
        gamma, beta, pb = torch.randn(cin).to(DEV), torch.randn(cin).to(DEV), torch.randn(cin).to(DEV)
        x = cl(shape[0], cin, *shape[1:], scale=2.0)
        w, bias = (0.05 * torch.randn(cout, 3, 3, cin)).to(DEV), torch.randn(cout).to(DEV)
        for pre in (None, pb):
            gn = (gamma, beta, 32, EPS, silu, _lib.gn_stats(x, 32, pre), pre)
            out(f"conv3x3_gn_small {cin}->{cout} silu{int(silu)} pre{int(pre is not None)}", _lib.conv3x3_gn_small(x, w, bias, gn))
    for cin, cout, H, W in ((512, 32, 8, 8), (512, 16, 32, 32)):
        gamma, beta, pb = torch.randn(cin).to(DEV), torch.randn(cin).to(DEV), torch.randn(cin).to(DEV)
        x = cl(3, cin, H, W, scale=1.5, shift=0.2)
        wk, bias = _lib.conv_f32_weights(0.05 * torch.randn(cout, cin, 3, 3).to(DEV)), torch.randn(cout).to(DEV)
        for silu in (True, False):
            for pre in (None, pb):
                gn = (gamma, beta, 32, EPS, silu, _lib.gn_stats(x, 32, pre), pre)
                out(f"conv3x3_f32 gn {cin}->{cout} {H}x{W} silu{int(silu)} pre{int(pre is not None)}",
                    _lib.conv3x3_f32(x, wk, cout, bias=bias, gn=gn))


if __name__ == "__main__":
    with torch.no_grad():
        main()
