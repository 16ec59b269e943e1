"""GPU: per-image SSIM / MS-SSIM (gq_ssim_f32, csrc/gq_ssim.h) against the fp64 restatement tests/ssim_ref.py, determinism, the
three-metric step record (gq_step_record_ssim_f32) against the one-metric record and pack(), graph capture, and
evaluate_sharded(metrics=...) at world size 1."""
import numpy as np
import pytest
import torch

import ssim_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(b, c, h, w, seed, noise=0.08):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, c, h, w, generator=g) * 2 - 1
    y = x + noise * torch.randn(b, c, h, w, generator=g)          # realistic reconstruction: some values beyond +-1
    return x, y


@pytest.mark.parametrize("b,c,h,w,cl,zero_mean", [(16, 3, 256, 256, False, True), (16, 3, 256, 256, True, True),
                                                  (4, 3, 512, 512, True, True), (2, 3, 257, 263, False, True),
                                                  (2, 3, 256, 384, True, False), (3, 1, 256, 256, False, False),
                                                  (3, 3, 32, 32, True, True), (2, 3, 8, 40, False, True),
                                                  (2, 1, 8, 40, True, False)])
def test_ssim_kernel_matches_fp64_reference(b, c, h, w, cl, zero_mean):
    from pit_hip.eval_dist import get_ssim, get_ssim_and_msssim

    x, y = _pair(b, c, h, w, seed=b * 1000 + h + w + c)
    if not zero_mean:
        x, y = (x + 1) / 2, (y + 1) / 2
    ws, wm = S.ssim_msssim(x.numpy(), y.numpy(), zero_mean)
    xd, yd = x.to(DEV), y.to(DEV)
    if cl:
        xd, yd = xd.contiguous(memory_format=torch.channels_last), yd.contiguous(memory_format=torch.channels_last)
    gs, gm = get_ssim_and_msssim(xd, yd, zero_mean=zero_mean)
    assert gs.device == xd.device and gs.dtype == torch.float32 and gs.shape == (b,)
    gs, gm = gs.cpu().numpy().astype(np.float64), gm.cpu().numpy().astype(np.float64)
    print(f"{(b, c, h, w)} cl={cl}: |ssim - ref| {np.abs(gs - ws).max():.2e}  |ms - ref| {np.nanmax(np.abs(gm - wm)) if h >= 256 and w >= 256 else float('nan'):.2e}")
    assert np.abs(gs - ws).max() <= 1e-6
    if h >= 256 and w >= 256:
        assert np.isfinite(gm).all() and np.abs(gm - wm).max() <= 1e-6
    else:
        assert np.isnan(gm).all()
    assert torch.equal(get_ssim(xd, yd, zero_mean=zero_mean).cpu(), torch.from_numpy(gs.astype(np.float32)))
    same_s, same_m = get_ssim_and_msssim(xd, xd.clone(memory_format=torch.preserve_format), zero_mean=zero_mean)
    assert (same_s.cpu() - 1).abs().max() <= 1e-6
    if h >= 256 and w >= 256:
        assert (same_m.cpu() - 1).abs().max() <= 1e-6


def test_ssim_kernel_is_deterministic_and_resets_its_workspace():
    from pit_hip import _lib

    x, y = _pair(4, 3, 257, 263, 11)
    x, y = x.to(DEV), y.to(DEV)
    ws = {}
    runs = [_lib.image_quality(x, y, True, True, ws) for _ in range(3)]
    torch.cuda.synchronize()
    for s, m in runs[1:]:
        assert torch.equal(s.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(m.view(torch.int32), runs[0][1].view(torch.int32))
    (buf,) = ws.values()
    assert int(buf[:256].count_nonzero()) == 0           # the per-image tickets are zero again
    s_only, none = _lib.image_quality(x, y, True, False, ws)   # NULL MS-SSIM: level 0 only, the same SSIM bits
    assert none is None and torch.equal(s_only, runs[0][0])


@pytest.mark.parametrize("B,C,H,W,K,cl", [(16, 3, 256, 256, 1, True), (3, 3, 257, 263, 3, False), (2, 3, 64, 48, 1, True)])
def test_three_metric_record(B, C, H, W, K, cl):
    """Index words = pack(); PSNR words bit-equal to the one-metric record's; SSIM / MS-SSIM words = get_ssim_and_msssim."""
    from pit_hip.eval_dist import StepRecord, get_ssim_and_msssim

    x, y = _pair(B, C, H, W, B + H)
    x, y = x.to(DEV), y.to(DEV)
    if cl:
        x, y = x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)
    h, w = max(H // 16, 1), max(W // 16, 1)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 65536, (B, K, h, w), generator=g).to(DEV)
    lay3, lay1 = StepRecord(B, K * h * w, n_metrics=3), StepRecord(B, K * h * w, n_metrics=1)
    for _ in range(3):
        rec3 = lay3.pack_with_metrics(idx, x, y)
    rec1 = lay1.pack_with_psnr(idx, x, y)
    torch.cuda.synchronize()
    assert torch.equal(rec3[3 * B:], lay3.pack(idx, torch.zeros(B, 3, device=DEV))[3 * B:])
    assert torch.equal(rec3[0:3 * B:3], rec1[:B])
    s, m = get_ssim_and_msssim(x, y, zero_mean=True)
    assert torch.equal(rec3[1:3 * B:3], s.view(torch.int32))
    assert torch.equal(rec3[2:3 * B:3], m.view(torch.int32))
    i3, m3 = lay3.unpack(rec3)
    assert torch.equal(i3.reshape(-1), idx.reshape(-1)) and m3.shape == (B, 3)
    if cl:   # NCHW inputs against a channels_last reconstruction (eval_sharded's case): the kernels, the same bits
        assert torch.equal(lay3.pack_with_metrics(idx, x.contiguous(), y), rec3)


def test_three_metric_record_replays_in_a_graph():
    from pit_hip.eval_dist import StepRecord

    B, C, H, W = 16, 3, 256, 256
    x, y = _pair(B, C, H, W, 21)
    x = x.to(DEV).contiguous(memory_format=torch.channels_last)
    y = y.to(DEV).contiguous(memory_format=torch.channels_last)
    idx = torch.randint(0, 65536, (B, 1, 16, 16), generator=torch.Generator().manual_seed(1)).to(DEV)
    lay = StepRecord(B, 256, n_metrics=3)
    eager = lay.pack_with_metrics(idx, x, y).clone()     # warm-up outside the capture: the workspace is allocated here
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = lay.pack_with_metrics(idx, x, y)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    y.mul_(0.5)                                            # new data through the same graph
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, lay.pack_with_metrics(idx, x, y))


class _StubModel:
    def encode(self, x, return_reg_log=True):
        ids = x[:, 0, 0, 0].round().long()
        tok = (ids[:, None] * 7 + torch.arange(4, device=x.device)[None]) % 65536
        return x, {"indices": tok.reshape(-1, 1, 2, 2)}

    def decode(self, z):
        return z * 0.8 + 0.05 * torch.sin(7 * z)


def test_evaluate_sharded_three_metrics_world_one():
    from pit_hip.eval_dist import evaluate_sharded, get_ssim_and_msssim, psnr_zero_mean

    def images_for(ids):
        g = torch.Generator().manual_seed(77)
        bank = torch.rand(6, 3, 256, 256, generator=g) * 2 - 1
        bank[:, 0, 0, 0] = torch.arange(6, dtype=torch.float32)
        return bank[ids]

    dev = torch.device(DEV)
    out = evaluate_sharded(_StubModel(), images_for, 6, 2, 0, 1, dev, 4, metrics=("psnr", "ssim", "ms_ssim"))
    x = images_for(list(range(6))).to(dev)
    xr = _StubModel().decode(x)
    s, m = get_ssim_and_msssim(x, xr, zero_mean=True)
    assert torch.equal(out["ssim"], s) and torch.equal(out["ms_ssim"], m)
    np.testing.assert_allclose(out["psnr"].cpu().numpy(), psnr_zero_mean(x, xr).cpu().numpy(), rtol=2e-6)
    base = evaluate_sharded(_StubModel(), images_for, 6, 2, 0, 1, dev, 4)
    assert set(base) == {"indices", "psnr"} and torch.equal(base["indices"], out["indices"])
    np.testing.assert_allclose(base["psnr"].cpu().numpy(), out["psnr"].cpu().numpy(), rtol=2e-6)
