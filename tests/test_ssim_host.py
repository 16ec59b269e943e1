"""CPU: SSIM / MS-SSIM (pit/evaluations/ssim.py via pytorch_msssim) -- the fp64 restatement tests/ssim_ref.py against an
independent scipy formulation and closed forms, the torch restatement of pit_hip.eval_dist against it, and the three-metric
step record through StepRecord and evaluate_sharded under gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ssim_ref as S


def _pair(b, c, h, w, seed, noise=0.1, video_t=0):
    g = np.random.default_rng(seed)
    shape = (b, c, video_t, h, w) if video_t else (b, c, h, w)
    x = (g.random(shape, dtype=np.float32) * 2 - 1).astype(np.float32)
    y = (x + noise * g.standard_normal(shape).astype(np.float32)).astype(np.float32)   # some values beyond +-1: decoders do not clamp
    return x, y


def _torch64(x, y, zero_mean, win=None):
    """eval_dist's torch restatement run in fp64 on the fp32-scaled inputs (the ssim_ref recipe)."""
    from pit_hip.eval_dist import _ms_ssim_torch, _ssim_torch, ssim_window

    win = ssim_window() if win is None else win
    X = torch.from_numpy(S.scale(x, zero_mean)).double()
    Y = torch.from_numpy(S.scale(y, zero_mean)).double()
    ssim = _ssim_torch(X, Y, win)[0].mean(1).numpy()
    if x.shape[-2] < 256 or x.shape[-1] < 256:
        return ssim, np.full_like(ssim, np.nan)
    return ssim, _ms_ssim_torch(X, Y, win).numpy()


def test_restatement_matches_scipy_gaussian_filter():
    """The ssim_map mean of ssim_ref against scipy.ndimage.gaussian_filter1d (sigma 1.5, truncate 5 / 1.5: an 11-tap fp64 window),
    cropped 5 px per border = the valid positions.  With ssim_ref given the fp64 window they agree to 1e-12."""
    from scipy.ndimage import gaussian_filter1d

    x, y = _pair(2, 3, 40, 57, 1)
    X, Y = S.scale(x, True).astype(np.float64), S.scale(y, True).astype(np.float64)

    def G(a):
        a = gaussian_filter1d(a, 1.5, axis=-2, truncate=5 / 1.5)
        a = gaussian_filter1d(a, 1.5, axis=-1, truncate=5 / 1.5)
        return a[..., 5:-5, 5:-5]

    mu1, mu2 = G(X), G(Y)
    s11, s22, s12 = G(X * X) - mu1 ** 2, G(Y * Y) - mu2 ** 2, G(X * Y) - mu1 * mu2
    cs = (2 * s12 + S.C2) / (s11 + s22 + S.C2)
    want = (((2 * mu1 * mu2 + S.C1) / (mu1 ** 2 + mu2 ** 2 + S.C1)) * cs).mean(axis=(-2, -1))
    got, _, smap = S.level(X, Y, S.window64())
    assert smap.shape == (2, 3, 30, 47)
    assert np.abs(got - want).max() <= 1e-12
    got32 = S.level(X, Y, S.window32())[0]
    print(f"fp32 window vs fp64 window: {np.abs(got32 - want).max():.3e}")
    assert 0 < np.abs(got32 - want).max() < 1e-5


def test_closed_forms():
    x, _ = _pair(2, 3, 256, 256, 2)
    s, m = S.ssim_msssim(x, x, zero_mean=True)
    np.testing.assert_allclose(s, 1.0, atol=1e-14)
    np.testing.assert_allclose(m, 1.0, atol=1e-14)
    # constant planes a and b under a unit-sum window: cs = 1 and ssim = (2ab + C1) / (a^2 + b^2 + C1)
    a, b = 100.0, 140.0
    X, Y = np.full((1, 2, 20, 30), a), np.full((1, 2, 20, 30), b)
    ss, cs, _ = S.level(X, Y, S.window64())
    np.testing.assert_allclose(cs, 1.0, atol=1e-12)
    np.testing.assert_allclose(ss, (2 * a * b + S.C1) / (a * a + b * b + S.C1), atol=1e-12)
    # the fp32 window (the reference's) sums to 1 only within its rounding: with s = sum(w)^2 (two passes) mu = a s and
    # G(XX) - mu^2 = a^2 s (1 - s), a small "variance" of a flat plane that the reference carries too
    s2 = float(np.sum(S.window32().astype(np.float64))) ** 2
    ss, cs, _ = S.level(X, Y, S.window32())
    v1, v2, v12 = a * a * s2 * (1 - s2), b * b * s2 * (1 - s2), a * b * s2 * (1 - s2)
    np.testing.assert_allclose(cs, (2 * v12 + S.C2) / (v1 + v2 + S.C2), rtol=1e-9)
    # strongly anti-correlated: cs < 0 at the finest level, relu -> 0, MS-SSIM 0
    s, m = S.ssim_msssim(x, -x, zero_mean=True)
    assert (s < 0).all() and (m == 0).all()
    from pit_hip.eval_dist import get_ssim_and_msssim

    ts, tm = get_ssim_and_msssim(torch.from_numpy(x), torch.from_numpy(-x), zero_mean=True)
    assert (tm == 0).all() and (ts < 0).all()


@pytest.mark.parametrize("shape,zero_mean", [((2, 3, 257, 263), True), ((2, 1, 256, 384), False), ((3, 3, 8, 40), True),
                                             ((2, 3, 32, 32), False), ((1, 3, 11, 11), True), ((2, 2, 1, 13), True)])
def test_torch_restatement_fp64_matches_reference(shape, zero_mean):
    """Odd sides at every level (257 x 263 -> 129 x 132 -> 65 x 66 -> 33 x 33 -> 17 x 17), non-square, a side under 11 (left
    unfiltered along it), below 256^2 (MS-SSIM NaN), a 1-pixel side."""
    from pit_hip.eval_dist import ssim_window

    x, y = _pair(*shape, seed=sum(shape))
    win = ssim_window()
    ws, wm = S.ssim_msssim(x, y, zero_mean, w=win.numpy())
    gs, gm = _torch64(x, y, zero_mean, win)
    assert np.abs(gs - ws).max() <= 1e-12
    if min(shape[2:]) >= 256:
        assert np.isfinite(wm).all() and np.abs(gm - wm).max() <= 1e-12
    else:
        assert np.isnan(wm).all() and np.isnan(gm).all()
    if shape[2] == 8:            # unfiltered along H: the map keeps all 8 rows
        assert S.level(S.scale(x, True), S.scale(y, True), win.numpy())[2].shape[-2:] == (8, 30)


@pytest.mark.parametrize("shape", [(4, 3, 256, 256), (2, 3, 257, 263), (2, 3, 64, 48)])
def test_torch_restatement_fp32_is_the_references_arithmetic(shape):
    """get_ssim_and_msssim on fp32 CPU tensors runs pytorch_msssim's fp32 op sequence: close to the fp64 restatement, and the
    gap is the reference's own rounding error (printed)."""
    from pit_hip.eval_dist import get_ssim, get_ssim_and_msssim

    x, y = _pair(*shape, seed=7)
    ws, wm = S.ssim_msssim(x, y, zero_mean=True)
    gs, gm = get_ssim_and_msssim(torch.from_numpy(x), torch.from_numpy(y), zero_mean=True)
    assert gs.dtype == torch.float32 and gs.shape == (shape[0],)
    ds = np.abs(gs.numpy() - ws).max()
    assert ds < 1e-4
    if shape[2] >= 256:
        dm = np.abs(gm.numpy() - wm).max()
        assert dm < 1e-4
        print(f"{shape}: fp32 torch vs fp64 ssim {ds:.2e}, ms-ssim {dm:.2e}")
    else:
        assert torch.isnan(gm).all()
    assert torch.equal(get_ssim(torch.from_numpy(x), torch.from_numpy(y), zero_mean=True), gs)


def test_video_averages_frames():
    from pit_hip.eval_dist import get_ssim, get_ssim_and_msssim

    x, y = _pair(2, 3, 20, 24, 5, video_t=3)
    ws, wm = S.ssim_msssim(x, y, zero_mean=True, is_video=True)
    gs, gm = get_ssim_and_msssim(torch.from_numpy(x), torch.from_numpy(y), zero_mean=True, is_video=True)
    assert gs.shape == (2,) and torch.isnan(gm).all() and np.isnan(wm).all()
    np.testing.assert_allclose(gs.numpy(), ws, atol=1e-4)
    per_frame = torch.stack([get_ssim(torch.from_numpy(x[:, :, t]), torch.from_numpy(y[:, :, t]), True) for t in range(3)])
    np.testing.assert_allclose(gs.numpy(), per_frame.mean(0).numpy(), atol=1e-6)
    xv, yv = _pair(1, 3, 256, 256, 6, video_t=2)
    ws, wm = S.ssim_msssim(xv, yv, zero_mean=False, is_video=True)
    gs, gm = get_ssim_and_msssim(torch.from_numpy(xv), torch.from_numpy(yv), zero_mean=False, is_video=True)
    np.testing.assert_allclose(gm.numpy(), wm, atol=1e-4)


def test_three_metric_step_record_layout():
    from pit_hip.eval_dist import StepRecord, get_ssim_and_msssim, psnr_zero_mean

    B, K = 3, 5
    lay = StepRecord(bs=B, tokens_per_image=K, n_metrics=3)
    x, y = _pair(B, 3, 256, 256, 9)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 65536, (B, 1, K), generator=g)
    rec = lay.pack_with_metrics(idx, x, y)
    assert rec.numel() == lay.words == 3 * B + (B * K + 1) // 2
    i2, m2 = lay.unpack(rec)
    s, m = get_ssim_and_msssim(x, y, zero_mean=True)
    assert torch.equal(i2, idx.reshape(B, K))
    assert torch.equal(m2, torch.stack([psnr_zero_mean(x, y), s, m], 1))
    assert torch.equal(rec[3 * B:], lay.pack(idx, m2)[3 * B:])
    with pytest.raises(ValueError):
        StepRecord(B, K, n_metrics=2).pack_with_metrics(idx, x, y)
    # the one-metric layout goes through pack_with_psnr unchanged
    one = StepRecord(B, K, n_metrics=1)
    assert torch.equal(one.pack_with_metrics(idx, x, y), one.pack_with_psnr(idx, x, y))


class _StubModel:
    """encode: indices derived from the image's id (its top-left value); decode: a fixed distortion of the image."""

    def encode(self, x, return_reg_log=True):
        ids = x[:, 0, 0, 0].round().long()
        tok = (ids[:, None] * 7 + torch.arange(4)[None]) % 65536
        return x, {"indices": tok.reshape(-1, 1, 2, 2)}

    def decode(self, z):
        return z * 0.75 + 0.1


def _images_for(ids, size=256):
    out = []
    for i in ids:
        g = torch.Generator().manual_seed(100 + i)
        x = torch.rand(3, size, size, generator=g) * 2 - 1
        x[0, 0, 0] = float(i)
        out.append(x)
    return torch.stack(out)


def _worker(rank, world, port, n, bs, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "vq-vae-from-gaussian-vae_amd"))
    from pit_hip.eval_dist import evaluate_sharded, init_from_env

    env = init_from_env("gloo")
    out = evaluate_sharded(_StubModel(), _images_for, n, bs, env["rank"], env["world"], torch.device("cpu"), 4,
                           metrics=("psnr", "ssim", "ms_ssim"))
    if rank == 0:
        q.put({k: v.numpy() for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_three_metrics_in_dataset_order():
    from pit_hip.eval_dist import get_ssim_and_msssim, psnr_zero_mean

    world, n, bs = 2, 7, 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, bs, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    total = (-(-n // world) // bs) * bs * world
    ids = [int(i) for i in np.arange(total) % n]
    x = _images_for(ids)
    xr = _StubModel().decode(x)
    s, m = get_ssim_and_msssim(x, xr, zero_mean=True)
    assert set(out) == {"indices", "psnr", "ssim", "ms_ssim"}
    assert np.array_equal(out["indices"], (np.array(ids)[:, None] * 7 + np.arange(4)[None]) % 65536)
    np.testing.assert_array_equal(out["psnr"], psnr_zero_mean(x, xr).numpy())
    np.testing.assert_array_equal(out["ssim"], s.numpy())
    np.testing.assert_array_equal(out["ms_ssim"], m.numpy())
    assert len(set(np.round(out["ssim"], 6))) > 1            # distinct per image: an order mistake would show


def test_evaluate_sharded_metrics_argument():
    from pit_hip.eval_dist import evaluate_sharded

    ids_for = lambda ids: _images_for(ids, size=16)      # noqa: E731
    out = evaluate_sharded(_StubModel(), ids_for, 3, 1, 0, 1, torch.device("cpu"), 4)
    assert set(out) == {"indices", "psnr"}
    out3 = evaluate_sharded(_StubModel(), ids_for, 3, 1, 0, 1, torch.device("cpu"), 4, metrics=("ms_ssim", "psnr", "ssim"))
    assert torch.equal(out3["psnr"], out["psnr"]) and torch.equal(out3["indices"], out["indices"])
    assert out3["ssim"].shape == (3,) and torch.isnan(out3["ms_ssim"]).all()
    with pytest.raises(ValueError):
        evaluate_sharded(_StubModel(), ids_for, 3, 1, 0, 1, torch.device("cpu"), 4, metrics=("lpips",))


def test_cabi_ssim_sizing_and_argument_checks():
    """Host-only halves of the entry points (no launch happens before these checks)."""
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = L.lib()
    assert lib.gq_ssim_workspace_bytes(0, 3, 256, 256) == -1 and lib.gq_ssim_workspace_bytes(2, 3, 0, 8) == -1
    five, one = lib.gq_ssim_workspace_bytes(16, 3, 256, 256), lib.gq_ssim_workspace_bytes(16, 3, 255, 256)
    assert five > one > 0                                 # below 256 only level 0: no pooled planes
    assert five >= 8 * 2 * 16 * 3 * (128 * 128 + 64 * 64)  # the two fp64 ping-pong buffers of levels 1 and 2
    rec3 = lib.gq_step_record_ssim_workspace_bytes(16, 3, 256, 256)
    assert rec3 >= five + lib.gq_step_record_workspace_bytes(16, 3 * 256 * 256)
    fake = 256                                           # never dereferenced: every call below fails its checks first
    assert lib.gq_ssim_f32(None, fake, 2, 3, 64, 64, 0, 1, fake, None, fake, 1 << 20, None) == 1
    assert lib.gq_ssim_f32(fake, fake, 2, 3, 64, 64, 2, 1, fake, None, fake, 1 << 20, None) == 1     # layout 2
    assert lib.gq_ssim_f32(fake, fake, 2, 3, 64, 64, 0, 1, fake, None, None, 1 << 20, None) == 2     # no workspace
    assert lib.gq_ssim_f32(fake, fake, 2, 3, 64, 64, 0, 1, fake, None, fake, 8, None) == 2           # too small
    assert lib.gq_ssim_f32(fake, fake, 2, 3, 64, 64, 0, 1, None, None, None, 0, None) == 0          # nothing asked
    assert lib.gq_step_record_ssim_f32(fake, fake, fake, fake, 2, 3, 64, 64, 0, 8, fake, 8, None) == 2
    assert lib.gq_step_record_ssim_f32(fake, fake, None, fake, 2, 3, 64, 64, 0, 8, fake, 1 << 20, None) == 1
