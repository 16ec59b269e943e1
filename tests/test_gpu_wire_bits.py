"""-m gpu: the bit-packed index wire format on the device (gqhip.h: gq_indices_pack_bits / gq_indices_unpack_bits /
gq_index_histogram_packed / gq_step_record_bits_f32 / gq_step_record_ssim_bits_f32) against the torch packer of
pit_hip/eval_dist.py (itself pinned to the format's definition by tests/test_wire_bits_host.py), the uint16 records, and the eval
loop around a real 2^17-entry VQQuantizer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 0x5A5A5A5A


def _L():
    from pit_hip import _lib

    return _lib


def _rand_idx(count, w, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 1 << w, (count,), generator=g, dtype=torch.int64)
    v[0], v[-1] = (1 << w) - 1, (1 << w) - 1
    return v


def _pack_guarded(idx_dev, w, n_codes):
    """gq_indices_pack_bits into a buffer with guard words behind the stream and around the violations word."""
    L = _L()
    n_words = (idx_dev.numel() * w + 31) // 32
    buf = torch.full((n_words + 8,), GUARD, dtype=torch.int32, device=DEV)
    viol = torch.full((3,), GUARD, dtype=torch.int32, device=DEV)
    L.indices_pack_bits(idx_dev, w, n_codes, buf[:n_words], viol[1:2])
    assert bool((buf[n_words:] == GUARD).all()) and int(viol[0]) == GUARD == int(viol[2])
    return buf[:n_words], int(viol[1])


@pytest.mark.parametrize("w", range(1, 33))
def test_kernel_packer_equals_the_torch_packer_word_for_word(w):
    """Every width at 1, 33 and 4097 indices (4097: more than one LDS pass for w <= 3, more than one block for w >= 2), and the
    unpack kernel back, from a field that sits at an offset inside a wider row."""
    from pit_hip.eval_dist import pack_index_bits

    L = _L()
    for count in (1, 33, 4097):
        v = _rand_idx(count, w, 77 * w + count)
        want = pack_index_bits(v, w)
        got, viol = _pack_guarded(v.to(DEV), w, 1 << w)
        assert torch.equal(got.cpu(), want), (w, count)
        assert viol == 0
        rows = torch.full((2, want.numel() + 5), GUARD, dtype=torch.int32, device=DEV)
        rows[0, 3: 3 + want.numel()] = got
        rows[1, 3: 3 + want.numel()] = pack_index_bits(v.flip(0), w).to(DEV)
        back = L.indices_unpack_bits(rows, 3, count, w)
        assert back.dtype == torch.int64 and torch.equal(back.cpu(), torch.stack([v, v.flip(0)])), (w, count)


@pytest.mark.parametrize("w", [1, 3, 5, 7, 11, 18, 31])
def test_kernel_packer_over_many_blocks_counts_each_violation_once(w):
    """20 011 indices: several 256-word blocks whose boundaries fall inside an index (8192 % w != 0 except w = 1).  Negative and
    >= n_codes indices are injected -- among them the indices that straddle a block boundary -- and are packed as their low w
    bits; the count is exact."""
    from pit_hip.eval_dist import count_index_violations, pack_index_bits

    count, n_codes = 20011, (1 << w) - (1 if w > 1 else 0)
    g = torch.Generator().manual_seed(w)
    v = torch.randint(0, n_codes, (count,), generator=g, dtype=torch.int64)
    got, viol = _pack_guarded(v.to(DEV), w, n_codes)
    assert torch.equal(got.cpu(), pack_index_bits(v, w)) and viol == 0
    hits = sorted({0, count - 1, 4097} | {b * 8192 // w for b in range(1, count * w // 8192 + 1)})
    for j, k in enumerate(hits):
        v[k] = (-1 - j, n_codes + j, (1 << 40) + j)[j % 3]
    want_viol = int(count_index_violations(v, n_codes))
    assert want_viol == len(hits)
    got, viol = _pack_guarded(v.to(DEV), w, n_codes)
    assert torch.equal(got.cpu(), pack_index_bits(v, w))
    assert viol == want_viol


def test_pack_arguments_are_checked_on_the_host():
    L = _L()
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    for w, n_codes in ((0, 1), (33, 5), (4, 17), (4, 0)):            # width out of 1..32, n_codes > 2^w, n_codes < 1
        with pytest.raises(L.GqHipError, match="invalid"):
            L.indices_pack_bits(idx, w, n_codes)
    rows = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(L.GqHipError, match="invalid"):               # the field leaves the row: 2 + ceil(5 * 18 / 32) > 4
        L.indices_unpack_bits(rows, 2, 5, 18)
    with pytest.raises(L.GqHipError, match="invalid"):
        L.index_histogram_packed(rows, 2, 5, 18, torch.zeros(8, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------ the records
def _images(B, C, H, W, cl, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, C, H, W, generator=g) * 2 - 1).to(DEV)
    xr = (x + 0.05 * torch.randn(B, C, H, W, generator=g).to(DEV)).clamp(-1, 1)
    if cl:
        x, xr = x.contiguous(memory_format=torch.channels_last), xr.contiguous(memory_format=torch.channels_last)
    return x, xr


def _ws_is_zero(lay):
    return all(int(t.count_nonzero()) == 0 for t in lay._ws.values())


@pytest.mark.parametrize("cl", [False, True])
def test_psnr_record_words_equal_the_uint16_record_bit_for_bit(cl):
    """B = 3, 3 x 32 x 32: the PSNR words of gq_step_record_bits_f32 are those of gq_step_record_f32 for every width tried; the
    index words are the torch packer's; n_codes = 65536 reproduces the uint16 record's index words; the workspace is all zero
    behind every call."""
    from pit_hip.eval_dist import StepRecord, pack_index_bits

    B, T = 3, 37                                                      # 111 indices: an odd count
    x, xr = _images(B, 3, 32, 32, cl, 5)
    old = StepRecord(B, T, 1)
    for n_codes in (65536, 1 << 18, 1000, 2, 1 << 32):
        new = StepRecord(B, T, 1, n_codes=n_codes)
        idx = torch.randint(0, min(n_codes, 65536), (B, 1, T), generator=torch.Generator().manual_seed(n_codes % 1013)).to(DEV)
        r_old = old.pack_with_psnr(idx, x, xr)
        for _ in range(2):                                            # the second call runs in the workspace the first left
            r_new = new.pack_with_psnr(idx, x, xr)
        assert r_new.numel() == new.words and torch.equal(r_new[:B], r_old[:B]), n_codes
        assert torch.equal(r_new[B:-1].cpu(), pack_index_bits(idx.reshape(-1).cpu(), new.index_bits)) and int(r_new[-1]) == 0
        if n_codes == 65536:
            assert torch.equal(r_new[B:-1], r_old[B:])
        assert torch.equal(new.unpack(r_new)[0].reshape(-1), idx.reshape(-1))
        assert _ws_is_zero(new) and len(new._ws) == 1
        # pack(): the metrics handed over, the index words from gq_indices_pack_bits
        r_pack = new.pack(idx, new.unpack(r_new)[1])
        assert torch.equal(r_pack, r_new)


def test_three_metric_record_words_equal_the_uint16_record_bit_for_bit():
    """B = 2, 3 x 256 x 256 (the smallest size with a finite MS-SSIM): all six metric words."""
    from pit_hip.eval_dist import StepRecord, pack_index_bits

    B, T = 2, 256
    x, xr = _images(B, 3, 256, 256, True, 9)
    idx = torch.randint(0, 1 << 18, (B, 1, 16, 16), generator=torch.Generator().manual_seed(2)).to(DEV)
    old, new = StepRecord(B, T, 3), StepRecord(B, T, 3, n_codes=1 << 18)
    r_old = old.pack_with_metrics(idx & 0xFFFF, x, xr)
    for _ in range(2):
        r_new = new.pack_with_metrics(idx, x, xr)
    assert torch.equal(r_new[: 3 * B], r_old[: 3 * B])
    assert bool(torch.isfinite(new.unpack(r_new)[1]).all())
    assert torch.equal(r_new[3 * B: -1].cpu(), pack_index_bits(idx.reshape(-1).cpu(), 18)) and int(r_new[-1]) == 0
    assert _ws_is_zero(new)
    new16 = StepRecord(B, T, 3, n_codes=65536)
    assert torch.equal(new16.pack_with_metrics(idx & 0xFFFF, x, xr)[:-1], r_old)


def _raw_record(x, xr, idx, w, n_codes, ws):
    """gq_step_record_bits_f32 on a caller's workspace, into a record with guard words behind it."""
    L = _L()
    B, per = x.shape[0], x[0].numel()
    words = B + (idx.numel() * w + 31) // 32 + 1
    rec = torch.full((words + 8,), GUARD, dtype=torch.int32, device=DEV)
    rc = L.lib().gq_step_record_bits_f32(x.data_ptr(), xr.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, per, idx.numel(), w, n_codes,
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and bool((rec[words:] == GUARD).all())
    return rec[:words]


def test_record_workspace_is_left_zero_and_serves_a_shorter_last_batch():
    """One workspace sized for B = 5 (two PSNR chunks per image), then the short last batch of B = 2 in the same bytes: the same
    words as from a fresh workspace, all zero behind each call; a workspace 8 bytes short (the uint16 record's size) is refused."""
    L = _L()
    x, xr = _images(5, 3, 64, 48, False, 11)                          # 9216 floats per image: 2 chunks
    per = x[0].numel()
    idx = torch.randint(0, 1 << 20, (5 * 48,), generator=torch.Generator().manual_seed(4)).to(DEV)
    idx[7], idx[100] = -5, 1 << 20
    need = L.lib().gq_step_record_bits_workspace_bytes(5, per)
    assert need == L.lib().gq_step_record_workspace_bytes(5, per) + 8
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    full = _raw_record(x, xr, idx, 20, 1 << 20, ws)
    assert int(ws.count_nonzero()) == 0 and int(full[-1]) == 2
    short = _raw_record(x[:2], xr[:2], idx[:96], 20, 1 << 20, ws)
    assert int(ws.count_nonzero()) == 0 and int(short[-1]) == 1
    fresh = _raw_record(x[:2], xr[:2], idx[:96], 20, 1 << 20, torch.zeros(need, dtype=torch.uint8, device=DEV))
    assert torch.equal(short, fresh) and torch.equal(short[:2], full[:2])
    again = _raw_record(x, xr, idx, 20, 1 << 20, ws)
    assert torch.equal(again, full) and int(ws.count_nonzero()) == 0
    rec = torch.zeros(full.numel(), dtype=torch.int32, device=DEV)
    rc = L.lib().gq_step_record_bits_f32(x.data_ptr(), xr.data_ptr(), idx.data_ptr(), rec.data_ptr(), 5, per, idx.numel(), 20, 1 << 20,
                                         ws.data_ptr(), need - 8, torch.cuda.current_stream().cuda_stream)
    assert rc == 2                                                    # GQHIP_ERR_WORKSPACE
    # no indices at all: the violations word is still written
    none = _raw_record(x[:1], xr[:1], idx[:0], 20, 1 << 20, ws)
    assert none.numel() == 2 and int(none[-1]) == 0 and torch.equal(none[:1], full[:1])


def test_record_violations_word_counts_injected_indices_exactly():
    from pit_hip.eval_dist import StepRecord

    B, T, n_codes = 3, 2731, 200000                                   # 18 bits; 8193 indices: 19 packing blocks
    x, xr = _images(B, 3, 32, 32, False, 21)
    idx = torch.randint(0, n_codes, (B, T), generator=torch.Generator().manual_seed(8))
    lay = StepRecord(B, T, 1, n_codes=n_codes)
    assert int(lay.pack_with_psnr(idx.to(DEV), x, xr)[-1]) == 0
    bad = idx.clone().reshape(-1)
    where = torch.randperm(bad.numel(), generator=torch.Generator().manual_seed(9))[:301]
    bad[where[:100]] = -1 - torch.arange(100)
    bad[where[100:200]] = n_codes + torch.arange(100)                 # some of them still fit 18 bits
    bad[where[200:]] = (1 << 33) + torch.arange(101)
    rec = lay.pack_with_psnr(bad.reshape(B, T).to(DEV), x, xr)
    assert int(rec[-1]) == 301
    assert torch.equal(lay.unpack(rec)[0].reshape(-1).cpu(), bad & ((1 << 18) - 1))
    assert int(lay.pack_with_psnr(idx.to(DEV), x, xr)[-1]) == 0        # the count does not leak into the next call
    assert torch.equal(lay.pack(bad.reshape(B, T).to(DEV), torch.zeros(B, 1, device=DEV))[B:], rec[B:])


@pytest.mark.parametrize("bs,tokens,n_metrics", [(3, 5, 1), (3, 5, 3), (1, 1, 1)])
def test_uint16_records_unpack_on_the_device_as_in_torch(bs, tokens, n_metrics):
    """The uint16 record takes the unpack kernel too (w = 16): a [2, words] stack, odd counts, the index field at word 3 / 9 / 1."""
    from pit_hip.eval_dist import StepRecord, unpack_index_bits

    lay = StepRecord(bs, tokens, n_metrics)
    g = torch.Generator().manual_seed(bs * 10 + n_metrics)
    idx = torch.randint(0, 65536, (2, bs, tokens), generator=g)
    idx[0, 0, 0], idx[1, -1, -1] = 65535, 32768
    met = torch.randn(2, bs, n_metrics, generator=g)
    stack = torch.stack([lay.pack(idx[r], met[r]) for r in range(2)])
    assert stack.shape == (2, lay.words)
    got_idx, got_met = lay.unpack(stack.to(DEV))
    want_idx, want_met = lay.unpack(stack)
    assert torch.equal(want_idx, idx) and torch.equal(want_idx.reshape(2, -1), unpack_index_bits(stack[:, lay.metric_words:], bs * tokens, 16))
    assert got_idx.dtype == torch.int64 and torch.equal(got_idx.cpu(), want_idx)
    assert torch.equal(got_met.cpu(), want_met)


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("B,C,H,W,T", [(3, 3, 5, 7, 5), (2, 3, 64, 48, 3), (1, 3, 256, 256, 4)])
def test_one_step_record_wrapper_serves_every_format_and_metric_count(B, C, H, W, T, cl):
    """_lib.step_record through uint16 / bits x one / three metrics on ONE ws_cache: per_image not a multiple of 4 with one chunk and
    an odd index count; two PSNR chunks with a NaN MS-SSIM; five SSIM levels behind the record's head.  Index and violations
    words: the torch packers, exactly.  PSNR: the torch expression within 2e-6 (fp64 sum of the reference's fp32 terms vs torch's
    fp32 mean; test_step_record_one_launch_matches_the_torch_expressions) and the same bits from all four; SSIM / MS-SSIM: the bits
    of get_ssim_and_msssim (test_three_metric_record), NaN included.  Every workspace is all zero behind the calls, and serves a
    smaller B."""
    from pit_hip.eval_dist import (count_index_violations, get_ssim_and_msssim, index_bits_for, pack_index_bits,
                                   psnr_zero_mean)

    L = _L()
    x, xr = _images(B, C, H, W, cl, B * 100 + H)
    want_psnr = psnr_zero_mean(x, xr)
    ssim, ms = get_ssim_and_msssim(x, xr, zero_mean=True)
    assert bool(torch.isnan(ms).all()) == (H < 256)
    idx = torch.randint(0, 65536, (B, T), generator=torch.Generator().manual_seed(T)).to(DEV)
    idx[0, 0], idx[-1, -1] = 65535, 65536 + 3                        # the last one: out of range for n_codes = 65536 only
    flat = idx.reshape(-1).cpu()
    ws_cache, psnr_words = {}, []
    for n_metrics in (1, 3):
        for n_codes in (None, 65536, 1 << 18):
            w = 16 if n_codes is None else index_bits_for(n_codes)
            n_words = (B * T * w + 31) // 32
            rec = torch.full((B * n_metrics + n_words + (n_codes is not None) + 4,), GUARD, dtype=torch.int32, device=DEV)
            for _ in range(2):                                        # the second call runs in the workspace the first left
                out = L.step_record(x, xr, idx, rec[:-4], ws_cache, n_metrics, None if n_codes is None else w, n_codes)
            assert out.data_ptr() == rec.data_ptr() and bool((rec[-4:] == GUARD).all())
            m = B * n_metrics
            assert torch.equal(rec[m: m + n_words].cpu(), pack_index_bits(flat, w)), (n_metrics, n_codes)
            if n_codes is not None:
                assert int(rec[m + n_words]) == int(count_index_violations(flat, n_codes)) == (n_codes == 65536)
            psnr_words.append(rec[0:m:n_metrics].clone())
            if n_metrics == 3:
                assert torch.equal(rec[1:m:3], ssim.view(torch.int32)) and torch.equal(rec[2:m:3], ms.view(torch.int32))
    assert all(torch.equal(p, psnr_words[0]) for p in psnr_words)
    torch.testing.assert_close(psnr_words[0].view(torch.float32), want_psnr, rtol=2e-6, atol=0)
    assert len(ws_cache) == 4 and all(int(t.count_nonzero()) == 0 for t in ws_cache.values())
    if B > 1:                                                         # a smaller B: its own entries of the same cache
        short = torch.empty(3 * (B - 1) + ((B - 1) * T * 18 + 31) // 32 + 1, dtype=torch.int32, device=DEV)
        L.step_record(x[:B - 1], xr[:B - 1], idx[:B - 1], short, ws_cache, 3, 18, 1 << 18)
        assert torch.equal(short[0:3 * (B - 1):3], psnr_words[0][:B - 1])
        assert torch.equal(short[1:3 * (B - 1):3], ssim[:B - 1].view(torch.int32))
        assert torch.equal(short[3 * (B - 1): -1].cpu(), pack_index_bits(flat[:(B - 1) * T], 18)) and int(short[-1]) == 0
        assert len(ws_cache) == 5 and all(int(t.count_nonzero()) == 0 for t in ws_cache.values())


def test_packed_histogram_equals_bincount():
    """n = 2^18, two records, w = 18, the field 3 words into rows wider than the field; it ADDS to hist; with a smaller n the values
    >= n are skipped."""
    from pit_hip.eval_dist import pack_index_bits

    L = _L()
    n, w, count = 1 << 18, 18, 5001
    g = torch.Generator().manual_seed(12)
    a = torch.randint(0, n, (count,), generator=g)
    b = torch.cat([torch.randint(0, 50, (count - 1,), generator=g), torch.tensor([n - 1])])      # a contended corner of the table
    field = (count * w + 31) // 32
    rows = torch.randint(-(1 << 31), 1 << 31, (2, field + 9), generator=g, dtype=torch.int64).to(torch.int32)
    rows[0, 3: 3 + field], rows[1, 3: 3 + field] = pack_index_bits(a, w), pack_index_bits(b, w)
    rows = rows.to(DEV)
    want = torch.bincount(torch.cat([a, b]), minlength=n)
    hist = torch.zeros(n, dtype=torch.int64, device=DEV)
    L.index_histogram_packed(rows, 3, count, w, hist)
    assert torch.equal(hist.cpu(), want)
    L.index_histogram_packed(rows[1:], 3, count, w, hist)
    assert torch.equal(hist.cpu(), want + torch.bincount(b, minlength=n))
    small = torch.zeros(200000, dtype=torch.int64, device=DEV)
    L.index_histogram_packed(rows, 3, count, w, small)
    assert torch.equal(small.cpu(), want[:200000])


# ------------------------------------------------------------------------------------------ the eval loop around a real quantiser
class _VQModel:
    """Identity encoder / decoder around VQQuantizer(n = 2^17, dim = 4): z is the image itself ([B, 4, 4, 4]: 16 tokens)."""

    def __init__(self, q):
        self.q = q

    def encode(self, x, return_reg_log=True):
        return self.q(x)

    def decode(self, z):
        return z


def test_eval_loop_with_a_real_vq_quantiser_of_131072_codes():
    from pit_hip import eval_dist as E
    from pit_hip.quantization.vq import VQQuantizer

    n, n_images, bs, T = 1 << 17, 10, 2, 16
    torch.manual_seed(31)
    q = VQQuantizer("bchw", n, 4)
    q.embedding.weight.data.normal_()
    images = torch.randn(n_images, 4, 4, 4, generator=torch.Generator().manual_seed(32))
    # the CPU computation: nearest code in fp64, index order [B, h, w]
    rows = images.permute(0, 2, 3, 1).reshape(-1, 4).double()
    want_idx = torch.cdist(rows, q.embedding.weight.data.double()).argmin(1).reshape(n_images, T)
    assert int(want_idx.max()) >= 65536
    want_hist = torch.bincount(want_idx.reshape(-1), minlength=n)
    want_usage, want_ent = E.cal_ent(want_hist)

    q = q.eval().to(DEV)
    model, dev_images = _VQModel(q), images.to(DEV)

    def images_for(ids):
        return dev_images[torch.as_tensor(ids)]

    out = E.evaluate_sharded(model, images_for, n_images, bs, 0, 1, DEV, T, n_codes=n)
    assert torch.equal(out["indices"].cpu(), want_idx)
    assert out["hist"].dtype == torch.int64 and torch.equal(out["hist"].cpu(), want_hist)
    assert float(out["usage"]) == float(want_usage)
    # entropy: a sum of same-sign fp32 terms, each a few ulp off between the CPU's and the device's log2, reduced in another order
    assert abs(float(out["entropy"]) - float(want_ent)) <= 1e-5 * float(want_ent)
    want_psnr = E.psnr_zero_mean(dev_images, q.embedding.weight.data[want_idx.to(DEV)].reshape(n_images, 4, 4, 4).permute(0, 3, 1, 2))
    torch.testing.assert_close(out["psnr"], want_psnr, rtol=2e-6, atol=0)
    # the loop itself never reads the device from the host (workspaces and the codebook cache were sized by the run above)
    layout = E.StepRecord(bs, T, 1, n_codes=n)
    hist = torch.zeros(n, dtype=torch.int64, device=DEV)
    batches = E.shard_batches(n_images, 1, 0, bs)
    idx_dev = [torch.as_tensor(b, device=DEV) for b in batches]
    for strict in (False, True):                                      # the first pass sizes this layout's workspace
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error" if strict else "default")
        try:
            it = iter(idx_dev)
            gathered = E.sharded_eval_steps(model, lambda ids: dev_images[next(it)], batches, layout, 1, DEV, hist)
            if strict:                                                # the mode is live: a host read in this window raises
                with pytest.raises(RuntimeError):
                    hist[0].item()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    assert len(layout._ws) == 1                                       # the records came from gq_step_record_bits_f32
    assert torch.equal(hist.cpu(), 2 * want_hist)
    assert torch.equal(layout.unpack(torch.stack(gathered, 1))[0].reshape(-1, T).cpu(), want_idx)
