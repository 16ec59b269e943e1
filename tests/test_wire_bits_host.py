"""CPU: the bit-packed index wire format of the sharded eval path (pit_hip/eval_dist.py: pack_index_bits, StepRecord(n_codes=...),
evaluate_sharded(n_codes=...)) -- the torch packer against a bit-by-bit definition of the format, the w = 16 words against
the uint16 record, the record layout, and the eval loop at gloo world size 2 with indices up to 2^18 - 1."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

COUNTS = (1, 31, 32, 33, 63, 65)       # word-boundary straddles
N18 = 1 << 18


def _format_words(values, w):
    """The format's definition, bit by bit: index k's bit j is stream bit k w + j; stream bit p is bit p % 32 of word p // 32."""
    values = np.asarray(values, dtype=np.uint64)
    bits = ((values[:, None] >> np.arange(w, dtype=np.uint64)[None]) & np.uint64(1)).reshape(-1)
    bits = np.concatenate([bits, np.zeros(-bits.size % 32, dtype=np.uint64)])
    words = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)[None]).sum(1)
    return torch.from_numpy(words.astype(np.uint32).view(np.int32))


def _values(kind, count, w, seed):
    if kind == "ones":
        return torch.full((count,), (1 << w) - 1, dtype=torch.int64)
    if kind == "zeros":
        return torch.zeros(count, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 1 << w, (count,), generator=g, dtype=torch.int64)
    v[0] = (1 << w) - 1                  # the top bit of the first index is always exercised
    return v


@pytest.mark.parametrize("w", range(1, 33))
def test_torch_packer_round_trip_and_definition(w):
    from pit_hip.eval_dist import pack_index_bits, unpack_index_bits

    for count in COUNTS:
        for kind in ("random", "ones", "zeros"):
            v = _values(kind, count, w, seed=1000 * w + count)
            words = pack_index_bits(v, w)
            assert words.dtype == torch.int32 and words.numel() == (count * w + 31) // 32
            assert torch.equal(words, _format_words(v.numpy(), w)), (w, count, kind)
            assert torch.equal(unpack_index_bits(words, count, w), v), (w, count, kind)
    # leading dimensions unpack row by row
    a, b = _values("random", 33, w, 1), _values("random", 33, w, 2)
    both = torch.stack([pack_index_bits(a, w), pack_index_bits(b, w)])
    assert torch.equal(unpack_index_bits(both, 33, w), torch.stack([a, b]))


def test_out_of_range_values_keep_their_low_bits():
    from pit_hip.eval_dist import count_index_violations, pack_index_bits, unpack_index_bits

    v = torch.tensor([5, -1, 1 << 18, (1 << 18) + 3, (1 << 40) + 9, -(1 << 33) + 2, 7])
    assert torch.equal(unpack_index_bits(pack_index_bits(v, 18), 7, 18), v & (N18 - 1))
    assert int(count_index_violations(v, N18)) == 5
    assert int(count_index_violations(v, 6)) == 6          # 7 >= 6 too
    assert count_index_violations(v, N18).dtype == torch.int32


def test_sixteen_bits_are_the_legacy_pair_words():
    """w = 16 is exactly the uint16 "low half first" record: same index words from both layouts, even and odd counts."""
    from pit_hip.eval_dist import StepRecord, pack_index_bits

    g = torch.Generator().manual_seed(3)
    for bs, tokens in ((3, 5), (2, 8), (1, 1)):
        idx = torch.randint(0, 65536, (bs, tokens), generator=g)
        idx[0, 0], idx[-1, -1] = 65535, 32768
        met = torch.randn(bs, 2, generator=g)
        old, new = StepRecord(bs, tokens, 2), StepRecord(bs, tokens, 2, n_codes=65536)
        r_old, r_new = old.pack(idx, met), new.pack(idx, met)
        assert new.index_bits == 16 and new.index_words == old.index_words and new.words == old.words + 1
        assert torch.equal(r_new[:-1], r_old) and int(r_new[-1]) == 0
        assert torch.equal(pack_index_bits(idx.reshape(-1), 16), r_old[old.metric_words:])
        assert torch.equal(old.unpack(r_old)[0], new.unpack(r_new)[0])


@pytest.mark.parametrize("bs,tokens", [(3, 5), (1, 1), (2, 8)])
def test_uint16_record_masks_indices_outside_its_domain(bs, tokens):
    """Outside the documented domain (values < 2^16) a uint16 record packed without the range check carries each index's low 16
    bits -- the words of pack_index_bits(., 16), which are the kernel's -- and no index spills into its neighbour's half-word."""
    from pit_hip.eval_dist import StepRecord, pack_index_bits

    flat = torch.randint(0, 65536, (bs * tokens,), generator=torch.Generator().manual_seed(bs * 100 + tokens))
    flat[0] = 65536 + 7
    if flat.numel() > 1:
        flat[-1], flat[1], flat[-2] = -1, -1, 65536 + 7       # an even and an odd position each
    lay = StepRecord(bs, tokens, 2, check_range=False)
    met = torch.randn(bs, 2, generator=torch.Generator().manual_seed(1))
    rec = lay.pack(flat.reshape(bs, tokens), met)
    assert rec.numel() == lay.words and torch.equal(rec[lay.metric_words:], pack_index_bits(flat, 16))
    idx, m2 = lay.unpack(rec)
    assert torch.equal(idx.reshape(-1), flat & 0xFFFF) and torch.equal(m2, met)
    if flat.numel() == 1:                                     # (1, 1) holds one index: the other value in a record of its own
        rec = lay.pack(torch.tensor([[-1]]), met)
        assert torch.equal(rec[lay.metric_words:], pack_index_bits(torch.tensor([-1]), 16))
        assert lay.unpack(rec)[0].tolist() == [[0xFFFF]]


def test_record_layout_words_and_violations_word():
    from pit_hip.eval_dist import StepRecord, index_bits_for

    assert [index_bits_for(n) for n in (1, 2, 3, 4, 5, 1024, 1025, 65536, 65537, N18, 1 << 23, 1 << 32)] == \
        [1, 1, 2, 2, 3, 10, 11, 16, 17, 18, 23, 32]
    with pytest.raises(ValueError):
        index_bits_for(0)
    with pytest.raises(ValueError):
        index_bits_for((1 << 32) + 1)
    for n_codes, bs, tokens, n_metrics in ((N18, 3, 5, 1), (1000, 4, 7, 3), (1 << 32, 2, 3, 2), (2, 3, 11, 1), (512 * 2, 16, 256, 1)):
        lay = StepRecord(bs, tokens, n_metrics, n_codes=n_codes)
        w = max(1, (n_codes - 1).bit_length())
        assert lay.index_bits == w and lay.metric_words == bs * n_metrics
        assert lay.index_words == -(-bs * tokens * w // 32)
        assert lay.words == bs * n_metrics + lay.index_words + 1
        g = torch.Generator().manual_seed(n_codes % 977)
        idx = torch.randint(0, n_codes, (bs, 1, tokens), generator=g)
        idx[0, 0, 0] = n_codes - 1
        met = torch.randn(bs, n_metrics, generator=g)
        rec = lay.pack(idx, met)
        assert rec.dtype == torch.int32 and rec.numel() == lay.words and int(rec[-1]) == 0
        i2, m2 = lay.unpack(rec)
        assert torch.equal(i2, idx.reshape(bs, tokens)) and torch.equal(m2, met)
        # a stack of records unpacks along the last dimension, and the violations words come back per record
        bad = idx.clone()
        bad[-1, 0, -1], bad[0, 0, 0] = n_codes, -1
        two = torch.stack([rec, lay.pack(bad, met)])
        i3, m3 = lay.unpack(two)
        assert torch.equal(i3[0], i2) and torch.equal(m3[1], met)
        assert lay.violations(two).tolist() == [0, 2]
        assert torch.equal(i3[1], bad.reshape(bs, tokens) & ((1 << w) - 1))       # packed as their low w bits
    # the 1024-code codebook of the last case: 10 bits per token instead of 16
    assert StepRecord(16, 256, 1, n_codes=1024).index_words == 1280 < StepRecord(16, 256, 1).index_words == 2048
    with pytest.raises(ValueError):
        StepRecord(2, 2, 1).violations(torch.zeros(4, dtype=torch.int32))


def test_running_histogram_from_packed_records_skips_values_past_n():
    from pit_hip.eval_dist import StepRecord

    n_codes = 5                          # 3 bits: the packed values 5, 6, 7 exist but are no codes
    lay = StepRecord(2, 6, 1, n_codes=n_codes)
    idx = torch.tensor([[0, 1, 4, 4, 4, 2], [7, 5, 3, 3, 0, 6]])
    met = torch.zeros(2, 1)
    hist = torch.zeros(n_codes, dtype=torch.int64)
    lay.add_to_histogram(torch.stack([lay.pack(idx, met), lay.pack(idx.flip(1), met)]), hist)
    lay.add_to_histogram(lay.pack(idx, met), hist)
    assert hist.tolist() == [6, 3, 3, 6, 9]


# ----------------------------------------------------------------------------- the eval loop, gloo world 2
class _WideModel:
    """encode: indices derived from the image content, reaching 2^18 - 1 (image 0, token 0); ``bad`` = (image id, value): that
    image's last token becomes ``value``."""

    def __init__(self, bad=None):
        self.bad = bad

    @staticmethod
    def tokens(ids):
        return (N18 - 1 - (ids[:, None] * 7919 + torch.arange(4)[None] * 30011)) % N18

    def encode(self, x, return_reg_log=True):
        ids = x[:, 0, 0, 0].round().long()
        tok = self.tokens(ids)
        if self.bad is not None:
            tok[ids == self.bad[0], 3] = self.bad[1]
        return x, {"indices": tok.reshape(-1, 1, 2, 2)}

    def decode(self, z):
        return z * 0.5


def _images_for(ids):
    x = torch.zeros(len(ids), 3, 4, 4)
    for k, i in enumerate(ids):
        x[k] = float(i)
    return x


def _worker(rank, world, port, n, bs, bad, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "vq-vae-from-gaussian-vae_amd"))
    from pit_hip.eval_dist import evaluate_sharded, init_from_env

    env = init_from_env("gloo")
    try:
        out = evaluate_sharded(_WideModel(bad), _images_for, n, bs, env["rank"], env["world"], torch.device("cpu"), 4,
                               n_codes=N18)
        msg = {k: v.numpy() for k, v in out.items()} if rank == 0 else None
    except ValueError as e:
        msg = {"error": str(e)}
    if rank == 0:
        q.put(msg)
    dist.barrier()
    dist.destroy_process_group()


def _run_world(world, n, bs, bad=None):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, bs, bad, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return out


def test_two_rank_gloo_eval_with_a_two_to_the_eighteen_codebook():
    """Indices up to 2^18 - 1 through the one gather per step: dataset order with the sampler's wrap, the whole-set histogram equal
    to torch.bincount of what came back, usage / entropy from cal_ent.  (The uint16 record raises ValueError on the first batch.)"""
    from pit_hip.eval_dist import cal_ent

    n, bs = 37, 4
    out = _run_world(2, n, bs)
    assert "error" not in out, out
    steps = -(-n // 2) // bs
    total = steps * bs * 2
    want_ids = torch.arange(total) % n                    # dataset order (the sampler wraps when it pads)
    want_tok = _WideModel.tokens(want_ids)
    assert int(want_tok.max()) == N18 - 1 and int(want_tok.max()) >= 65536
    assert np.array_equal(out["indices"], want_tok.numpy())
    assert out["psnr"].shape == (total,)
    want_hist = torch.bincount(want_tok.reshape(-1), minlength=N18)
    assert out["hist"].dtype == np.int64 and out["hist"].shape == (N18,)
    assert np.array_equal(out["hist"], want_hist.numpy()) and int(out["hist"].sum()) == total * 4
    usage, ent = cal_ent(want_hist)
    assert float(out["usage"]) == float(usage) and float(out["entropy"]) == float(ent)


def test_two_rank_gloo_eval_reports_the_rank_and_step_of_a_violation():
    """Image 13 is rank 1's (13 % 2), its 7th item -> step 6 // 4 = 1: every rank raises after the loop, naming both."""
    out = _run_world(2, 37, 4, bad=(13, N18))
    assert set(out) == {"error"}, out
    assert "rank 1" in out["error"] and "step 1" in out["error"] and "1 indices" in out["error"], out["error"]


def test_single_rank_eval_raises_after_the_loop_for_a_negative_index():
    from pit_hip.eval_dist import evaluate_sharded

    calls = []

    def images_for(ids):
        calls.append(list(ids))
        return _images_for(ids)

    with pytest.raises(ValueError, match=r"rank 0, step 2: 1 indices outside \[0, 262144\)"):
        evaluate_sharded(_WideModel(bad=(5, -3)), images_for, 12, 2, 0, 1, torch.device("cpu"), 4, n_codes=N18)
    assert len(calls) == 6               # the loop ran to its end first: no per-step check
    out = evaluate_sharded(_WideModel(), images_for, 12, 2, 0, 1, torch.device("cpu"), 4, n_codes=N18)
    assert torch.equal(out["indices"], _WideModel.tokens(torch.arange(12)))
    assert torch.equal(out["hist"], torch.bincount(out["indices"].reshape(-1), minlength=N18))


def test_without_n_codes_the_loop_still_refuses_wide_indices():
    """The default path is untouched: uint16 record, per-step range check."""
    from pit_hip.eval_dist import evaluate_sharded

    with pytest.raises(ValueError, match="65536"):
        evaluate_sharded(_WideModel(), _images_for, 12, 2, 0, 1, torch.device("cpu"), 4)
