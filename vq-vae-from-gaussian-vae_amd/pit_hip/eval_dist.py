"""Image-sharded evaluation over RCCL / xGMI (one process per GPU).

Re-expression of the reference's ``eval.py`` data path (eval.py:78-107 process
group + DistributedSampler sharding, :144-205 per-batch encode -> decode ->
metric -> all_gather, :207-257 rank-0 re-interleave).  What changes:

* the reference issues six small ``all_gather``s per batch (PSNR, SSIM, MS-SSIM,
  LPIPS, two Inception feature blocks; eval.py:166-201); every one is latency
  bound on xGMI.  Here each rank packs everything it wants to publish for the
  batch -- the code indices as uint16 (2^16-entry codebook) bit-cast into the
  same buffer as the fp32 per-image metrics -- into ONE int32 record and the
  step does ONE ``all_gather_into_tensor``.
  A codebook of any other size (``n_codes``, up to 2^32) takes the bit-packed
  record instead: bit_length(n_codes - 1) bits per index, a violations word in
  place of the per-step host range check, and a whole-set usage histogram
  accumulated on rank 0 from the gathered words.
* records stay on the device; nothing is copied to the host until the end.
* no data-path collective besides that gather: images are independent, the
  4 MiB codebook and the weights are replicated (regenerated from the seed).
* SSIM and MS-SSIM (eval.py:170-178, pit/evaluations/ssim.py) ride in the same
  record (``metrics=("psnr", "ssim", "ms_ssim")``): still one gather per step.
* FID (eval.py:186-203, 241-259; ``fid_features=...``): instead of two more
  gathers and two host copies per step and 2 N 2048 features kept on the host,
  each rank folds its feature blocks into fp64 raw moments on its own device
  (pit_hip/evaluations/fid/fid_score.py) and the ranks meet ONCE, after the loop.

Sharding semantics are exactly ``DistributedSampler(shuffle=False)`` (pads the
index list by wrapping so every rank gets ceil(N/W) items) followed by a
``drop_last=True`` loader, and the restore order is ``[j % W][j // W]``
(eval.py:213-214).  Works with backend "nccl" (= RCCL on ROCm) and "gloo".
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist
import torch.nn.functional as F


# ----------------------------------------------------------------------------- sharding
def sampler_indices(n: int, world: int, rank: int) -> List[int]:
    """DistributedSampler(shuffle=False, drop_last=False) index list of ``rank``."""
    if n <= 0:
        return []
    total = -(-n // world) * world
    idx = list(range(n))
    pad = total - n
    if pad > 0:
        reps = -(-pad // n)
        idx += (idx * reps)[:pad]
    return idx[rank:total:world]


def shard_batches(n: int, world: int, rank: int, bs: int) -> List[List[int]]:
    """Batches of dataset indices rank ``rank`` evaluates (loader drop_last=True)."""
    ids = sampler_indices(n, world, rank)
    return [ids[i:i + bs] for i in range(0, len(ids) - bs + 1, bs)]


def reinterleave(per_rank: Sequence[torch.Tensor]) -> torch.Tensor:
    """per_rank[r] is the concatenation (over steps) of rank r's per-image rows.
    Returns rows in dataset order: out[j] = per_rank[j % W][j // W] (eval.py:213-214)."""
    w = len(per_rank)
    stacked = torch.stack(list(per_rank), dim=1)  # [items_per_rank, W, ...]
    return stacked.reshape((stacked.shape[0] * w,) + tuple(stacked.shape[2:]))


# ----------------------------------------------------------------------------- process group
def init_from_env(backend: Optional[str] = None) -> Dict[str, int]:
    """env:// rendezvous (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), one rank per GPU."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        kwargs = {}
        if backend == "nccl":
            kwargs["device_id"] = torch.device("cuda", local_rank)
        dist.init_process_group(backend=backend, init_method="env://", rank=rank, world_size=world, **kwargs)
    return {"rank": rank, "local_rank": local_rank, "world": world}


# ----------------------------------------------------------------------------- packed record
def index_bits_for(n_codes: int) -> int:
    """Bits per index of the bit-packed wire format for a codebook of ``n_codes`` entries: the width of n_codes - 1, at least 1."""
    if not 1 <= n_codes <= 1 << 32:
        raise ValueError(f"the bit-packed wire format takes 1 <= n_codes <= 2^32, got {n_codes}")
    return max(1, (n_codes - 1).bit_length())


def _wrap_i32(words: torch.Tensor) -> torch.Tensor:
    """int64 values in [0, 2^32) as the int32 words of the same 32 bits."""
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)


def pack_index_bits(flat: torch.Tensor, index_bits: int) -> torch.Tensor:
    """The bit-packed index stream in torch expressions (any device; no host read): index k of the int64 vector ``flat`` -- its
    low ``index_bits`` bits, the value taken as unsigned 32-bit -- occupies bits [k w, (k + 1) w) of a little-endian bit stream
    over int32 words (stream bit p = bit p mod 32 of word p div 32), zero-padded to a whole word.  w = 16 is the "low half
    first" uint16 pair format.  The words gq_indices_pack_bits writes, bit for bit."""
    w = index_bits
    if not 1 <= w <= 32:
        raise ValueError(f"index_bits is in 1..32, got {w}")
    count = flat.numel()
    n_words = (count * w + 31) // 32
    v = flat.reshape(-1).to(torch.int64) & ((1 << w) - 1)
    p = torch.arange(count, dtype=torch.int64, device=flat.device) * w
    word, off = p >> 5, p & 31
    c = v << off                                   # < 2^63: at most 32 value bits shifted by at most 31
    acc = torch.zeros(n_words + 1, dtype=torch.int64, device=flat.device)
    acc.index_add_(0, word, c & 0xFFFFFFFF)        # the fields are disjoint bit ranges: the sum is their OR
    acc.index_add_(0, word + 1, c >> 32)
    return _wrap_i32(acc[:n_words])


def unpack_index_bits(words: torch.Tensor, count: int, index_bits: int) -> torch.Tensor:
    """Inverse of pack_index_bits along the last dimension: int32 [..., >= ceil(count w / 32)] -> int64 [..., count], each value
    in [0, 2^w)."""
    w = index_bits
    if not 1 <= w <= 32:
        raise ValueError(f"index_bits is in 1..32, got {w}")
    n_words = (count * w + 31) // 32
    u = words[..., :n_words].to(torch.int64) & 0xFFFFFFFF
    u = torch.cat([u, u.new_zeros(u.shape[:-1] + (1,))], dim=-1)
    p = torch.arange(count, dtype=torch.int64, device=words.device) * w
    word, off = p >> 5, p & 31
    lo, hi = u.index_select(-1, word), u.index_select(-1, word + 1)
    hi = hi & ((torch.ones_like(off) << off) - 1)  # a straddling index takes fewer than `off` bits of the next word
    return ((lo >> off) | (hi << (32 - off))) & ((1 << w) - 1)


def count_index_violations(flat: torch.Tensor, n_codes: int) -> torch.Tensor:
    """The record's violations word: how many indices lie outside [0, n_codes), saturated at 2^31 - 1; a 0-d int32 tensor."""
    bad = ((flat < 0) | (flat >= n_codes)).sum()
    return bad.clamp(max=(1 << 31) - 1).to(torch.int32)


class StepRecord:
    """Layout of one rank's per-step record: int32 words =
    [ per-image metrics as fp32 bits (bs * n_metrics) | indices as uint16 pairs ]
    or, with ``n_codes`` (any codebook size up to 2^32), the bit-packed record
    [ per-image metrics as fp32 bits | ceil(bs tokens w / 32) index words (pack_index_bits) | 1 violations word ]
    with w = index_bits_for(n_codes).  The violations word counts this record's indices outside [0, n_codes) (such an index is
    packed as its low w bits); nothing is read on the host while packing."""

    def __init__(self, bs: int, tokens_per_image: int, n_metrics: int, check_range: bool = False,
                 n_codes: Optional[int] = None) -> None:
        """``check_range``: validate 0 <= index < 2^16 on every pack (a device->host sync: eval drivers set it, the
        benchmark's timed loop does not -- its codebook has exactly 2^16 entries).  ``n_codes``: None keeps that uint16 format;
        an integer selects the bit-packed record, whose range check is the violations word (``check_range`` is not used)."""
        self.bs, self.tokens, self.n_metrics = bs, tokens_per_image, n_metrics
        self.check_range = check_range
        self.n_codes = n_codes
        self.metric_words = bs * n_metrics
        self.index_bits = 16 if n_codes is None else index_bits_for(n_codes)
        self.index_words = (bs * tokens_per_image * self.index_bits + 31) // 32
        self.words = self.metric_words + self.index_words + (n_codes is not None)
        self._ws = {}        # the library's zeroed, self-resetting workspaces (_lib.step_record)

    def _check_counts(self, who: str, indices: torch.Tensor, n_items: int, items: str, want_items: int) -> None:
        if indices.numel() != self.bs * self.tokens or n_items != want_items:
            raise ValueError(f"StepRecord.{who}: got {indices.numel()} indices / {n_items} {items}, layout is "
                             f"{self.bs} x {self.tokens} / {want_items}")

    def pack(self, indices: torch.Tensor, metrics: torch.Tensor) -> torch.Tensor:
        """indices: int64 [bs, ...] with values < 2^16 (< n_codes in the bit-packed record); metrics: fp32 [bs, n_metrics].  The
        index words are the stream of pack_index_bits in both formats (w = 16: the uint16 pairs), so an index outside the stated
        range is packed as its low w bits; gq_indices_pack_bits writes them on a HIP device, the torch expressions elsewhere."""
        flat = indices.reshape(-1)
        self._check_counts("pack", flat, metrics.numel(), "metrics", self.metric_words)
        if self.n_codes is None and self.check_range:
            _check_index_range(flat)
        rec = torch.empty(self.words, dtype=torch.int32, device=indices.device)
        rec[: self.metric_words] = metrics.reshape(-1).to(torch.float32).view(torch.int32)
        end = self.metric_words + self.index_words
        viol = rec[end:] if self.n_codes is not None else None
        if flat.is_cuda and flat.dtype == torch.int64:
            from . import _lib

            _lib.indices_pack_bits(flat, self.index_bits, self.n_codes or 1 << 16, rec[self.metric_words: end], viol)
        else:
            rec[self.metric_words: end] = pack_index_bits(flat, self.index_bits)
            if viol is not None:
                viol[0] = count_index_violations(flat, self.n_codes)
        return rec

    def _pack_on_device(self, indices: torch.Tensor, x: torch.Tensor, x_rec: torch.Tensor) -> Optional[torch.Tensor]:
        """The finished record from ONE library call (_lib.step_record: the metrics of (x, x_rec; zero_mean), the index words and
        the violations word), or None where the kernels do not apply: off a HIP device, or for images / indices they do not take
        (_lib.step_record_ok; three metrics: images brought to one dense layout first, and _lib.ssim_ok).
        Which PSNR a record carries is observable -- the kernel sums in fp64, torch's mean in fp32 -- and ``check_range`` (the
        uint16 record's host read of the indices' range; the bit-packed record has its violations word instead) decides it by one
        rule: a uint16 record with ``check_range`` and ONE metric is not packed here but by the torch expressions (pack() checks
        the range); with THREE metrics the range is checked on the host here and the kernels run."""
        host_check = self.n_codes is None and self.check_range
        if not indices.is_cuda or (host_check and self.n_metrics == 1):
            return None
        from . import _lib

        self._check_counts("pack_with_psnr" if self.n_metrics == 1 else "pack_with_metrics", indices, x.shape[0], "images", self.bs)
        if self.n_metrics == 3:
            x, x_rec = _dense_pair(x, x_rec)
        if not _lib.step_record_ok(x, x_rec, indices) or (self.n_metrics == 3 and not _lib.ssim_ok(x, x_rec)):
            return None
        if host_check:
            _check_index_range(indices.reshape(-1))
        rec = torch.empty(self.words, dtype=torch.int32, device=indices.device)
        return _lib.step_record(x, x_rec, indices, rec, self._ws, self.n_metrics,
                                None if self.n_codes is None else self.index_bits, self.n_codes)

    def pack_with_psnr(self, indices: torch.Tensor, x: torch.Tensor, x_rec: torch.Tensor) -> torch.Tensor:
        """pack(indices, psnr_zero_mean(x, x_rec)) for the one-metric layout.  On a HIP device: ONE launch of libgqhip
        (gq_step_record_f32 / gq_step_record_bits_f32: the PSNR reduction and the index packing in the same kernel) instead of
        the ~13 elementwise / reduction kernels of the torch expressions; elsewhere exactly those expressions."""
        rec = self._pack_on_device(indices, x, x_rec) if self.n_metrics == 1 else None
        return rec if rec is not None else self.pack(indices, psnr_zero_mean(x, x_rec)[:, None])

    def pack_with_metrics(self, indices: torch.Tensor, x: torch.Tensor, x_rec: torch.Tensor) -> torch.Tensor:
        """pack(indices, metrics of (x, x_rec) with zero_mean) for the one-metric layout (PSNR: pack_with_psnr) or the
        three-metric one (PSNR, SSIM, MS-SSIM per image: eval.py:165-178).  Three metrics on a HIP device: ONE library call
        (gq_step_record_ssim_f32 / gq_step_record_ssim_bits_f32, whose PSNR and index words are those of pack_with_psnr bit for
        bit); elsewhere, or for a layout the kernels do not take, the torch expressions."""
        if self.n_metrics == 1:
            return self.pack_with_psnr(indices, x, x_rec)
        if self.n_metrics != 3:
            raise ValueError(f"StepRecord.pack_with_metrics: n_metrics is 1 (psnr) or 3 (psnr, ssim, ms_ssim), not {self.n_metrics}")
        rec = self._pack_on_device(indices, x, x_rec)
        if rec is not None:
            return rec
        ssim, ms = get_ssim_and_msssim(x, x_rec, zero_mean=True)
        return self.pack(indices, torch.stack([psnr_zero_mean(x, x_rec), ssim.to(torch.float32), ms.to(torch.float32)], 1))

    def unpack(self, rec: torch.Tensor):
        """rec: int32 [..., words] -> (indices int64 [..., bs, tokens], metrics fp32 [..., bs, n_metrics]); gq_indices_unpack_bits
        on a HIP device, unpack_index_bits elsewhere, both formats."""
        lead = rec.shape[:-1]
        metrics = rec[..., : self.metric_words].contiguous().view(torch.float32).reshape(*lead, self.bs, self.n_metrics)
        count = self.bs * self.tokens
        if rec.is_cuda:
            from . import _lib

            flat = _lib.indices_unpack_bits(rec.reshape(-1, self.words), self.metric_words, count, self.index_bits)
        else:
            flat = unpack_index_bits(rec[..., self.metric_words: self.metric_words + self.index_words], count, self.index_bits)
        return flat.reshape(*lead, self.bs, self.tokens), metrics

    def violations(self, rec: torch.Tensor) -> torch.Tensor:
        """rec: int32 [..., words] of the bit-packed record -> its violations words, int32 [...]."""
        if self.n_codes is None:
            raise ValueError("StepRecord.violations: the uint16 record has no violations word")
        return rec[..., -1]

    def add_to_histogram(self, rec: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
        """hist (int64 [n_codes]) += the index counts of the bit-packed records rec (int32 [..., words]); a packed value >= n_codes
        is skipped.  On a HIP device the kernel reads the packed words (gq_index_histogram_packed: no int64 indices are formed);
        elsewhere torch expressions.  No host read."""
        if self.n_codes is None:
            raise ValueError("StepRecord.add_to_histogram: needs the bit-packed record (n_codes)")
        if rec.is_cuda:
            from . import _lib

            return _lib.index_histogram_packed(rec.reshape(-1, self.words), self.metric_words, self.bs * self.tokens,
                                               self.index_bits, hist)
        flat = unpack_index_bits(rec[..., self.metric_words: -1], self.bs * self.tokens, self.index_bits).reshape(-1)
        ok = (flat < self.n_codes).to(torch.int64)
        hist.index_add_(0, flat.clamp(max=self.n_codes - 1), ok)
        return hist


def _check_index_range(flat: torch.Tensor) -> None:
    if flat.numel() and (int(flat.max()) >= 65536 or int(flat.min()) < 0):
        raise ValueError("StepRecord.pack: the uint16 wire format needs 0 <= index < 65536")


def gather_step(rec: torch.Tensor, world: int, always_collective: bool = False) -> torch.Tensor:
    """ONE collective per step: [words] -> [world, words].  ``always_collective`` issues the
    all-gather even for a single rank (tests use it to drive RCCL on a one-GPU box)."""
    if world == 1 and not always_collective:
        return rec[None]
    rec = rec.reshape(-1)
    if rec.is_cuda and dist.get_backend() == "gloo":   # debug configuration: gloo gathers through the host
        host = torch.empty(world * rec.numel(), dtype=rec.dtype)
        dist.all_gather_into_tensor(host, rec.cpu())
        return host.to(rec.device).reshape(world, -1)
    out = torch.empty(world * rec.numel(), dtype=rec.dtype, device=rec.device)
    dist.all_gather_into_tensor(out, rec)  # concatenated along dim 0 (works on RCCL and gloo)
    return out.reshape(world, -1)


def get_psnr(x_input: torch.Tensor, x_recon: torch.Tensor, zero_mean: bool = False, is_video: bool = False) -> torch.Tensor:
    """pit/evaluations/psnr.py:17-35: PSNR per item on the [0, 255] scale; ``zero_mean``: inputs in [-1, 1]
    (eval.py:165 calls it that way), else in [0, 1].  Same op order as the reference (golden g12_psnr)."""
    if zero_mean:
        a, b = (x_input + 1) * 127.5, (x_recon + 1) * 127.5
    else:
        a, b = x_input * 255, x_recon * 255
    mse = torch.mean((a - b) ** 2, dim=[1, 2, 3, 4] if is_video else [1, 2, 3])
    return 20 * torch.log10(255.0 / torch.sqrt(mse))


def psnr_zero_mean(x: torch.Tensor, x_rec: torch.Tensor) -> torch.Tensor:
    """get_psnr(zero_mean=True), per image."""
    return get_psnr(x, x_rec, zero_mean=True)


# ----------------------------------------------------------------------------- SSIM / MS-SSIM
# pit/evaluations/ssim.py:5-63 calls pytorch_msssim (1.0) with data_range 255 and size_average False.  On a HIP device the images
# go to gq_ssim_f32 (csrc/gq_ssim.h: fp64 moments and maps, one launch per scale); elsewhere -- and for layouts the kernel does
# not take -- _ssim_torch / _ms_ssim_torch restate pytorch_msssim's op sequence (grouped conv2d with the fp32 window, avg_pool2d)
# in the inputs' dtype.
_MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_SSIM_WS: Dict[tuple, dict] = {}      # per (device, stream): the library's self-resetting workspaces


def ssim_window(size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """pytorch_msssim's 1-D Gaussian window: exp(-(k - size // 2)^2 / (2 sigma^2)) in fp32, divided by its sum."""
    coords = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _gaussian_filter(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """Separable 'valid' filter per channel: along H, then W; a side shorter than the window is skipped."""
    c = x.shape[1]
    out = x
    for i, s in enumerate(x.shape[2:]):
        if s >= win.numel():
            w = win.reshape(1, 1, 1, -1).repeat(c, 1, 1, 1).transpose(2 + i, -1)
            out = F.conv2d(out, w, stride=1, padding=0, groups=c)
    return out


def _ssim_torch(X: torch.Tensor, Y: torch.Tensor, win: torch.Tensor, data_range: float = 255.0):
    """One scale: (ssim, cs) per (image, channel), in X's dtype."""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    win = win.to(X.device, dtype=X.dtype)
    mu1, mu2 = _gaussian_filter(X, win), _gaussian_filter(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = _gaussian_filter(X * X, win) - mu1_sq
    sigma2_sq = _gaussian_filter(Y * Y, win) - mu2_sq
    sigma12 = _gaussian_filter(X * Y, win) - mu1_mu2
    cs_map = (2 * sigma12 + c2) / (sigma1_sq + sigma2_sq + c2)
    ssim_map = ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1), torch.flatten(cs_map, 2).mean(-1)


def _ms_ssim_torch(X: torch.Tensor, Y: torch.Tensor, win: torch.Tensor, data_range: float = 255.0) -> torch.Tensor:
    """Five scales joined by avg_pool2d(2, padding = side % 2); per image."""
    weights = torch.tensor(_MS_WEIGHTS, dtype=torch.float32).to(X)     # the reference's fp32 weights, whatever X's dtype
    mcs = []
    for i in range(len(_MS_WEIGHTS)):
        ssim_pc, cs = _ssim_torch(X, Y, win, data_range)
        if i < len(_MS_WEIGHTS) - 1:
            mcs.append(torch.relu(cs))
            padding = [s % 2 for s in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=padding)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=padding)
    vals = torch.stack(mcs + [torch.relu(ssim_pc)], dim=0)
    return torch.prod(vals ** weights.view(-1, 1, 1), dim=0).mean(1)


def _scale(x: torch.Tensor, zero_mean: bool) -> torch.Tensor:
    return (x + 1) * 127.5 if zero_mean else x * 255


def _frames(x: torch.Tensor, is_video: bool) -> torch.Tensor:
    """[B, C, T, H, W] -> [B * T, C, H, W] (image-major); images pass through."""
    if not is_video:
        return x
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)


def _dense_pair(a: torch.Tensor, b: torch.Tensor):
    """HIP fp32 image batches in ONE dense layout, so the kernels take them: b follows a's layout (a channels_last decoder output
    against NCHW inputs costs one copy, not a fall-back); other tensors pass through."""
    from . import _lib

    if not (a.is_cuda and b.is_cuda and a.dim() == 4 and a.shape == b.shape and a.dtype == b.dtype == torch.float32):
        return a, b
    la = _lib.image_layout(a)
    if la is None:
        a, la = a.contiguous(), 0
    if _lib.image_layout(b) != la:
        b = b.contiguous(memory_format=torch.channels_last if la == 1 else torch.contiguous_format)
    return a, b


def _image_quality(x_input: torch.Tensor, x_recon: torch.Tensor, zero_mean: bool, is_video: bool, msssim: bool):
    """(ssim, ms_ssim or None) per item; video items average their frames."""
    a, b = _dense_pair(_frames(x_input, is_video), _frames(x_recon, is_video))
    from . import _lib

    if _lib.ssim_ok(a, b):
        key = (a.device, torch.cuda.current_stream(a.device).cuda_stream)
        ssim, ms = _lib.image_quality(a, b, zero_mean, msssim, _SSIM_WS.setdefault(key, {}))
    else:
        X, Y = _scale(a, zero_mean), _scale(b, zero_mean)
        win = ssim_window()
        ssim = _ssim_torch(X, Y, win)[0].mean(1)
        ms = _ms_ssim_torch(X, Y, win) if msssim else None
    if is_video:
        n = x_input.shape[0]
        ssim = ssim.reshape(n, -1).mean(1)
        ms = ms.reshape(n, -1).mean(1) if ms is not None else None
    return ssim, ms


def get_ssim(x_input: torch.Tensor, x_recon: torch.Tensor, zero_mean: bool = False, is_video: bool = False) -> torch.Tensor:
    """pit/evaluations/ssim.py:5-27: SSIM per item on the [0, 255] scale (``zero_mean``: inputs in [-1, 1], else [0, 1]);
    ``is_video``: [B, C, T, H, W], the frames' mean."""
    return _image_quality(x_input, x_recon, zero_mean, is_video, msssim=False)[0]


def get_ssim_and_msssim(x_input: torch.Tensor, x_recon: torch.Tensor, zero_mean: bool = False, is_video: bool = False):
    """pit/evaluations/ssim.py:30-63: (SSIM, MS-SSIM) per item; MS-SSIM is NaN when H or W is under 256."""
    h, w = x_input.shape[2 + is_video], x_input.shape[3 + is_video]
    if h < 256 or w < 256:
        ssim = get_ssim(x_input, x_recon, zero_mean, is_video)
        return ssim, torch.ones_like(ssim) * torch.nan
    return _image_quality(x_input, x_recon, zero_mean, is_video, msssim=True)


def cal_ent(hist: torch.Tensor):
    """eval.py:137-141 (dead code there): codebook usage (fraction of entries hit at least once)
    and entropy in bits of the usage histogram, with the reference's ``+ 1e-5`` inside the log.  Returns
    (usage, entropy) as 0-d tensors on hist's device."""
    hist = hist.to(torch.float32)
    unused = torch.sum((hist == 0).to(dtype=torch.float32)) / hist.shape[0]
    p = hist / torch.sum(hist)
    ent = -torch.sum(p * torch.log2(p + 1e-5))
    return 1 - unused, ent


def codebook_usage(indices: torch.Tensor, n_codes: int):
    """Histogram (HIP kernel, eval.py:127,152-154's all_hist) + cal_ent of a batch of indices on the device."""
    from . import _lib

    hist = _lib.index_histogram(indices.contiguous(), n_codes)
    usage, ent = cal_ent(hist)
    return hist, usage, ent


class FidAccumulator:
    """One rank's Frechet statistics of the inputs and of the reconstructions (eval.py:186-203 without its two gathers and two
    host copies per step).  ``features``: a callable images -> fp32 [B, D] or [B, D, h, w] (pooled as eval.py:188-190 pools);
    D is taken from the first call.  The raw moments are additive over images, so the ranks meet ONCE, after the loop."""

    def __init__(self, features) -> None:
        self.features = features
        self.stats = None                     # [FrechetStats of the inputs, of the reconstructions], made at the first step

    def update(self, x: torch.Tensor, x_rec: torch.Tensor) -> None:
        from .evaluations.fid.fid_score import FrechetStats

        blocks = [self.features(x), self.features(x_rec)]
        if self.stats is None:
            self.stats = [FrechetStats(f.shape[1], f.device) for f in blocks]
        for stats, feats in zip(self.stats, blocks):
            stats.update(feats)

    def reduce(self, world: int) -> None:
        """Every rank's two states summed in rank order, on every rank: ONE all_gather_into_tensor of the stacked
        [2, D D + D + 1] fp64 states (not all_reduce, whose order is not fixed).  Every rank must call it; ranks without a step
        (then no rank has one: the sampler gives every rank the same number of batches) have nothing to gather."""
        if world == 1 or self.stats is None:
            return
        both = gather_step(torch.stack([s.state for s in self.stats]), world).reshape(world, 2, -1)
        for k, stats in enumerate(self.stats):
            stats.state.zero_()
            stats.merge_(both[r, k] for r in range(world))

    def result(self) -> Dict[str, object]:
        """{"fid", "fid_count"}: the reference's mean / covariance / calculate_frechet_distance (eval.py:241-259) of everything
        folded in; the count includes the items the sampler wrapped around (eval.py:205, total_num)."""
        from .evaluations.fid.fid_score import calculate_frechet_distance

        (n, mu_x, cov_x), (_, mu_r, cov_r) = (s.moments() for s in self.stats)
        return {"fid": calculate_frechet_distance(mu_r, cov_r, mu_x, cov_x), "fid_count": n}


@torch.no_grad()
def sharded_eval_steps(model, images_for, batches, layout: StepRecord, world: int, device,
                       hist: Optional[torch.Tensor] = None, fid: Optional["FidAccumulator"] = None) -> List[torch.Tensor]:
    """The per-step loop of evaluate_sharded: encode / decode / pack / ONE gather per batch of ``batches``; returns the gathered
    [world, words] records, one per step.  ``hist`` (int64 [n_codes], bit-packed records only): each gathered record's indices are
    added to it as they arrive.  ``fid`` (a FidAccumulator): the features of every batch and of its reconstruction are folded into
    this rank's two FrechetStats -- no collective, no host read.  With a bit-packed ``layout`` nothing in the loop reads the device
    from the host."""
    gathered = []
    for ids in batches:
        x = images_for(ids).to(device, non_blocking=True)
        zhat, info = model.encode(x, return_reg_log=True)
        rec_img = model.decode(zhat)
        if layout.n_metrics == 1:
            rec = layout.pack_with_psnr(info["indices"], x, rec_img)
        else:
            rec = layout.pack_with_metrics(info["indices"], x, rec_img)
        gathered.append(gather_step(rec, world))
        if hist is not None:
            layout.add_to_histogram(gathered[-1], hist)
        if fid is not None:
            fid.update(x, rec_img)
    return gathered


@torch.no_grad()
def evaluate_sharded(model, images_for, n_images: int, bs: int, rank: int, world: int, device,
                     tokens_per_image: int, metrics: Sequence[str] = ("psnr",),
                     n_codes: Optional[int] = None, fid_features=None) -> Optional[Dict[str, torch.Tensor]]:
    """The reference eval loop for this path: each rank encodes/decodes its shard, one gather per
    step, rank 0 returns indices + PSNR in dataset order.  ``images_for(ids) -> [len(ids),3,H,W]``.
    ``metrics``: ("psnr",) or ("psnr", "ssim", "ms_ssim") (eval.py:165-178; any order): the three-metric record, still ONE
    gather per step, and "ssim" / "ms_ssim" in the result too.
    ``n_codes``: None keeps the uint16 record and its per-step range check (a host read per step; indices < 2^16).  An integer
    (1 .. 2^32) selects the bit-packed record of StepRecord(n_codes=...): max(1, bit_length(n_codes - 1)) bits per index on the
    wire, no host read inside the loop; every rank checks the gathered violations words once after the loop and raises
    ValueError naming the first (rank, step) whose indices left [0, n_codes).  Rank 0 also accumulates the whole evaluated
    set's usage histogram from the gathered records (eval.py:127,152-154's all_hist; the items the sampler wraps around to pad
    the last batch count, as they do in "indices") and the result gains "hist" (int64 [n_codes]), "usage" and "entropy"
    (cal_ent: eval.py:137-141).
    ``fid_features``: None, or a callable images -> fp32 [B, D] or [B, D, h, w] (eval.py:186-203's inception_v3(img)[0]).  Each
    step calls it on the batch and on its reconstruction and folds the features into two per-rank FrechetStats on the device
    (pit_hip/evaluations/fid/fid_score.py): the step keeps its ONE gather, with no new collective and no host read.  After the loop
    every rank takes part in ONE all-gather of the stacked states, summed in rank order, and rank 0's result gains "fid" (a
    float: calculate_frechet_distance of the reconstructions' statistics against the inputs', eval.py:241-259) and "fid_count"
    (the rows behind it; the wrapped items count, as in eval.py:205)."""
    names = set(metrics)
    if names == {"psnr"}:
        n_metrics = 1
    elif names == {"psnr", "ssim", "ms_ssim"}:
        n_metrics = 3
    else:
        raise ValueError(f"evaluate_sharded: metrics are ('psnr',) or ('psnr', 'ssim', 'ms_ssim'), got {tuple(metrics)}")
    batches = shard_batches(n_images, world, rank, bs)
    hist = None
    if n_codes is None:
        layout = StepRecord(bs, tokens_per_image, n_metrics=n_metrics, check_range=True)
    else:
        layout = StepRecord(bs, tokens_per_image, n_metrics=n_metrics, n_codes=n_codes)
        if rank == 0:
            hist = torch.zeros(n_codes, dtype=torch.int64, device=device)
    fid = None if fid_features is None else FidAccumulator(fid_features)
    gathered = sharded_eval_steps(model, images_for, batches, layout, world, device, hist, fid)
    if fid is not None:
        fid.reduce(world)      # a collective: before any rank returns
    if not gathered or (rank != 0 and n_codes is None):
        return None
    if n_codes is not None:
        viol = torch.stack([layout.violations(g) for g in gathered], dim=1).cpu()   # [W, steps]: the ONE host read of the range check
        bad = torch.nonzero(viol)
        if bad.numel():
            r, s = (int(v) for v in bad[0])
            raise ValueError(f"evaluate_sharded: rank {r}, step {s}: {int(viol[r, s])} indices outside [0, {n_codes}) "
                             f"({bad.shape[0]} rank-steps in all)")
    if rank != 0:
        return None
    allrec = torch.stack(gathered, dim=1)  # [W, steps, words]
    idx, met = layout.unpack(allrec)       # [W, steps, bs, tokens], [W, steps, bs, n_metrics]
    per_rank_idx = [idx[r].reshape(-1, tokens_per_image) for r in range(world)]
    out = {"indices": reinterleave(per_rank_idx)}
    if n_metrics == 1:
        out["psnr"] = reinterleave([met[r].reshape(-1) for r in range(world)])
    else:
        for k, name in enumerate(("psnr", "ssim", "ms_ssim")):
            out[name] = reinterleave([met[r][..., k].reshape(-1) for r in range(world)])
    if n_codes is not None:
        out["hist"] = hist
        out["usage"], out["entropy"] = cal_ent(hist)
    if fid is not None:
        out.update(fid.result())
    return out
