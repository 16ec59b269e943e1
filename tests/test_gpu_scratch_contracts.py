"""-m gpu: the scratch-memory contracts of include/gqhip.h, call after call.

The rest of the suite checks single calls on fresh buffers.  This module checks what a call may find in its scratch and what it
leaves there: (1) the don't-care workspace of the arg-max family and of the attention backward gives bit-equal results whatever it
held before, (2) one Workspace walked through a sequence of different calls equals fresh ones, (3) a call touches exactly its
`*_workspace_bytes` and lays them out from its shape, not from the size it is handed, (4) the zero-in / zero-out workspace of the
metric calls is ALL zero behind every call, so that one allocation serves a stream of calls with any batch that fits.

Write-before-read table of the don't-care workspace (csrc/gqhip.hip:ws_layout, csrc/gq_common.h:WsHeader), from reading the
kernels; "L1" is the call's first launch (gq_prep_kernel; dims without a filter: a fill of the header + prep_plain_kernel), "L2" the
filter (grid path: index builder + search), "L3" the re-rank (grid path: the finish kernel).  A word that no launch of the call
reads is "-".

  WsHeader field            written by                                     read by
  fb_count                  L1 block 0 (= 0); exhaustive: the fill         L3 atomicAdd; grid: search appends, finish reads; debug_counters
  reranked, grid_leaves     L1 block 0 (= 0); exhaustive: the fill         L3 / search atomicAdd (debug statistics only); debug_*
  grid_next                 L1 block 0 (= 0)                               -
  loss_ticket               L1 block 0 (= 0); exhaustive: the fill         vq_loss_kernel (after the arg-min) atomicAdd
  ste_kind, ste, pure       L1 block 0 / prep_plain thread 0               every store of zhat (ste_mix) in L3 / search / finish / exhaustive
  absmax_part, r2_part      L1, all 256 code blocks, one word each         L3 / search (wave_absmax over the 256)
  cbsum                     L1, all 256 code blocks                        grid index builder (stamps the cache)
  gs                        L1 block 0 (rows = 0 when there is no block)   the statistics block inside L3
  loss_part[k]              vq_loss_kernel block k, before its ticket      the last block of the same launch, k < gridDim only
  stamps, pads              diagnostic builds only                         -

  region (ws_layout)        written by                                     read by
  rec                       L2: every (record set < rec_sets, row < rows)  L3, the same range; grid path: the undecided-row lists
                                                                           (und_row / und_thr / und_margin), entries < fb_count only
  fb                        -                                              - (the exhaustive kernel runs with all_rows: no list)
  dbg                       diagnostic builds only                         -
  mu, sd, lsd               L1 row blocks, rows < rows (from-z entries; plain rows: lsd only, when the caller passes none)
                                                                           L2 fp32 filter / L3 / search / exhaustive, rows < rows
  rowsum, coef              L1 row blocks, rows < rows                     L3 / search, rows < rows (dead lanes mirror the last row)
  cbimg (no image cache)    L1 code blocks: tiles < tiles_total (the ragged tile zero-padded)
                                                                           L2: chunks run into the CT padding tiles, which are
                                                                           staged through LDS but never multiplied (nt tiles only)
  rowimg, rowscale, rowaux  L1 row blocks, rows < rows                     L2 (row index clamped to rows - 1) / L3
  kl2                       L1 (from-z, gq_quantize_z_gauss_f32 only)      the statistics block / gauss_stats_finalize_kernel, rows < rows
  zrows of vq_quantize_z    = the mu region above                          vq_loss_kernel

  gq_mha_bwd_f32: n | D [B, H, L] written by mha_bwd_dq_f32_kernel for every row < L, read by mha_bwd_dkdv_f32_kernel for rows < L.

The reading found no word that a call reads before it has written it; the fills below (0xFF: NaN floats and -1 counters, random
bytes, the leftovers of another call) are the check of that reading.  The zero-in / zero-out workspace was different: before this
module the step record left its partial sums behind (see part 4)."""
import contextlib
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import ssim_ref as S
from oracle import gq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096          # guard bytes on either side of a workspace (a multiple of the 256-byte alignment the library asks for)
SENT = 0xA5
LAM0 = (1.0, 1.0, 1.0)


# ------------------------------------------------------------------------------------------ plumbing
_STOP = {"why": None}


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    """A HIP error met by one test ends the module: nothing more is launched on a device that has faulted."""
    if _STOP["why"]:
        pytest.fail(f"not run: an earlier test of this module met a GPU fault ({_STOP['why']})")
    yield
    try:                             # (a fault may also surface in a test's own reads of the device)
        torch.cuda.synchronize()
    except Exception as e:
        _STOP["why"] = repr(e)


@pytest.fixture(autouse=True, scope="module")
def _debug_counters_on():
    from pit_hip import _lib

    _lib.debug_enable(True)
    yield
    _lib.debug_enable(False)
    _lib.set_filter("auto")


def _sync():
    try:
        torch.cuda.synchronize()
    except Exception as e:           # an illegal access surfaces here
        _STOP["why"] = repr(e)
        raise


@contextlib.contextmanager
def _filter(kind):
    from pit_hip import _lib

    prev = _lib.get_filter()
    _lib.set_filter(kind)
    try:
        yield
    finally:
        _lib.set_filter(prev)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    """bit equality of two dicts of tensors / tuples"""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def _guarded(need, fill):
    """(whole, middle): `need` bytes between two guard regions of SENT; fill(middle) sets the workspace's initial contents."""
    whole = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    mid = whole[GUARD:GUARD + need]
    assert mid.data_ptr() % 256 == 0
    fill(mid)
    return whole, mid


def _guards_intact(whole, need):
    return bool((whole[:GUARD] == SENT).all()) and bool((whole[GUARD + need:] == SENT).all())


def _fill_zero(t):
    t.zero_()


def _fill_ff(t):
    t.fill_(0xFF)


def _fill_random(t):
    g = torch.Generator(device=DEV).manual_seed(20240 + t.numel() % 9973)
    t.copy_(torch.randint(0, 256, (t.numel(),), dtype=torch.uint8, device=DEV, generator=g))


def _ws_class():
    from pit_hip import _lib

    class Ws(_lib.Workspace):
        """A Workspace whose scratch the test owns (``buf``: the wrappers hand it to the library with ITS size) and which keeps
        one codebook cache per codebook shape, zeroed when first used, as a host with several quantisers would."""

        def __init__(self, buf=None, caches=None, use_cache=True):
            super().__init__()
            self.buf = buf
            self.caches = {} if caches is None else caches
            self.use_cache = use_cache

        def cache(self, n, dim, device):
            need = _lib.lib().gqhip_cb_cache_bytes(n, dim)
            if need <= 0 or not self.use_cache:
                self.cache_buf = None
                return None, 0
            t = self.caches.get((n, dim))
            if t is None:
                t = self.caches[(n, dim)] = torch.zeros(need, dtype=torch.uint8, device=device)
            self.cache_buf = t
            return t.data_ptr(), t.numel()

    return Ws


def _lsd(sd):
    with np.errstate(all="ignore"):
        return np.log(sd.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------ the calls
class Case:
    """One call of one entry point: its seeded inputs, how to run it on a given Workspace, its reference."""

    def __init__(self, name, kind, dim, n, rows=None, seed=1, filt="auto", use_cache=True, variant=None, K=1, layout="bchw",
                 grouping=0, ste=True, B=2, hw=(8, 8), bhl=None):
        self.name, self.kind, self.dim, self.n, self.seed, self.filt = name, kind, dim, n, seed, filt
        self.use_cache, self.variant, self.K, self.layout, self.grouping, self.ste = use_cache, variant, K, layout, grouping, ste
        self.B, self.hw, self.bhl = B, hw, bhl
        self.rows = rows if rows is not None else B * hw[0] * hw[1] * K
        self.cb_override = None          # a shared device codebook (the walk edits it in place)

    def __repr__(self):
        return self.name

    # ---- inputs (CPU tensors, made once) ----
    @functools.cached_property
    def inp(self):
        g = torch.Generator().manual_seed(self.seed)
        d, rows, n = self.dim, self.rows, self.n
        if self.kind == "argmax":
            cb = torch.from_numpy(O.codebook(n, d, 42))
            if self.variant == "undecided":          # max|cb| > 255: outside the fp16 filter's range, every row scans
                return dict(mu=torch.randn(rows, d, generator=g) * 60.0,
                            sd=torch.exp(0.5 * (-1.5 + 0.3 * torch.randn(rows, d, generator=g))) * 40.0, cb=cb * 80.0)
            if self.variant == "nonfinite":
                mu, sd = torch.randn(rows, d, generator=g), torch.rand(rows, d, generator=g) + 0.3
                mu[3, 5] = float("nan"); mu[7, 0] = float("inf"); sd[11, 2] = 0.0; sd[12, 3] = float("nan"); mu[20, 1] = -float("inf")
                return dict(mu=mu, sd=sd, cb=cb)
            return dict(mu=0.9 * torch.randn(rows, d, generator=g),
                        sd=torch.exp(0.5 * (-1.5 + 0.3 * torch.randn(rows, d, generator=g))), cb=cb)
        if self.kind == "vq_argmin":
            cb = torch.from_numpy(O.codebook(n, d, 42))
            if self.variant == "undecided":
                return dict(z=torch.randn(rows, d, generator=g) * 60.0, cb=cb * 80.0)
            return dict(z=0.9 * torch.randn(rows, d, generator=g), cb=cb)
        h, w = self.hw
        c = d * self.K
        if self.kind in ("qz", "gauss"):
            z = torch.cat([0.9 * torch.randn(self.B, c, h, w, generator=g), -1.5 + 0.3 * torch.randn(self.B, c, h, w, generator=g)], 1)
            noise = torch.randn(self.B, c, h, w, generator=g)
            if self.layout == "blc":
                z, noise = (t.permute(0, 2, 3, 1).reshape(self.B, h * w, -1).contiguous() for t in (z, noise))
            return dict(z=z, noise=noise, cb=torch.from_numpy(O.codebook(n, d, 42)))
        if self.kind == "vqz":
            z = torch.randn(self.B, c, h, w, generator=g)
            if self.layout == "blc":
                z = z.permute(0, 2, 3, 1).reshape(self.B, h * w, c).contiguous()
            return dict(z=z, cb=torch.randn(n, d, generator=g))
        raise AssertionError(self.kind)

    @functools.cached_property
    def dev(self):
        return {k: v.to(DEV) for k, v in self.inp.items()}

    def cb_dev(self):
        return self.cb_override if self.cb_override is not None else self.dev["cb"]

    def need(self):
        from pit_hip import _lib

        if self.kind == "mha":
            B, H, L = self.bhl
            return max(int(_lib.lib().gq_mha_bwd_workspace_bytes(B, L, H * 64, H)), 8)
        with _filter(self.filt):
            return int(_lib.lib().gqhip_workspace_bytes(self.rows, self.n, self.dim))

    # ---- the call ----
    def run(self, ws):
        """-> dict of device tensors (+ the debug counters of the call), after a synchronise"""
        from pit_hip import _lib

        ws.use_cache = self.use_cache
        with _filter(self.filt):
            out = self._run(ws, _lib)
            _sync()
            if self.kind != "mha":
                out["counters"] = _lib.debug_counters(ws)
                if self.dim == 4 and self.use_cache and self.filt == "auto" and _lib.lib().gqhip_grid_search_applies(self.n, 4):
                    out["grid"] = tuple(sorted(_lib.debug_grid(ws).items()))
        return out

    def _run(self, ws, _lib):
        d, v = self.dim, (self.dev if self.kind != "mha" else None)
        if self.kind == "argmax":
            idx, zhat = _lib.gq_argmax(v["mu"], v["sd"], self.cb_dev(), 1.0, ws=ws)
            return dict(idx=idx, zhat=zhat)
        if self.kind == "vq_argmin":
            idx, zq = _lib.vq_argmin(v["z"], self.cb_dev(), ws=ws, use_cache=self.use_cache)
            return dict(idx=idx, zq=zq)
        if self.kind == "qz":
            idx, zhat, mu_o, sd_o, noquant = _lib.gq_quantize_z(v["z"], self.cb_dev(), d, self.layout, self.grouping, ws=ws,
                                                                return_operands=True, noise=v["noise"])
            return dict(idx=idx, zhat=zhat, mu=mu_o, sd=sd_o, noquant=noquant)
        if self.kind == "gauss":
            lam = torch.tensor(LAM0, dtype=torch.float64, device=DEV)
            idx, zhat, quant, noquant, std, scalars = _lib.gq_quantize_z_gauss(
                v["z"], self.cb_dev(), d, self.layout, self.grouping, v["noise"], lam, int(math.log2(self.n)), 0.5, 1.01, (1e-7, 1e7),
                False, use_ste=self.ste, ws=ws)
            # the words gqhip.h defines in the 64 bytes: float[0..3] and double[0..2] at byte 32 (the rest is not written)
            return dict(idx=idx, zhat=zhat, quant=quant, noquant=noquant, std=std, scalars_f32=scalars[:16].view(torch.float32).clone(),
                        scalars_f64=scalars[32:56].view(torch.float64).clone(), lam=lam)
        if self.kind == "vqz":
            idx, zq, loss = _lib.vq_quantize_z(v["z"], self.cb_dev(), d, self.layout, 0.25, True, ws=ws)
            return dict(idx=idx, zq=zq, loss=loss)
        if self.kind == "mha":
            B, H, L = self.bhl
            qkv, dout, out, lse = self.mha_operands()
            dqkv = torch.full((B, L, 3 * H * 64), float("nan"), dtype=torch.float32, device=DEV)
            rc = _lib.lib().gq_mha_bwd_f32(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), B, L,
                                          H * 64, H, ws.buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            return dict(dqkv=dqkv)
        raise AssertionError(self.kind)

    def mha_operands(self):
        import test_gpu_vit_train as V
        from pit_hip import _lib

        qkv, dout = V._case(*self.bhl)[:2]
        if "mha_fwd" not in self.__dict__:
            self.__dict__["mha_fwd"] = _lib.mha_fwd_lse(qkv, self.bhl[1])
        out, lse = self.__dict__["mha_fwd"]
        return qkv, dout, out, lse

    # ---- the independent reference ----
    def pairs(self):
        return 0 if self.kind == "mha" else self.rows * self.n

    def check(self, out):
        from pit_hip import _lib

        cb = self.cb_dev().cpu().numpy() if self.kind != "mha" else None
        if self.kind == "argmax":
            mu, sd = self.inp["mu"].numpy(), self.inp["sd"].numpy()
            with np.errstate(all="ignore"):
                oi, _ = O.argmax_rows(mu, sd, cb, 1.0, logstd=_lsd(sd))
            assert np.array_equal(out["idx"].cpu().numpy(), oi)
            assert np.array_equal(out["zhat"].cpu().numpy(), cb[oi])
        elif self.kind == "vq_argmin":
            oi = O.vq_argmin_rows(self.inp["z"].numpy(), cb)
            assert np.array_equal(out["idx"].cpu().numpy(), oi)
            assert np.array_equal(out["zq"].cpu().numpy(), cb[oi])
        elif self.kind in ("qz", "gauss"):
            self._check_from_z(out, cb, _lib)
        elif self.kind == "vqz":
            ozq, oind, oloss, gap = O.vq_forward_eval(self.inp["z"].numpy(), cb, self.K, self.layout, 0.25, True)
            assert np.array_equal(out["idx"].cpu().numpy(), oind), float(gap.min())
            assert np.array_equal(out["zq"].cpu().numpy(), ozq)
            assert abs(float(out["loss"][0]) - float(oloss)) <= 2e-6 * max(1.0, abs(float(oloss)))
        elif self.kind == "mha":
            import test_gpu_vit_train as V

            _, _, _, g64, g32 = V._case(*self.bhl)
            V._gate(self.name, out["dqkv"], g64, g32, self.bhl[1])

    def _rows_of(self, idx):
        """module layout [B, K, h, w] / [B, L, K] -> rows (b, l, k)"""
        return (idx.permute(0, 2, 3, 1) if self.layout == "bchw" else idx).reshape(-1)

    def _check_from_z(self, out, cb, _lib):
        d = self.dim
        if self.kind == "qz":
            mu_r, sd_r = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
            idx = out["idx"]
        else:   # the operands the same kernels derive, through the plain module-level entry on a scratch of its own
            idx, _, mu_t, sd_t = _lib.gq_quantize_z(self.dev["z"], self.cb_dev(), d, self.layout, self.grouping, return_operands=True)
            _sync()
            mu_r, sd_r = mu_t.cpu().numpy(), sd_t.cpu().numpy()
            assert torch.equal(out["idx"], idx)
        oi, _ = O.argmax_rows(mu_r, sd_r, cb, 1.0, logstd=_lsd(sd_r))
        assert np.array_equal(self._rows_of(idx).cpu().numpy(), oi)
        codes = _lib.gq_dequant(out["idx"], self.cb_dev(), d, self.layout, self.grouping)
        # zhat_noquant = mu + noise * sd: against the fp64 expression (two fp32 roundings of values of size ~ |mu| + |noise| sd)
        z, noise = self.inp["z"].double(), self.inp["noise"].double()
        ax = 1 if self.layout == "bchw" else 2
        mu, lv = z.chunk(2, dim=ax)
        want = mu + noise * torch.exp(0.5 * lv.clamp(-30.0, 20.0))
        assert float((out["noquant"].cpu().double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max() + 1.0)
        if self.kind == "qz":
            assert torch.equal(out["zhat"], codes)
            return
        assert torch.equal(out["quant"], codes) and torch.equal(out["zhat"], codes)      # finite sample: (g - g) + code == code
        zn = self.inp["z"].numpy()
        if self.layout == "blc":
            zn = zn.reshape(self.B, self.hw[0], self.hw[1], -1).transpose(0, 3, 1, 2)
        want_s, state = O.gq2_quant_gaussian_stats(zn, d, self.n, LAM0)
        f4, d3 = out["scalars_f32"].cpu(), out["scalars_f64"].cpu()
        for i, k in enumerate(("kl_loss", "bits-mean", "bits-min", "bits-max")):
            assert abs(float(f4[i]) - float(want_s[k])) <= 2e-6 * max(1.0, abs(float(want_s[k]))), (k, float(f4[i]), want_s[k])
        assert tuple(float(x) for x in d3) == state and tuple(float(x) for x in out["lam"].cpu()) == state
        sd_want = torch.exp(0.5 * lv.clamp(-30.0, 20.0))
        np.testing.assert_allclose(out["std"].cpu().double().numpy(), sd_want.numpy(), rtol=2.4e-7)


def _cases():
    c = []
    # dense fp16 filter + re-rank with the codebook's image in the cache, dims 8 / 16 / 32; every filter selection at dim 16
    for dim in (8, 16, 32):
        c.append(Case(f"dense{dim}", "argmax", dim, 4096, rows=300, seed=10 + dim))
    for filt in ("fp32", "bf16", "mixed"):
        c.append(Case(f"dense16_{filt}", "argmax", 16, 4096, rows=300, seed=26, filt=filt))
    c.append(Case("record_sets", "argmax", 16, 65536 + 40, rows=600, seed=3))
    c.append(Case("grid4", "argmax", 4, 16384, rows=300, seed=4))
    c.append(Case("grid4_no_cache", "argmax", 4, 16384, rows=300, seed=4, use_cache=False))
    c.append(Case("exhaustive6", "argmax", 6, 512, rows=257, seed=6))
    c.append(Case("all_undecided", "argmax", 16, 8192, rows=300, seed=5, variant="undecided"))
    c.append(Case("non_finite_rows", "argmax", 16, 8192, rows=64, seed=7, variant="nonfinite"))
    c.append(Case("vq_all_undecided", "vq_argmin", 16, 8192, rows=300, seed=5, variant="undecided"))
    c.append(Case("vq16", "vq_argmin", 16, 4096, rows=300, seed=8))
    c.append(Case("qz_bchw_strided", "qz", 8, 4096, seed=31, K=2, layout="bchw", grouping=0))
    c.append(Case("qz_blc_contiguous", "qz", 8, 4096, seed=32, K=2, layout="blc", grouping=1))
    c.append(Case("gauss_ste", "gauss", 16, 4096, seed=33, K=1, layout="bchw", grouping=1, ste=True))
    c.append(Case("gauss_no_ste", "gauss", 16, 4096, seed=33, K=1, layout="bchw", grouping=1, ste=False))
    c.append(Case("vqz_k1", "vqz", 16, 4096, seed=34, K=1, layout="bchw"))
    c.append(Case("vqz_k2", "vqz", 16, 4096, seed=35, K=2, layout="blc"))
    c.append(Case("mha_2_3_33", "mha", 64, 0, rows=0, bhl=(2, 3, 33)))
    c.append(Case("mha_1_2_129", "mha", 64, 0, rows=0, bhl=(1, 2, 129)))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# The calls that leave the leftovers: more rows, another dim, another entry point, another filter selection than the case they dirty.
DIRT = {
    "dense_vq": Case("dirt_dense_vq", "vq_argmin", 32, 4096, rows=700, seed=91, filt="bf16"),
    "grid_gq": Case("dirt_grid_gq", "argmax", 4, 16384, rows=700, seed=92),
    "grid_vq": Case("dirt_grid_vq", "vq_argmin", 4, 16384, rows=700, seed=94),
    "exhaustive_vq": Case("dirt_exhaustive_vq", "vqz", 6, 512, seed=93, K=1, layout="bchw", hw=(20, 20)),
    "record_sets_gq": BY_NAME["record_sets"],
}


def _dirt_for(case):
    """dense -> grid -> exhaustive -> dense, and VQ <-> GQ"""
    if case.kind == "mha":
        return DIRT["record_sets_gq"]      # the largest footprint of the module under the two row sums
    if case.name.startswith("grid4") or case.name == "record_sets":
        return DIRT["dense_vq"]            # dense (VQ, dim 32, split-bf16) -> grid (GQ, dim 4) / -> the fp16 filter at dim 16
    if case.name == "exhaustive6":
        return DIRT["grid_vq"]             # grid (VQ, dim 4) -> exhaustive (GQ, dim 6)
    if case.kind in ("vq_argmin", "vqz"):
        return DIRT["grid_gq"]             # GQ -> VQ
    return DIRT["exhaustive_vq"]           # exhaustive (VQ from z, dim 6) -> dense (GQ)


@functools.lru_cache(maxsize=None)
def _big():
    """One buffer sized for the largest call of the module; it is never cleared: leftovers pile up in it."""
    need = max(c.need() for c in list(CASES) + list(DIRT.values()))
    return torch.zeros(need + 8448, dtype=torch.uint8, device=DEV)


_BASE = {}


def _baseline(case):
    """The call on exactly `need` zero-filled bytes between two guard regions: outputs, counters, the caches it leaves, and
    whether the guards survived.  Run once per case and shared."""
    if case.name not in _BASE:
        Ws = _ws_class()
        need = case.need()
        whole, mid = _guarded(need, _fill_zero)
        caches = {}
        out = case.run(Ws(mid, caches))
        _BASE[case.name] = (out, caches, _guards_intact(whole, need), need)
    return _BASE[case.name]


def _refilled_run(case, fill):
    Ws = _ws_class()
    out0, caches, _, need = _baseline(case)
    whole, mid = _guarded(need, fill)
    out = case.run(Ws(mid, caches))
    assert _guards_intact(whole, need)
    return out0, out


# ------------------------------------------------------------------------------------------ 1. don't-care scratch
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_zero_filled_workspace_of_the_declared_size_matches_the_reference(case):
    out, _, guards, need = _baseline(case)
    assert need > 0 and guards, "the call wrote outside its declared workspace"
    case.check(out)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_leftovers_of_a_different_call_do_not_change_the_result(case):
    Ws = _ws_class()
    out0, caches, _, _ = _baseline(case)
    big, dirt = _big(), _dirt_for(case)
    assert dirt.need() > 0 and (case.kind == "mha" or (dirt.rows > case.rows or dirt.n > case.n) and dirt.kind != case.kind)
    dirt.run(Ws(big, {}))                       # its own codebook, its own cache
    _same(case.run(Ws(big, caches)), out0)      # the same scratch, untouched in between, with the larger byte count


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_workspace_of_ff_bytes_does_not_change_the_result(case):
    out0, out = _refilled_run(case, _fill_ff)
    _same(out, out0)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_workspace_of_random_bytes_does_not_change_the_result(case):
    out0, out = _refilled_run(case, _fill_random)
    _same(out, out0)


# ------------------------------------------------------------------------------------------ 3. the declared size is the footprint
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_layout_follows_from_the_shape_not_from_the_size_of_the_buffer(case):
    """(The guards of the exact-size runs are asserted by the tests above.)  A larger buffer, with the larger count passed in,
    gives the same bits; the attention backward takes no byte count: its larger buffer only moves nothing."""
    Ws = _ws_class()
    out0, caches, guards, need = _baseline(case)
    assert guards
    extra = 8448
    whole, mid = _guarded(need + extra, _fill_zero)
    _same(case.run(Ws(mid, caches)), out0)
    assert _guards_intact(whole, need + extra)
    assert int(mid[need:].count_nonzero()) == 0, "bytes beyond the declared size were written"


# ------------------------------------------------------------------------------------------ 2. history
def _walk():
    """(steps, codebooks): ~20 calls on shared device codebooks; an entry is a Case, or a tuple naming something else to do."""
    cbs = {(4096, 16): torch.from_numpy(O.codebook(4096, 16, 42)).to(DEV), (16384, 4): torch.from_numpy(O.codebook(16384, 4, 42)).to(DEV),
           (4096, 8): torch.from_numpy(O.codebook(4096, 8, 42)).to(DEV), (512, 6): torch.from_numpy(O.codebook(512, 6, 42)).to(DEV),
           (65536 + 40, 16): torch.from_numpy(O.codebook(65536 + 40, 16, 42)).to(DEV)}
    rng = np.random.default_rng(77)
    r = lambda lo, hi: int(rng.integers(lo, hi))
    steps = [
        Case("w_dense16", "argmax", 16, 4096, rows=r(200, 400), seed=101),
        Case("w_grid4", "argmax", 4, 16384, rows=r(150, 300), seed=102),
        Case("w_vq16_one_row", "vq_argmin", 16, 4096, rows=1, seed=103),
        Case("w_exhaustive6", "argmax", 6, 512, rows=257, seed=104),
        Case("w_qz", "qz", 8, 4096, seed=105, K=2, layout="bchw", grouping=0),
        Case("w_short_last_batch", "argmax", 16, 4096, rows=r(40, 90), seed=106),
        Case("w_gauss_ste", "gauss", 16, 4096, seed=107, layout="bchw", grouping=1, ste=True),
        Case("w_vqz_k2", "vqz", 8, 4096, seed=108, K=2, layout="blc"),
        ("invalid_arg",),
        Case("w_dense8_grows", "argmax", 8, 4096, rows=r(500, 560), seed=109),
        Case("w_dense16_bf16", "argmax", 16, 4096, rows=r(200, 400), seed=110, filt="bf16"),
        Case("w_dim4_bf16_one_row", "argmax", 4, 16384, rows=1, seed=111, filt="bf16"),
        ("edit", (4096, 16)),
        Case("w_dense16_edited", "argmax", 16, 4096, rows=r(200, 400), seed=112),
        ("edit", (16384, 4)),
        Case("w_grid4_edited", "argmax", 4, 16384, rows=r(150, 300), seed=113),
        ("workspace_too_small",),
        Case("w_vq4_grid", "vq_argmin", 4, 16384, rows=r(300, 400), seed=114),
        Case("w_record_sets", "argmax", 16, 65536 + 40, rows=r(100, 130), seed=115),
        Case("w_gauss_no_ste_one_image", "gauss", 16, 4096, seed=116, B=1, layout="bchw", grouping=1, ste=False),
        Case("w_vq16_fp32", "vq_argmin", 16, 4096, rows=r(100, 200), seed=117, filt="fp32"),
        Case("w_one_row", "argmax", 16, 4096, rows=1, seed=118),
    ]
    for s in steps:
        if isinstance(s, Case):
            s.cb_override = cbs[(s.n, s.dim)]
    return steps, cbs


def _rejected(L, status, call):
    """A rejected call: its status, and outputs pre-filled with a sentinel that stay as they were."""
    idx = torch.full((64,), -7, dtype=torch.int64, device=DEV)
    zhat = torch.full((64, 64), 777.0, dtype=torch.float32, device=DEV)
    assert call(idx, zhat) == status
    _sync()
    assert bool((idx == -7).all()) and bool((zhat == 777.0).all())


def test_one_workspace_through_a_walk_of_calls_equals_fresh_workspaces():
    """One scratch buffer and one cache per codebook shape through rows that grow and shrink (1, a short last batch), every launch
    path, two filter switches, codebooks edited in place halfway, a call the library rejects and one whose buffer is a byte short:
    every accepted call is bit-equal to the same call on a fresh Workspace and agrees with the oracle; a rejected call writes
    nothing."""
    from pit_hip import _lib

    L, Ws = _lib.lib(), _ws_class()
    steps, cbs = _walk()
    assert sum(s.pairs() for s in steps if isinstance(s, Case)) <= 40_000_000       # the oracle budget of test_gpu_stress.py
    ws = Ws()
    st = torch.cuda.current_stream().cuda_stream
    mu, sd = torch.randn(64, 16, device=DEV), torch.rand(64, 16, device=DEV) + 0.5
    done = 0
    for s in steps:
        if isinstance(s, Case):
            got = s.run(ws)
            fresh = s.run(Ws())
            _same(got, fresh)
            s.check(got)
            done += 1
        elif s[0] == "edit":
            g = torch.Generator(device=DEV).manual_seed(5)
            cb = cbs[s[1]]
            cb.mul_(1.5).add_(0.05 * torch.randn(cb.shape, device=DEV, generator=g))       # in place: same pointer, no version the library sees
        elif s[0] == "invalid_arg":
            cb = cbs[(4096, 16)]
            _rejected(L, 1, lambda idx, zhat: L.gq_argmax_f32(mu.data_ptr(), sd.data_ptr(), None, cb.data_ptr(), idx.data_ptr(),
                                                               zhat.data_ptr(), 65, 64, 4096, 1.0, ws.buf.data_ptr(), ws.buf.numel(),
                                                               None, 0, st))
        else:
            cb = cbs[(4096, 16)]
            need = L.gqhip_workspace_bytes(64, 4096, 16)
            assert ws.buf.numel() >= need
            _rejected(L, 2, lambda idx, zhat: L.gq_argmax_f32(mu.data_ptr(), sd.data_ptr(), None, cb.data_ptr(), idx.data_ptr(),
                                                               zhat.data_ptr(), 16, 64, 4096, 1.0, ws.buf.data_ptr(), need - 1,
                                                               None, 0, st))
    assert done == 18                           # + the two rejected calls


# ------------------------------------------------------------------------------------------ 4. zero-in / zero-out scratch
def _images(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g) * 2 - 1
    y = (x + 0.05 * torch.randn(B, C, H, W, generator=g)).clamp(-1, 1)
    return x, y


class _Metric:
    """The three metric entry points over ctypes on a buffer the test owns.  call(ws, nbytes, x, y, idx) -> the record words."""

    def __init__(self, name, C, H, W, tokens=35):
        from pit_hip import _lib

        self.name, self.C, self.H, self.W, self.tokens, self.L = name, C, H, W, tokens, _lib.lib()

    def bytes(self, B):
        f = {"step_record": lambda: self.L.gq_step_record_workspace_bytes(B, self.C * self.H * self.W),
             "ssim": lambda: self.L.gq_ssim_workspace_bytes(B, self.C, self.H, self.W),
             "step_record_ssim": lambda: self.L.gq_step_record_ssim_workspace_bytes(B, self.C, self.H, self.W)}[self.name]
        return int(f())

    def call(self, ws, nbytes, x, y, idx):
        B, st, L = x.shape[0], torch.cuda.current_stream().cuda_stream, self.L
        C, H, W = self.C, self.H, self.W
        words = (idx.numel() + 1) // 2
        if self.name == "step_record":
            rec = torch.full((B + words,), -1234567, dtype=torch.int32, device=DEV)
            rc = L.gq_step_record_f32(x.data_ptr(), y.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, C * H * W, idx.numel(),
                                      ws.data_ptr(), nbytes, st)
        elif self.name == "ssim":
            rec = torch.full((2 * B,), float("nan"), dtype=torch.float32, device=DEV)     # [ssim | ms_ssim]
            rc = L.gq_ssim_f32(x.data_ptr(), y.data_ptr(), B, C, H, W, 0, 1, rec.data_ptr(), rec[B:].data_ptr(), ws.data_ptr(), nbytes, st)
        else:
            rec = torch.full((3 * B + words,), -1234567, dtype=torch.int32, device=DEV)
            rc = L.gq_step_record_ssim_f32(x.data_ptr(), y.data_ptr(), idx.data_ptr(), rec.data_ptr(), B, C, H, W, 0, idx.numel(),
                                           ws.data_ptr(), nbytes, st)
        assert rc == 0, rc
        _sync()
        return rec


@functools.lru_cache(maxsize=None)
def _metric_refs(C, H, W, Bmax, seed):
    """Images, indices and the references of a stream, computed once for the largest batch; a call with B images takes the first
    B.  PSNR: the torch expressions of test_step_record_one_launch_matches_the_torch_expressions; SSIM: tests/ssim_ref.py (fp64)."""
    from pit_hip.eval_dist import psnr_zero_mean

    x, y = _images(Bmax, C, H, W, seed)
    y[Bmax - 1] = x[Bmax - 1]                      # the last image of the largest batch: identical, PSNR +inf, partial sums exactly 0
    ssim, ms = S.ssim_msssim(x.numpy(), y.numpy(), True)
    xd, yd = x.to(DEV), y.to(DEV)
    psnr = psnr_zero_mean(xd, yd)
    idx = torch.randint(0, 65536, (Bmax, 35), generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return xd, yd, idx, psnr, ssim, ms


def _check_record(m, rec, B, idx, psnr, ssim, ms):
    from pit_hip.eval_dist import StepRecord

    if m.name == "ssim":
        got = rec.cpu().numpy().astype(np.float64)
        assert np.abs(got[:B] - ssim[:B]).max() <= 1e-6
        if m.H >= 256 and m.W >= 256:
            assert np.abs(got[B:] - ms[:B]).max() <= 1e-6
        else:
            assert np.isnan(got[B:]).all()
        return
    nm = 1 if m.name == "step_record" else 3
    lay = StepRecord(B, m.tokens, n_metrics=nm)
    gi, gm = lay.unpack(rec)
    assert torch.equal(gi.reshape(-1), idx.reshape(-1))
    assert torch.equal(rec[nm * B:], lay.pack(idx, torch.zeros(B, nm, device=DEV))[nm * B:])      # the packed words, the odd count's zero pad
    got, want = gm[:, 0].cpu().numpy(), psnr[:B].cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (got, want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=2e-6)
    if nm == 3:
        g = gm.cpu().numpy().astype(np.float64)
        assert np.abs(g[:, 1] - ssim[:B]).max() <= 1e-6
        if m.H >= 256 and m.W >= 256:
            assert np.abs(g[:, 2] - ms[:B]).max() <= 1e-6
        else:
            assert np.isnan(g[:, 2]).all()


def _stream_of_batches(m, batches, seed):
    """One allocation, zeroed once, sized for the largest batch and set between guards, through a stream of calls of varying B.
    After EVERY call: the record against the references, bit-equal to the same call on a freshly zeroed buffer of its own, the
    guards intact, and the workspace in the state gqhip.h promises: every byte zero again."""
    Bmax = max(batches)
    xd, yd, idx, psnr, ssim, ms = _metric_refs(m.C, m.H, m.W, Bmax, seed)
    need = m.bytes(Bmax)
    assert need > 0 and all(0 < m.bytes(B) <= need for B in batches)
    whole, ws = _guarded(need, _fill_zero)
    left = []
    for i, B in enumerate(batches):
        x, y, ix = xd[:B], yd[:B], idx[:B]
        got = m.call(ws, need, x, y, ix)
        print(f"{m.name} {m.C}x{m.H}x{m.W} call {i} B {B}: metric words {got[:min(3, got.numel())].tolist()}")
        own = torch.zeros(max(m.bytes(B), 8), dtype=torch.uint8, device=DEV)
        fresh = m.call(own, m.bytes(B), x, y, ix)
        assert torch.equal(_bits(got), _bits(fresh)), f"call {i} (B = {B}) on the reused workspace differs from a fresh one"
        _check_record(m, got, B, ix, psnr, ssim, ms)
        assert _guards_intact(whole, need)
        left.append((i, B, int(ws.count_nonzero()), int(own.count_nonzero())))
    # (after the records, so that a workspace that is not reset shows first as what it costs: a wrong metric word)
    assert all(a == 0 and b == 0 for _, _, a, b in left), f"(call, B, non-zero bytes left in the shared / in the fresh workspace): {left}"


@pytest.mark.parametrize("C,H,W", [(3, 64, 48), (3, 96, 96)])
def test_step_record_one_allocation_serves_a_stream_of_batches(C, H, W):
    """16 -> 6 -> 1 -> 16: the short last batch of an epoch and the next epoch's first, in the buffer allocated for 16.  Before the
    finishing thread cleared the partial sums, the second call's tickets started from the bits of the first call's doubles.  B = 1
    has an odd index count; the last image of the 16 is identical to its reconstruction."""
    _stream_of_batches(_Metric("step_record", C, H, W), [16, 6, 1, 16], seed=C * H + W)


@pytest.mark.parametrize("C,H,W,batches", [(3, 64, 48, [16, 6, 1, 16]), (3, 64, 48, [65, 3, 65]), (3, 64, 48, [3, 65]), (3, 96, 96, [16, 6, 1, 16]),
                                           (1, 256, 256, [2, 1, 2])])
def test_ssim_one_allocation_serves_a_stream_of_batches(C, H, W, batches):
    """... and across a multiple of 64 images, where the ticket region of gq_ssim_f32 changes its size; 256 x 256 runs the five
    levels of MS-SSIM, whose pooled planes are cleared by the call's last launch."""
    _stream_of_batches(_Metric("ssim", C, H, W), batches, seed=C * H + W + len(batches))


@pytest.mark.parametrize("C,H,W,batches", [(3, 64, 48, [16, 6, 1, 16]), (3, 96, 96, [16, 6, 1, 16]), (1, 256, 256, [2, 1, 2])])
def test_three_metric_record_one_allocation_serves_a_stream_of_batches(C, H, W, batches):
    _stream_of_batches(_Metric("step_record_ssim", C, H, W), batches, seed=C * H + W + 7)


@pytest.mark.parametrize("name", ["step_record", "ssim", "step_record_ssim"])
def test_metric_calls_lay_their_workspace_out_from_the_shape(name):
    """A zeroed buffer larger than needed, with the larger count passed in: the same bits, nothing written beyond the declared
    size; and the PSNR / index words of the three-metric record are those of the one-metric record."""
    m = _Metric(name, 3, 96, 96)
    xd, yd, idx, psnr, ssim, ms = _metric_refs(3, 96, 96, 16, 3 * 96 + 96)
    B = 6
    need = m.bytes(B)
    exact = m.call(torch.zeros(need, dtype=torch.uint8, device=DEV), need, xd[:B], yd[:B], idx[:B])
    whole, ws = _guarded(need + 8448, _fill_zero)
    ws[need:].fill_(SENT)
    larger = m.call(ws, need + 8448, xd[:B], yd[:B], idx[:B])
    assert torch.equal(_bits(exact), _bits(larger))
    assert _guards_intact(whole, need + 8448) and bool((ws[need:] == SENT).all()) and int(ws[:need].count_nonzero()) == 0
    if name == "step_record_ssim":
        one = _Metric("step_record", 3, 96, 96)
        rec1 = one.call(torch.zeros(one.bytes(B), dtype=torch.uint8, device=DEV), one.bytes(B), xd[:B], yd[:B], idx[:B])
        assert torch.equal(exact[0:3 * B:3], rec1[:B]) and torch.equal(exact[3 * B:], rec1[B:])
