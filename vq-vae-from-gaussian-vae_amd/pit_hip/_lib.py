"""ctypes binding of libgqhip.so (the C ABI declared in include/gqhip.h, which is read at import: the signatures come from its
prototypes).  A new entry point is a prototype there, a definition in csrc/ and a wrapper here that goes through ``_call``.

torch is used only for device memory and the current HIP stream: every call
hands raw ``data_ptr()`` values and ``torch.cuda.current_stream().cuda_stream``
to the library.  There is NO CPU fallback here: if the library is missing or a
tensor is not on a HIP device the call raises.
"""
from __future__ import annotations

import ctypes
import threading
import math
import os
import re
import subprocess
from typing import NamedTuple, Optional, Tuple

import torch

_CSRC = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc"))
LIB_PATH = os.environ.get("GQHIP_LIB", os.path.join(_CSRC, "libgqhip.so"))  # GQHIP_LIB: diagnostic builds

ABI_VERSION = 8
GNSTAT_WORDS = 8     # int64 words per (image, group) statistics record (gqhip.h: gqhip_gnstat_t)
GQHIP_LAYOUT = {"bchw": 0, "blc": 1}
GQHIP_GROUP_STRIDED = 0
GQHIP_GROUP_CONTIGUOUS = 1

_lib: Optional[ctypes.CDLL] = None

_i64 = ctypes.c_int64


class GqHipError(RuntimeError):
    pass


# ---- the C ABI, read from include/gqhip.h ------------------------------------------------------------------------------------
# The header is the one statement of the ABI: scalars map by type, a pointer whose name ends in _host is one the library
# dereferences on the host (typed), every other pointer is a device address or the stream (opaque).
_SCALAR_CTYPES = {"int": ctypes.c_int, "int64_t": _i64, "float": ctypes.c_float, "double": ctypes.c_double}
_HOST_ELEMENT_CTYPES = dict(_SCALAR_CTYPES, int32_t=ctypes.c_int32)
_RETURN_CTYPES = {"int": ctypes.c_int, "int64_t": _i64, "const char *": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"^[ \t]*(int64_t\b|int\b|const\s+char\s*\*)\s*(\w+)\s*\(([^()]*)\)\s*;", re.M)
_PARAMETER = re.compile(r"(?:const\s+)?(\w+)(?:\s+|\s*(\*)\s*)(\w+)")      # [const] type [*] name


def _parse_header(text: str):
    """({name: (restype, [argtypes])}, {name: (parameter names)}) of every prototype ``int | int64_t | const char * name(args);``
    in the text of a C header.  A parameter the mapping above does not cover raises: a guessed width is a garbage argument."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    signatures, params = {}, {}
    for ret, name, arglist in _PROTOTYPE.findall(text):
        argtypes, names = [], []
        for p in ([] if arglist.strip() == "void" else arglist.split(",")):
            m = _PARAMETER.fullmatch(p.strip())
            ctype, star, pname = m.groups() if m else (None, None, "")
            if not star:
                arg = _SCALAR_CTYPES.get(ctype)
            elif not pname.endswith("_host"):
                arg = ctypes.c_void_p
            else:
                arg = ctypes.POINTER(_HOST_ELEMENT_CTYPES[ctype]) if ctype in _HOST_ELEMENT_CTYPES else None
            if arg is None:
                raise GqHipError(f"gqhip.h: no ctypes mapping for the parameter {p.strip()!r} of {name}({' '.join(arglist.split())})")
            argtypes.append(arg)
            names.append(pname)
        signatures[name] = (_RETURN_CTYPES[" ".join(ret.replace("*", " *").split())], argtypes)
        params[name] = tuple(names)
    return signatures, params


def _read_header():
    path = os.path.normpath(os.path.join(_CSRC, "..", "..", "include", "gqhip.h"))    # the Makefile's -I../../include
    if not os.path.exists(path):
        raise GqHipError(f"{path} is missing: the binding reads the C ABI from it. There is no second copy.")
    with open(path) as f:
        return _parse_header(f.read())


_SIGNATURES, _PARAMS = _read_header()      # name -> (restype, [argtypes]); name -> parameter names
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _pointer(a):
    return a if a is None or isinstance(a, int) else a.data_ptr()


def _same(a):
    return a


def _converters(name: str):
    """(one converter per argument the caller passes, whether a trailing ``stream`` follows them) of an entry."""
    argtypes, names = _SIGNATURES[name][1], _PARAMS[name]
    has_stream = bool(names) and names[-1] == "stream"
    kinds = {ctypes.c_void_p: _pointer, ctypes.c_int: int, _i64: int, ctypes.c_float: float, ctypes.c_double: float}
    return tuple(kinds.get(t, _same) for t in (argtypes[:-1] if has_stream else argtypes)), has_stream


_CONVERTERS = {name: _converters(name) for name in _SIGNATURES}


def _call_args(name: str, args) -> list:
    """The caller's arguments of entry ``name`` as ctypes takes them, by the entry's declared types: a tensor for a ``void *``
    becomes its data_ptr() (None and an int address pass), ``int`` / ``int64_t`` take int() (a bool is 0 / 1), ``float`` /
    ``double`` take float(), typed host pointers pass.  The stream is not among them: _call supplies it."""
    converters = _CONVERTERS[name][0]
    if len(args) != len(converters):
        raise GqHipError(f"{name}: takes {len(converters)} arguments" + (" and the stream" if _CONVERTERS[name][1] else "")
                         + f", got {len(args)}")
    return [c(a) for c, a in zip(converters, args)]


def _call(name: str, device, *args) -> None:
    """THE way into a launching entry point: on ``device``, with _call_args' conversions and the current stream, raising a
    GqHipError that names the entry when the status is not 0."""
    with torch.cuda.device(device):
        converted = _call_args(name, args)
        if _CONVERTERS[name][1]:
            converted.append(_stream())
        rc = getattr(lib(), name)(*converted)
        if rc != 0:
            _check(rc, name)


def build(force: bool = False) -> str:
    """Compile libgqhip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-s", "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args + ["libgqhip.so"])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load the library, failing loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GqHipError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C vq-vae-from-gaussian-vae_amd/csrc`). There is no CPU fallback."
            )
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.gqhip_abi_version() != ABI_VERSION:
            raise GqHipError("libgqhip.so ABI version mismatch")
        _lib = L
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        L = lib()
        raise GqHipError(f"{what}: {L.gqhip_status_string(rc).decode()} (hipError {L.gqhip_last_hip_error()})")


def _dev(t: torch.Tensor, dtype: torch.dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GqHipError(f"{name} must be a tensor on a HIP device (got {getattr(t, 'device', type(t))}); "
                         "the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise GqHipError(f"{name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _stream() -> int:
    """The current stream of the current device as a hipStream_t: torch.cuda.current_stream().cuda_stream without the Stream
    object in between (about 2 us of an 11 us call: profiles/r30/host_call_overhead.txt; torch's compiled code asks the same way)."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class _Scratch:
    """A grow-only device buffer that is never replaced during or after a HIP graph capture that used it: a captured graph has
    the pointer baked in, so growing the buffer then -- or after the capture, by an eager call with a bigger shape -- would leave
    the graph writing into freed memory.  It grows when a request exceeds it (or names another device), refuses to while the
    current stream is capturing or once pinned, and pins itself when it is used under capture; size it with a warm-up call first.
    ``zeroed``: new memory comes from torch.zeros.  ``pin``: the pin of another scratch, to share it (buffers that one capture
    uses together); a one-element list, so that sharing it ties no reference cycle around the buffers."""

    _what = "scratch"

    def __init__(self, what: Optional[str] = None, zeroed: bool = False, pin: Optional[list] = None) -> None:
        self.buf: Optional[torch.Tensor] = None
        self._pin = [False] if pin is None else pin      # [True] once a graph capture has used the buffer: never replaced again
        self._what = what or self._what
        self._new = torch.zeros if zeroed else torch.empty

    def _take(self, need: int, device, shape: str = "", stale: bool = False) -> Tuple[int, int]:
        """(pointer, bytes) of at least ``need`` bytes on ``device``; ``need`` < 0 is the library's "unsupported shape"."""
        if need < 0:
            raise GqHipError(f"unsupported shape {shape}")
        capturing = torch.cuda.is_current_stream_capturing()
        if self.buf is None or stale or self.buf.numel() < need or self.buf.device != device:
            if capturing or self._pin[0]:
                raise GqHipError(f"{self._what} would have to grow during / after a HIP graph capture that uses it: "
                                 "run a warm-up call of the largest shape before capturing, or use a separate one")
            self.buf = self._new(need, dtype=torch.uint8, device=device)
        if capturing:
            self._pin[0] = True
        return self.buf.data_ptr(), self.buf.numel()


class Workspace(_Scratch):
    """Caller-owned scratch, grown on demand and reused across calls, plus the persistent CODEBOOK CACHE of the shapes that keep
    one (gqhip.h: gqhip_cb_cache_bytes -- dims 4 / 8: the spatial index of the pruned search; the library validates it against a
    content hash of the codebook on every call and rebuilds it in-stream when it is stale, so nothing here has to track the
    codebook).  The sizes come from the library under its current selections (``set_filter``, ``set_odd_dims``, ``set_wide_dims``): nothing to redo here
    after changing one.  One workspace serves one stream at a time (its header carries the per-call counters).  Graph captures: the rule
    of ``_Scratch``, one pin for both buffers; size them with a warm-up call first (``reserve``)."""

    _what = "workspace"

    def __init__(self) -> None:
        super().__init__()
        self._cache = _Scratch("the codebook cache", zeroed=True, pin=self._pin)    # zeros: no stamp -> built by the first call
        self._cache_key = None
        self._cache_calls = 0     # calls that were handed the current cache buffer
        self.no_search = False    # the dim-4 index of this codebook was found degenerate (gqhip_cb_cache_degenerate): dense path from then on

    @property
    def cache_buf(self) -> Optional[torch.Tensor]:
        return self._cache.buf

    @cache_buf.setter
    def cache_buf(self, t: Optional[torch.Tensor]) -> None:
        self._cache.buf = t

    def cache(self, n: int, dim: int, device) -> Tuple[Optional[int], int]:
        """(pointer, bytes) of the codebook cache for (n, dim), or (None, 0) for shapes that keep none."""
        need = lib().gqhip_cb_cache_bytes(n, dim)
        if need <= 0 or self.no_search:
            return None, 0
        key = (n, dim, device)
        old = self._cache.buf
        out = self._cache._take(need, device, stale=self._cache_key != key)
        if self._cache.buf is not old:
            self._cache_key = key
            self._cache_calls = 0
        # ONE look at what the index builder found, at the call after the one that built it (a 4-KiB synchronous copy, once per
        # cache buffer): a clustered / collapsed codebook puts most codes into one sub-leaf, and the search then hands every row to
        # the block-per-row finish kernel -- milliseconds per call where filter + re-rank takes ~100 us.  Such a book goes
        # back to the dense path for good (always exact; a codebook that changes every step should not pass a cache at all: vq.py).
        self._cache_calls += 1
        searches = lib().gqhip_grid_search_applies(n, dim) or lib().gqhip_low_dim_search_applies(n, dim)   # (dims 1-3: the exhaustive route then)
        if self._cache_calls == 2 and searches and not torch.cuda.is_current_stream_capturing():
            if lib().gqhip_cb_cache_degenerate(out[0], n, dim) == 1:
                self.no_search = True
                return None, 0
        return out

    def reserve(self, rows: int, n: int, dim: int, device) -> None:
        """Size the scratch and the codebook cache for a shape ahead of a graph capture."""
        self.get(rows, n, dim, device)
        self.cache(n, dim, device)

    def get(self, rows: int, n: int, dim: int, device) -> Tuple[int, int]:
        return self._take(lib().gqhip_workspace_bytes(rows, n, dim), device, f"rows={rows} n={n} dim={dim}")


def gq_scores(mu, sd, cb, out, beta: float = 1.0) -> None:
    """Compat op (reference gq_cuda.ops.gq_cuda): fills out[rows, n] in place."""
    mu, sd, cb = (_dev(t, torch.float32, n) for t, n in ((mu, "mu"), (sd, "std"), (cb, "codebook")))
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
        raise GqHipError("out must be a contiguous float32 HIP tensor")
    rows, dim = mu.shape
    n = cb.shape[0]
    if sd.shape != mu.shape or cb.shape[1] != dim or tuple(out.shape) != (rows, n):
        raise GqHipError("shape mismatch in gq_scores")
    _call("gq_scores_f32", mu.device, mu, sd, cb, out, dim, rows, n, beta)


def gq_argmax(mu, sd, cb, beta: float = 1.0, logsd=None, ws: Optional[Workspace] = None, want_zhat: bool = True):
    """Fused score+argmax+gather on (mu, sd[, log sd]) rows -> (idx int64 [rows], zhat [rows, dim])."""
    mu, sd, cb = (_dev(t, torch.float32, n) for t, n in ((mu, "mu"), (sd, "std"), (cb, "codebook")))
    logsd = None if logsd is None else _dev(logsd, torch.float32, "logsd")
    rows, dim = mu.shape
    n = cb.shape[0]
    if sd.shape != mu.shape or cb.shape[1] != dim:
        raise GqHipError("shape mismatch in gq_argmax")
    ws = ws or Workspace()
    idx = torch.empty(rows, dtype=torch.int64, device=mu.device)
    zhat = torch.empty(rows, dim, dtype=torch.float32, device=mu.device) if want_zhat else None
    with torch.cuda.device(mu.device):
        wptr, wbytes = ws.get(rows, n, dim, mu.device)
        cptr, cbytes = ws.cache(n, dim, mu.device)
    _call("gq_argmax_f32", mu.device, mu, sd, logsd, cb, idx, zhat, dim, rows, n, beta, wptr, wbytes, cptr, cbytes)
    return idx, zhat


def gq_quantize_z(z, cb, dim: int, layout: str, grouping: int, lv_range=(-30.0, 20.0), beta: float = 1.0,
                  ws: Optional[Workspace] = None, return_operands: bool = False, noise=None):
    """Module-level fused quantiser on the encoder output z (see gqhip.h).  ``noise`` (same shape as the returned
    zhat): the first launch also writes ``zhat_noquant = mu + noise * sd`` (gaussian.py:121), returned as a third value."""
    z, cb = _dev(z, torch.float32, "z"), _dev(cb, torch.float32, "codebook")
    n = cb.shape[0]
    B, L, c, K, rows, shape, idx_shape = _z_geometry(z, dim, layout)
    ws = ws or Workspace()
    dev = z.device
    idx = torch.empty(idx_shape, dtype=torch.int64, device=dev)
    zhat = torch.empty(shape, dtype=torch.float32, device=dev)
    noquant = None
    if noise is not None:
        noise = _dev(noise, torch.float32, "noise")
        if tuple(noise.shape) != tuple(zhat.shape):
            raise GqHipError(f"noise must have the shape of zhat {tuple(zhat.shape)}, got {tuple(noise.shape)}")
        noquant = torch.empty_like(zhat)
    mu_o = sd_o = None
    if return_operands:
        mu_o = torch.empty(rows, dim, dtype=torch.float32, device=dev)
        sd_o = torch.empty(rows, dim, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(max(rows, 1), n, dim, dev)
        cptr, cbytes = ws.cache(n, dim, dev)
    _call("gq_quantize_z_f32", dev, z, noise, cb, idx, zhat, noquant, mu_o, sd_o, B, L, c, dim, n, GQHIP_LAYOUT[layout], grouping,
          lv_range[0], lv_range[1], beta, wptr, wbytes, cptr, cbytes)
    out = (idx, zhat)
    if return_operands:
        out = out + (mu_o, sd_o)
    if noise is not None:
        out = out + (noquant,)
    return out


def gq_quantize_z_gauss(z, cb, dim: int, layout: str, grouping: int, noise, lam_state, log2n: int, tolerance: float,
                        lam_factor: float, lam_range, lam_max_decreases: bool, use_ste: bool = True, lv_range=(-30.0, 20.0),
                        beta: float = 1.0, ws: Optional[Workspace] = None, want_std: bool = True):
    """GaussianQuantRegularizer2's eval forward in one call (gqhip.h: gq_quantize_z_gauss_f32).  ``lam_state``: float64 [3] device
    tensor {lam, lam_min, lam_max}, advanced in place.  Returns (idx, zhat, zhat_quant, zhat_noquant, std or None, scalars):
    ``zhat_quant`` holds the codewords themselves (info["zhat_quant"]; zhat itself when ``use_ste`` is off), ``scalars`` is a
    fresh 64-byte device buffer: float32 view [0:4] = kl_loss, bits-mean, bits-min, bits-max; float64 view of bytes 32..56 = the
    lambdas after the update."""
    z, cb, noise = _dev(z, torch.float32, "z"), _dev(cb, torch.float32, "codebook"), _dev(noise, torch.float32, "noise")
    _lam_ok(lam_state, "lam_state")
    n = cb.shape[0]
    B, L, c, K, rows, shape, idx_shape = _z_geometry(z, dim, layout)
    ws = ws or Workspace()
    dev = z.device
    idx = torch.empty(idx_shape, dtype=torch.int64, device=dev)
    zhat = torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(noise.shape) != tuple(zhat.shape):
        raise GqHipError(f"noise must have the shape of zhat {tuple(zhat.shape)}, got {tuple(noise.shape)}")
    noquant = torch.empty_like(zhat)
    pure = torch.empty_like(zhat) if use_ste else None
    std = torch.empty_like(zhat) if want_std else None
    scalars = torch.empty(64, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(max(rows, 1), n, dim, dev)
        cptr, cbytes = ws.cache(n, dim, dev)
    _call("gq_quantize_z_gauss_f32", dev, z, noise, cb, idx, zhat, pure, noquant, std, scalars, lam_state, B, L, c, dim, n,
          GQHIP_LAYOUT[layout], grouping, lv_range[0], lv_range[1], beta, bool(use_ste), log2n, tolerance, lam_factor,
          lam_range[0], lam_range[1], bool(lam_max_decreases), wptr, wbytes, cptr, cbytes)
    return idx, zhat, (pure if use_ste else zhat), noquant, std, scalars


def _channel_geometry(t, layout: str, channels: Optional[int] = None, holds: str = ""):
    """(B, L, C, shape) of a tensor in a module layout (gqhip.h): [B, C, ...] ("bchw", L = the positions of one image) or
    [B, L, C] ("blc"); ``shape(k)`` is the shape of an output with k channels in that layout.  ``channels``: what C must be,
    ``holds`` naming it in the error."""
    if layout not in GQHIP_LAYOUT or t.dim() < 3 or (layout == "blc" and t.dim() != 3):
        raise GqHipError(f"expected [B, C, ...] (bchw) or [B, L, C] (blc), got {tuple(t.shape)} as {layout!r}")
    if layout == "bchw":
        B, C, L = t.shape[0], t.shape[1], int(t[0, 0].numel())
    else:
        B, L, C = t.shape
    if channels is not None and C != channels:
        raise GqHipError(f"{C} channels do not hold {holds}")

    def shape(k):
        return ((B, k) + tuple(t.shape[2:])) if layout == "bchw" else (B, L, k)

    return B, L, C, shape


def _z_geometry(t, dim: int, layout: str, holds: str = "mu|logvar"):
    """(B, L, c, K, rows, shape of zhat, shape of the indices) of a tensor in a module layout whose channel axis holds
    [mu | logvar] (an encoder output: 2 c channels), "z" (c channels) or "idx" (the indices themselves: K = c / dim channels)."""
    B, L, ch, shape = _channel_geometry(t, layout)
    c = {"mu|logvar": ch // 2, "z": ch, "idx": ch * dim}[holds]
    K = c // dim
    return B, L, c, K, B * L * K, shape(c), shape(K)


def _grad_of(t, shape, name: str, of: str):
    """A gradient that must have ``shape`` (that of ``of``): None passes through, fp32 on the device, contiguous."""
    if t is None:
        return None
    t = _dev(t, torch.float32, name)
    if tuple(t.shape) != tuple(shape):
        raise GqHipError(f"{name} must have the shape of {of} {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _grad_scalar(t, name: str):
    """A gradient that holds one float: None passes through, fp32 on the device."""
    if t is None:
        return None
    t = _dev(t, torch.float32, name)
    if t.numel() != 1:
        raise GqHipError(f"{name} must hold one float")
    return t


def _lam_ok(t, name: str) -> None:
    if not (t.is_cuda and t.dtype == torch.float64 and t.numel() == 3 and t.is_contiguous()):
        raise GqHipError(f"{name} must be a contiguous float64 [3] tensor on the HIP device")


def gq_gauss_train(z, dim: int, layout: str, grouping: int, noise, lam_state, log2n: int, tolerance: float, lam_factor: float,
                   lam_range, lam_max_decreases: bool, loss_divisor: float, lv_range=(-30.0, 20.0), want_std: bool = False):
    """GaussianQuantRegularizer's train-mode forward in one call (gqhip.h: gq_gauss_train_f32): no codebook, no workspace.
    ``lam_state``: float64 [3] device tensor {lam, lam_min, lam_max}, advanced in place.  Returns (zhat, std or None, kl2row,
    scalars) with ``scalars`` as gq_quantize_z_gauss returns it."""
    z, noise = _dev(z, torch.float32, "z"), _dev(noise, torch.float32, "noise")
    _lam_ok(lam_state, "lam_state")
    B, L, c, K, rows, shape, _ = _z_geometry(z, dim, layout)
    if tuple(noise.shape) != shape:
        raise GqHipError(f"noise must have the shape of zhat {shape}, got {tuple(noise.shape)}")
    dev = z.device
    zhat = torch.empty(shape, dtype=torch.float32, device=dev)
    std = torch.empty_like(zhat) if want_std else None
    kl2row = torch.empty(rows, dtype=torch.float32, device=dev)
    scalars = torch.empty(64, dtype=torch.uint8, device=dev)
    _call("gq_gauss_train_f32", dev, z, noise, zhat, std, kl2row, scalars, lam_state, B, L, c, dim, GQHIP_LAYOUT[layout], grouping,
          lv_range[0], lv_range[1], log2n, tolerance, lam_factor, lam_range[0], lam_range[1], bool(lam_max_decreases), loss_divisor)
    return zhat, std, kl2row, scalars


def gq_gauss_backward(z, dim: int, layout: str, grouping: int, noise, lam_before, log2n: int, tolerance: float,
                      loss_divisor: float, g_zhat=None, g_zhat_noquant=None, g_std=None, g_kl=None, lv_range=(-30.0, 20.0)):
    """grad_z of either train-mode forward in one call (gqhip.h: gq_gauss_backward_f32).  ``lam_before``: the float64 [3] state as
    it was before the forward.  Gradients may be None (zero); those of zhat and zhat_noquant are summed when both arrive, and a
    gradient that is not contiguous in the layout of zhat is made so.  ``g_kl``: one float32 on the device."""
    z, noise = _dev(z, torch.float32, "z"), _dev(noise, torch.float32, "noise")
    _lam_ok(lam_before, "lam_before")
    B, L, c, K, rows, shape, _ = _z_geometry(z, dim, layout)
    g_zhat, g_zhat_noquant, g_std = (_grad_of(t, shape, name, "zhat") for t, name in
                                     ((g_zhat, "g_zhat"), (g_zhat_noquant, "g_zhat_noquant"), (g_std, "g_std")))
    if g_zhat is not None and g_zhat_noquant is not None:
        g_zhat = g_zhat + g_zhat_noquant
    elif g_zhat is None:
        g_zhat = g_zhat_noquant
    g_kl = _grad_scalar(g_kl, "g_kl")
    grad_z = torch.empty_like(z)
    _call("gq_gauss_backward_f32", z.device, z, noise, g_zhat, g_std, g_kl, lam_before, grad_z, B, L, c, dim, GQHIP_LAYOUT[layout],
          grouping, lv_range[0], lv_range[1], log2n, tolerance, loss_divisor)
    return grad_z


def vq_quantize_z(z, emb, dim: int, layout: str, beta: float, legacy: bool, ws: Optional[Workspace] = None, use_cache: bool = True):
    """VQQuantizer's forward in one call (gqhip.h: vq_quantize_z_f32): z [B, c, ...] ("bchw") or [B, L, c] ("blc") ->
    (idx [B, K, ...] / [B, L, K], z_q in the layout of z, loss float32 [2] = {codebook_loss, mean((e - z)^2)}).
    ``use_cache=False``: no codebook cache in this call, as in vq_argmin (a codebook that changes every step)."""
    z, emb = _dev(z, torch.float32, "z"), _dev(emb, torch.float32, "embedding")
    n = emb.shape[0]
    B, L, c, K, rows, _, idx_shape = _z_geometry(z, dim, layout, holds="z")
    if c % dim or emb.shape[1] != dim:
        raise GqHipError("shape mismatch in vq_quantize_z")
    ws = ws or Workspace()
    dev = z.device
    idx = torch.empty(idx_shape, dtype=torch.int64, device=dev)
    zq = torch.empty_like(z)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(max(rows, 1), n, dim, dev)
        cptr, cbytes = ws.cache(n, dim, dev) if use_cache and not low_dim_search_applies(n, dim) else (None, 0)   # (dims 1-3: that cache serves the Gaussian score only)
    _call("vq_quantize_z_f32", dev, z, emb, idx, zq, loss, B, L, c, dim, n, GQHIP_LAYOUT[layout], beta, bool(legacy), wptr, wbytes,
          cptr, cbytes)
    return idx, zq, loss


class _TrainWorkspace(_Scratch):
    """Scratch of one family's train step, grown on demand and reused across calls; its contents never matter on entry.  One per
    stream at a time.  Graph captures: the rule of ``_Scratch``.  A family names its size function (gqhip.h) and that function's
    arguments; ``get(*arguments, device)`` -> (pointer, bytes)."""

    _size, _shape = "", ()

    def get(self, *shape_and_device) -> Tuple[int, int]:
        *shape, device = shape_and_device
        return self._take(getattr(lib(), self._size)(*shape), device, " ".join(f"{k}={v}" for k, v in zip(self._shape, shape)))


class VqBackwardWorkspace(_TrainWorkspace):     # of vq_backward
    _what, _size, _shape = "vq_backward's workspace", "vq_backward_workspace_bytes", ("items", "n", "dim")


class LfqTrainWorkspace(_TrainWorkspace):       # of lfq_train / lfq_backward
    _what, _size, _shape = "the LFQ train step's workspace", "lfq_train_workspace_bytes", ("rows", "d")


class BsqTrainWorkspace(_TrainWorkspace):       # of bsq_train / bsq_backward
    _what, _size, _shape = "the BSQ train step's workspace", "bsq_train_workspace_bytes", ("rows", "d")


def vq_backward(z, emb, idx, dim: int, layout: str, beta: float, legacy: bool, g_zq=None, g_loss=None, want_grad_z: bool = True,
                want_grad_emb: bool = True, ws: Optional[VqBackwardWorkspace] = None):
    """The backward of VQQuantizer's train step in one call (gqhip.h: vq_backward_f32).  z, emb, idx: the forward's operands and
    indices; ``g_zq`` (shape of z; made contiguous in z's layout when it is not) and ``g_loss`` (one float32 on the device) are
    the gradients arriving at z_q and codebook_loss, None = zero.  Returns (grad_z or None, grad_emb [n, dim] or None)."""
    z, emb, idx = _dev(z, torch.float32, "z"), _dev(emb, torch.float32, "embedding"), _dev(idx, torch.int64, "indices")
    n = emb.shape[0]
    B, L, c, K, items, _, idx_shape = _z_geometry(z, dim, layout, holds="z")
    if c % dim or emb.shape[1] != dim or tuple(idx.shape) != idx_shape:
        raise GqHipError("shape mismatch in vq_backward")
    g_zq, g_loss = _grad_of(g_zq, z.shape, "g_zq", "z"), _grad_scalar(g_loss, "g_loss")
    ws = ws or VqBackwardWorkspace()
    dev = z.device
    grad_z = torch.empty_like(z) if want_grad_z else None
    grad_emb = torch.empty_like(emb) if want_grad_emb else None
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(items, n, dim, dev)
    _call("vq_backward_f32", dev, z, emb, idx, g_zq, g_loss, grad_z, grad_emb, B, L, c, dim, n, GQHIP_LAYOUT[layout], beta,
          bool(legacy), wptr, wbytes)
    return grad_z, grad_emb


def gq_dequant(idx, cb, dim: int, layout: str, grouping: int):
    idx, cb = _dev(idx, torch.int64, "indices"), _dev(cb, torch.float32, "codebook")
    B, L, _, K, _, shape, _ = _z_geometry(idx, dim, layout, holds="idx")
    zhat = torch.empty(shape, dtype=torch.float32, device=idx.device)
    _call("gq_dequant_f32", idx.device, idx, cb, zhat, B, L, K, dim, cb.shape[0], GQHIP_LAYOUT[layout], grouping)
    return zhat


def vq_argmin(z, emb, ws: Optional[Workspace] = None, use_cache: bool = True):
    """``use_cache=False``: no codebook cache in this call -- the dense filter + re-rank path whatever the shape.  For codebooks
    that change every step (training): a dim-4 index would be rebuilt by one block on every call."""
    z, emb = _dev(z, torch.float32, "z"), _dev(emb, torch.float32, "embedding")
    rows, dim = z.shape
    n = emb.shape[0]
    ws = ws or Workspace()
    idx = torch.empty(rows, dtype=torch.int64, device=z.device)
    zq = torch.empty(rows, dim, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        wptr, wbytes = ws.get(max(rows, 1), n, dim, z.device)
        cptr, cbytes = ws.cache(n, dim, z.device) if use_cache and not low_dim_search_applies(n, dim) else (None, 0)
    _call("vq_argmin_f32", z.device, z, emb, idx, zq, dim, rows, n, wptr, wbytes, cptr, cbytes)
    return idx, zq


def lfq_pack(x):
    x = _dev(x, torch.float32, "x")
    rows, nbits = x.shape
    idx = torch.empty(rows, dtype=torch.int64, device=x.device)
    q = torch.empty_like(x)
    _call("lfq_pack_f32", x.device, x, idx, q, rows, nbits)
    return idx, q


def _lfq_avg_numel(dim: int) -> int:
    """floats in lfq_train's ``avg`` (a width the library refuses still gets a buffer: the refusal is the library's)"""
    return 1 << dim if 1 <= dim <= 16 else 1


def lfq_train(x, num_codebooks: int, dim: int, layout: str, w_s: float = 1.0, w_b: float = 1.0,
              ws: Optional[LfqTrainWorkspace] = None):
    """LFQQuantizer's train-mode forward in one call (gqhip.h: lfq_train_f32): x [B, C, ...] ("bchw") or [B, L, C] ("blc") ->
    (quantized in the layout of x, indices int64 [B, 1, ...] / [B, L, 1], avg float32 [2^dim] (for lfq_backward), scalars
    float32 [4] on the device = {entropy_aux_loss, per_sample_entropy, codebook_entropy, commit_loss})."""
    x = _dev(x, torch.float32, "x")
    B, L, C, shape = _channel_geometry(x, layout, num_codebooks * dim, f"{num_codebooks} codebooks of {dim} bits")
    ws = ws or LfqTrainWorkspace()
    dev = x.device
    quantized = torch.empty_like(x)
    idx = torch.empty(shape(1), dtype=torch.int64, device=dev)
    avg = torch.empty(_lfq_avg_numel(dim), dtype=torch.float32, device=dev)
    scalars = torch.empty(4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(B * L * num_codebooks, dim, dev)
    _call("lfq_train_f32", dev, x, quantized, idx, avg, scalars, B, L, C, num_codebooks, dim, GQHIP_LAYOUT[layout], w_s, w_b,
          wptr, wbytes)
    return quantized, idx, avg, scalars


def lfq_backward(x, avg, num_codebooks: int, dim: int, layout: str, w_s: float = 1.0, w_b: float = 1.0, g_q=None, g_aux=None,
                 g_commit=None, ws: Optional[LfqTrainWorkspace] = None):
    """The backward of LFQQuantizer's train step in one call (gqhip.h: lfq_backward_f32).  x, avg: the forward's operand and its
    ``avg``; ``g_q`` (shape of x; made contiguous in x's layout when it is not), ``g_aux`` and ``g_commit`` (one float32 on the
    device each) are the gradients arriving at quantized, entropy_aux_loss and commit_loss, None = zero.  Returns grad_x."""
    x, avg = _dev(x, torch.float32, "x"), _dev(avg, torch.float32, "avg")
    B, L, C, _ = _channel_geometry(x, layout, num_codebooks * dim, f"{num_codebooks} codebooks of {dim} bits")
    if avg.numel() != _lfq_avg_numel(dim):
        raise GqHipError(f"avg must hold 2^{dim} floats, got {avg.numel()}")
    g_q, g_aux, g_commit = _grad_of(g_q, x.shape, "g_q", "x"), _grad_scalar(g_aux, "g_aux"), _grad_scalar(g_commit, "g_commit")
    ws = ws or LfqTrainWorkspace()
    dev = x.device
    grad_x = torch.empty_like(x)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(B * L * num_codebooks, dim, dev)
    _call("lfq_backward_f32", dev, x, avg, g_q, g_aux, g_commit, grad_x, B, L, C, num_codebooks, dim, GQHIP_LAYOUT[layout], w_s, w_b,
          wptr, wbytes)
    return grad_x


def _bsq_avg_shape(dim: int):
    """shape of bsq_train's ``avg``: per bit of the 1..16 a BSQ codebook holds, the mean probabilities of its two values"""
    if not 1 <= dim <= 16:
        raise GqHipError(f"a BSQ codebook holds 1..16 bits, got {dim}")
    return dim, 2


def _aligned16(t):
    """The "blc" kernels move rows 16 bytes at a time: a view at an odd storage offset is copied."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def bsq_train(x, dim: int, layout: str, w_s: float = 1.0, w_b: float = 1.0, ws: Optional[BsqTrainWorkspace] = None):
    """BSQQuantizer's train-mode forward in one call (gqhip.h: bsq_train_f32): x [B, 16 dim, ...] ("bchw") or [B, L, 16 dim]
    ("blc") -> (quantized in the layout of x, indices int64 [B, dim, ...] / [B, L, dim], avg float32 [dim, 2] (for bsq_backward),
    scalars float32 [3] on the device = {entropy_aux_loss, per_sample_entropy, codebook_entropy})."""
    x = _aligned16(_dev(x, torch.float32, "x"))
    avg_shape = _bsq_avg_shape(dim)
    B, L, C, shape = _channel_geometry(x, layout, 16 * dim, f"16 codebooks of {dim} bits")
    ws = ws or BsqTrainWorkspace()
    dev = x.device
    quantized = torch.empty_like(x)
    idx = torch.empty(shape(dim), dtype=torch.int64, device=dev)
    avg = torch.empty(avg_shape, dtype=torch.float32, device=dev)
    scalars = torch.empty(3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(B * L, dim, dev)
    _call("bsq_train_f32", dev, x, quantized, idx, avg, scalars, B, L, C, dim, GQHIP_LAYOUT[layout], w_s, w_b, wptr, wbytes)
    return quantized, idx, avg, scalars


def bsq_backward(x, avg, dim: int, layout: str, w_s: float = 1.0, w_b: float = 1.0, g_q=None, g_aux=None,
                 ws: Optional[BsqTrainWorkspace] = None):
    """The backward of BSQQuantizer's train step in one call (gqhip.h: bsq_backward_f32).  x, avg: the forward's operand and its
    ``avg``; ``g_q`` (shape of x; made contiguous in x's layout when it is not) and ``g_aux`` (one float32 on the device) are the
    gradients arriving at quantized and entropy_aux_loss, None = zero.  Returns grad_x."""
    x, avg = _aligned16(_dev(x, torch.float32, "x")), _dev(avg, torch.float32, "avg")
    avg_shape = _bsq_avg_shape(dim)
    B, L, C, _ = _channel_geometry(x, layout, 16 * dim, f"16 codebooks of {dim} bits")
    if avg.numel() != math.prod(avg_shape):
        raise GqHipError(f"avg must hold [{dim}, 2] floats, got {avg.numel()}")
    g_q, g_aux = _aligned16(_grad_of(g_q, x.shape, "g_q", "x")), _grad_scalar(g_aux, "g_aux")
    ws = ws or BsqTrainWorkspace()
    dev = x.device
    grad_x = torch.empty_like(x)
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(B * L, dim, dev)
    _call("bsq_backward_f32", dev, x, avg, g_q, g_aux, grad_x, B, L, C, dim, GQHIP_LAYOUT[layout], w_s, w_b, wptr, wbytes)
    return grad_x


class LpipsHeadWorkspace(_TrainWorkspace):      # of lpips_head
    _what, _size, _shape = "the LPIPS head's workspace", "lpips_head_workspace_bytes", ("B", "C", "HW")


def _lpips_operands(f0, f1, w, keep, layout: str):
    """The checked operands of the LPIPS head and (B, C, HW): f0, f1 (and keep, uint8) [B, C, ...] ("bchw") or [B, L, C] ("blc")."""
    f0, f1, w = _dev(f0, torch.float32, "f0"), _dev(f1, torch.float32, "f1"), _dev(w, torch.float32, "w")
    if layout not in GQHIP_LAYOUT or f0.dim() < 3 or f0.shape != f1.shape:
        raise GqHipError(f"f0 and f1 must share a shape [B, C, ...] (bchw) or [B, L, C] (blc), got {tuple(f0.shape)}, {tuple(f1.shape)}")
    if layout == "bchw":
        B, C, HW = f0.shape[0], f0.shape[1], math.prod(f0.shape[2:])
    else:
        B, HW, C = f0.shape[0], math.prod(f0.shape[1:-1]), f0.shape[-1]
    if w.numel() != C:
        raise GqHipError(f"w holds {w.numel()} weights for {C} channels")
    if keep is not None:
        keep = _dev(keep, torch.uint8, "keep")
        if keep.shape != f0.shape:
            raise GqHipError(f"keep must have the shape of the features {tuple(f0.shape)}, got {tuple(keep.shape)}")
    return f0, f1, w, keep, B, C, HW


def lpips_head(f0, f1, w, layout: str, keep=None, keep_scale: float = 1.0, ws: Optional[LpipsHeadWorkspace] = None):
    """One LPIPS level's comparison head in one call (gqhip.h: lpips_head_f32): features f0, f1 in a library layout, the `lin`
    weights w [C], an optional uint8 keep mask in the features' layout with its scale -> out float32 [B]."""
    f0, f1, w, keep, B, C, HW = _lpips_operands(f0, f1, w, keep, layout)
    ws = ws or LpipsHeadWorkspace()
    dev = f0.device
    out = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0:                                          # an empty tensor has no pointer to hand over
        return out
    with torch.cuda.device(dev):
        wptr, wbytes = ws.get(B, C, HW, dev)
    _call("lpips_head_f32", dev, f0, f1, w, keep, keep_scale, out, B, C, HW, GQHIP_LAYOUT[layout], wptr, wbytes)
    return out


def lpips_head_backward(f0, f1, w, g_out, layout: str, keep=None, keep_scale: float = 1.0):
    """The gradient of ``lpips_head`` for its SECOND feature map in one call (gqhip.h: lpips_head_backward_f32); ``g_out`` [B] is the
    gradient arriving at out.  The head is symmetric: swap f0 and f1 for the gradient of the first."""
    f0, f1, w, keep, B, C, HW = _lpips_operands(f0, f1, w, keep, layout)
    g_out = _grad_of(g_out, (B,), "g_out", "out")
    grad = torch.empty_like(f1)
    if B == 0:
        return grad
    _call("lpips_head_backward_f32", f0.device, f0, f1, w, keep, keep_scale, g_out, grad, B, C, HW, GQHIP_LAYOUT[layout])
    return grad


def lfq_unpack(idx, nbits: int):
    idx = _dev(idx, torch.int64, "indices")
    rows = idx.numel()
    q = torch.empty(rows, nbits, dtype=torch.float32, device=idx.device)
    _call("lfq_unpack_f32", idx.device, idx, q, rows, nbits)
    return q


def _levels(levels):
    arr = (ctypes.c_int32 * len(levels))(*[int(v) for v in levels])
    return arr, len(levels)


def fsq_quantize(z, levels):
    """z [rows, nlev] -> (zhat [rows, nlev] fp32, packed indices [rows] int32)."""
    z = _dev(z, torch.float32, "z")
    rows, nlev = z.shape
    arr, n = _levels(levels)
    assert n == nlev
    zhat = torch.empty_like(z)
    idx = torch.empty(rows, dtype=torch.int32, device=z.device)
    _call("fsq_quantize_f32", z.device, z, arr, n, zhat, idx, rows)
    return zhat, idx


def fsq_train(z, levels, layout: str):
    """FSQQuantizer's forward with round_ste's value in one call (gqhip.h: fsq_train_f32): z [B, nlev, ...] ("bchw") or
    [B, L, nlev] ("blc") -> (zhat in the layout of z, packed indices int32 [B, 1, ...] / [B, L, 1])."""
    z = _dev(z, torch.float32, "z")
    B, L, _, shape = _channel_geometry(z, layout, len(levels), f"{len(levels)} levels")
    arr, n = _levels(levels)
    zhat = torch.empty_like(z)
    idx = torch.empty(shape(1), dtype=torch.int32, device=z.device)
    _call("fsq_train_f32", z.device, z, arr, n, zhat, idx, B, L, GQHIP_LAYOUT[layout])
    return zhat, idx


def fsq_backward(z, g_zhat, levels, layout: str):
    """The backward of fsq_train in one call (gqhip.h: fsq_backward_f32): ``g_zhat`` has the shape of z (made contiguous in z's
    layout when it is not).  Returns grad_z."""
    z = _dev(z, torch.float32, "z")
    B, L, _, _ = _channel_geometry(z, layout, len(levels), f"{len(levels)} levels")
    g_zhat = _grad_of(g_zhat, z.shape, "g_zhat", "z")
    if g_zhat is None:
        raise GqHipError("g_zhat is required")
    arr, n = _levels(levels)
    grad_z = torch.empty_like(z)
    _call("fsq_backward_f32", z.device, z, g_zhat, arr, n, grad_z, B, L, GQHIP_LAYOUT[layout])
    return grad_z


def fsq_dequant(idx, levels):
    idx = _dev(idx, torch.int32, "indices")
    arr, n = _levels(levels)
    rows = idx.numel()
    zhat = torch.empty(rows, n, dtype=torch.float32, device=idx.device)
    _call("fsq_dequant_f32", idx.device, idx, arr, n, zhat, rows)
    return zhat


def image_layout(x: torch.Tensor):
    """0 = NCHW contiguous, 1 = NHWC (torch channels_last) dense, None = neither (caller falls back)."""
    if x.dim() != 4:
        return None
    if x.is_contiguous():
        return 0
    if x.is_contiguous(memory_format=torch.channels_last):
        return 1
    return None


class StatsArena:
    """All GroupNorm statistics records of ONE forward of a module, carved out of one int64 buffer that a single fill zeroes at
    the forward's start (gqhip.h:gqhip_stats_prezeroed) -- instead of one 32-KB memset launch in front of every kernel that leaves
    statistics behind (~60 per encode + decode step).  Grows to the forward's demand; records that do not fit come from
    torch.empty and are zeroed by the entry point as before."""

    def __init__(self) -> None:
        self.buf, self.used, self.want = None, 0, 0

    def begin(self, device) -> None:
        if self.buf is None or self.buf.device != device or self.buf.numel() < self.want:
            self.buf = torch.zeros(max(self.want, 1), dtype=torch.int64, device=device)
        elif self.used:
            self.buf[: self.used].zero_()
        self.used = self.want = 0

    def take(self, nwords: int):
        self.want += nwords
        if self.buf is None or self.used + nwords > self.buf.numel():
            return None
        t = self.buf[self.used: self.used + nwords]
        self.used += nwords
        return t


class _ArenaState(threading.local):      # per thread, like the library's flag (gqhip_stats_prezeroed is thread-local)
    def __init__(self) -> None:
        self.state = {"active": None, "flag": 0}


_ARENA_TLS = _ArenaState()


class stats_arena:
    """``with stats_arena(arena, device): ...`` -- the statistics records allocated inside come from ``arena``."""

    def __init__(self, arena: StatsArena, device) -> None:
        self.arena, self.device = arena, device

    def __enter__(self):
        self.prev = _ARENA_TLS.state["active"]
        self.arena.begin(self.device)
        _ARENA_TLS.state["active"] = self.arena
        return self.arena

    def __exit__(self, *exc):
        _ARENA_TLS.state["active"] = self.prev
        _set_prezeroed(0)


def _set_prezeroed(on: int) -> None:
    if _ARENA_TLS.state["flag"] != on:
        lib().gqhip_stats_prezeroed(on)
        _ARENA_TLS.state["flag"] = on


def _stats_records(nwords: int, device):
    """An int64 tensor for ``nwords`` words of statistics records; tells the library whether it is already zero."""
    a = _ARENA_TLS.state["active"]
    t = a.take(nwords) if a is not None else None
    if t is not None and t.device == device:
        _set_prezeroed(1)
        return t
    _set_prezeroed(0)
    return torch.empty(nwords, dtype=torch.int64, device=device)


def gn_nhwc_ok(C: int, groups: int) -> bool:
    cpg = C // groups
    return C % groups == 0 and cpg % 4 == 0 and C % 4 == 0 and 256 % (C // 4) == 0 and groups <= 64


def _need_nhwc(who: str, x, c: int = 1, h: int = 1, w: int = 1, hw: int = 1) -> None:
    """The input test of the conv-stack wrappers: ``x`` is a dense channels_last fp32 HIP tensor whose C, H, W and H * W are
    multiples of ``c``, ``h``, ``w`` and ``hw``; the error names ``who`` and what it needs."""
    if (image_layout(x) != 1 or not x.is_cuda or x.dtype != torch.float32 or x.shape[1] % c or x.shape[2] % h or x.shape[3] % w
            or (x.shape[2] * x.shape[3]) % hw):
        needs = [f"{name} % {m} == 0" for name, m in (("C", c), ("H", h), ("W", w), ("H * W", hw)) if m > 1]
        raise GqHipError(f"{who} needs a dense channels_last fp32 HIP tensor" + (" with " + ", ".join(needs) if needs else ""))


def _need_residual(who: str, residual, shape) -> None:
    if residual is not None and (image_layout(residual) != 1 or tuple(residual.shape) != tuple(shape)):
        raise GqHipError(f"{who}: residual must be channels_last [B, Cout, H, W]")


def _out_nhwc(x, C: int, H: int, W: int):
    """An uninitialised channels_last [B, C, H, W] result for the input x."""
    return torch.empty((x.shape[0], C, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)


def _out_and_stats(x, C: int, H: int, W: int, stats_groups: int):
    """(_out_nhwc, the statistics records of its ``stats_groups`` GroupNorm groups or None).  Call it right before the library
    call that fills the records: _stats_records tells the library whether they are zero already, and the flag is the thread's."""
    y = _out_nhwc(x, C, H, W)
    return y, (_stats_records(GNSTAT_WORDS * x.shape[0] * stats_groups, x.device) if stats_groups else None)


def _y_or_both(y, ostats):
    return y if ostats is None else (y, ostats)


def _pow2_scale(bound, amp: float = 1.0) -> float:
    """The operand scale of the fp16 x 3 routes: the largest power of two, 2^14 at the most, that keeps amp * bound inside 32768
    (half of fp16's range: headroom for the rounding of the split)."""
    return min(2.0 ** math.floor(math.log2(32768.0 / (amp * max(float(bound), 1e-30)))), 2.0 ** 14)


def _operand_scales(scale, u_scale: float, post_scale: float = 1.0):
    """(device scales or None, v_scale, mscale) of a direct fp16 x 3 convolution: ``scale`` is a float bound of the
    activation, or the device float[2] of f16_scales -- the kernel then reads both factors there, and 0.0 goes in their place."""
    if torch.is_tensor(scale):
        return scale, 0.0, 0.0
    v_scale = _pow2_scale(scale)
    return None, v_scale, float(post_scale) / (v_scale * u_scale)


def _split_f16(w):
    """(hi, lo, u_scale): the two-term fp16 split hi + lo of w * u_scale, u_scale the power of two that brings max|w| into
    (8192, 16384] (1.0 for an all-zero w)."""
    w = w.detach().float()
    amax = float(w.abs().max())
    u_scale = 2.0 ** math.floor(math.log2(16384.0 / max(amax, 1e-30))) if amax > 0 else 1.0
    ws = w * u_scale
    hi = ws.half()
    return hi, (ws - hi.float()).half(), u_scale


class GnFold(NamedTuple):
    """The ``gn`` argument of the conv-stack wrappers: the GroupNorm (+ SiLU) a kernel applies to x + pre_bias while it stages
    it.  ``stats``: the statistics records of x + pre_bias (gn_stats, or what the producer of x left).  A plain 7-tuple in
    this order is taken as one."""
    gamma: Optional[torch.Tensor]
    beta: Optional[torch.Tensor]
    groups: int
    eps: float
    silu: bool
    stats: Optional[torch.Tensor]
    pre_bias: Optional[torch.Tensor]


_NO_GN = GnFold(None, None, 1, 0.0, False, None, None)    # what the kernels with an optional GroupNorm get without one


class F16Gemm(NamedTuple):
    """The ``f16`` argument of wino_conv3x3: U3 [T, 3 Cin, Cout] fp16 = [U_h; U_l; U_h] of U * u_scale, ``bound`` >= max|tensor
    the input transform sees|, ``wf2``: (U_h, U_l) in wino_gemm_f16x2's operand order (wino_weights_operand_order) or None.
    A plain 3- or 4-tuple in this order is taken as one."""
    U3: torch.Tensor
    u_scale: float
    bound: float
    wf2: Optional[torch.Tensor] = None


def gn_silu(x, gamma, beta, groups: int, eps: float, silu: bool = True, pre_bias=None):
    """Fused GroupNorm(+SiLU) on an NCHW or channels_last fp32 HIP tensor (see gqhip.h:gn_silu_f32)."""
    layout = image_layout(x)
    if not x.is_cuda or x.dtype != torch.float32 or layout is None:
        raise GqHipError("gn_silu needs a dense fp32 NCHW / channels_last HIP tensor")
    B, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    # statistics scratch: from the forward's arena (one per module, thread and stream, never under a graph capture:
    # modules/unet.py:_with_stats_arena) or a fresh stream-ordered tensor from the caching allocator
    ws = _stats_records(GNSTAT_WORDS * B * groups, x.device)
    y = torch.empty_like(x)  # preserves the memory format
    _call("gn_silu_f32", x.device, x, gamma, beta, pre_bias, y, B, C, HW, groups, eps, bool(silu), layout, ws)
    return y


def add_bias(a, b, bias=None):
    """y = a + b (+ bias[c]) on NCHW / channels_last fp32 HIP tensors of the same layout."""
    layout = image_layout(a)
    if layout is None or image_layout(b) != layout or not a.is_cuda or a.dtype != torch.float32:
        raise GqHipError("add_bias needs two dense fp32 HIP tensors of the same layout")
    B, C = a.shape[0], a.shape[1]
    HW = a.shape[2] * a.shape[3]
    y = torch.empty_like(a)
    _call("add_bias_f32", a.device, a, b, bias, y, B, C, HW, layout)
    return y


def add_bias_stats(a, b, bias, groups: int):
    """channels_last only: (a + b (+ bias[c]), GroupNorm statistics of that sum [2 * B * groups] fp64)."""
    _need_nhwc("add_bias_stats", a)
    if image_layout(b) != 1 or not gn_nhwc_ok(a.shape[1], groups):
        raise GqHipError("add_bias_stats needs two dense channels_last fp32 HIP tensors with a GroupNorm-compatible C")
    B, C = a.shape[0], a.shape[1]
    HW = a.shape[2] * a.shape[3]
    y = torch.empty_like(a)
    stats = _stats_records(GNSTAT_WORDS * B * groups, a.device)
    _call("add_bias_stats_f32", a.device, a, b, bias, y, B, C, HW, groups, stats)
    return y, stats


def gn_apply(x, gamma, beta, groups: int, eps: float, silu: bool, stats):
    """channels_last only: GroupNorm(+SiLU) of x from statistics computed by add_bias_stats."""
    _need_nhwc("gn_apply", x)
    B, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    y = torch.empty_like(x)
    _call("gn_apply_f32", x.device, x, gamma, beta, y, B, C, HW, groups, eps, bool(silu), stats)
    return y


def gn_stats_values(stats):
    """[2 * n_bg] fp64 (sum, sum of squares per (image, group)) from the fixed-point statistics records the kernels
    accumulate (gqhip.h: gqhip_gnstat_t; the readers' evaluation order).  For tests and diagnostics."""
    r = stats.view(-1, GNSTAT_WORDS).double()
    s = (r[:, 2] * 2.0 ** 24 + r[:, 1] * 2.0 ** -16) + r[:, 0] * 2.0 ** -56
    ss = (r[:, 5] * 2.0 ** 24 + r[:, 4] * 2.0 ** -16) + r[:, 3] * 2.0 ** -56
    bad = r[:, 6] != 0
    s = torch.where(bad, torch.full_like(s, float("nan")), s)
    ss = torch.where(bad, torch.full_like(ss, float("nan")), ss)
    return torch.stack([s, ss], 1).flatten()


def gn_stats(x, groups: int, pre_bias=None):
    """channels_last only: GroupNorm statistics of x (+ pre_bias[c]) as [2 * B * groups] fp64 (sum, sum of squares)."""
    _need_nhwc("gn_stats", x)
    if not gn_nhwc_ok(x.shape[1], groups):
        raise GqHipError("gn_stats needs a GroupNorm-compatible C")
    B, C = x.shape[0], x.shape[1]
    stats = _stats_records(GNSTAT_WORDS * B * groups, x.device)
    _call("gn_stats_f32", x.device, x, pre_bias, B, C, x.shape[2] * x.shape[3], groups, stats)
    return stats


def wino_conv3x3(x, U, gn=None, residual=None, bias=None, stats_groups: int = 0, f16=None):
    """3x3 stride-1 padding-1 convolution of a channels_last fp32 HIP tensor by Winograd F(2x2, 3x3) in three stages (input
    transform, GEMMs, output transform):
    U [16, Cin, Cout] = G g G^T (see unet._wino_weights).  Returns [B, Cout, H, W] channels_last, no bias.
    ``gn`` (a GnFold): the convolution's input is SiLU(GroupNorm(x + pre_bias)),
    applied inside the input transform (the normalised tensor is never materialised).
    ``stats_groups`` > 0: the output transform also adds bias[c] (+ ``residual``) and returns
    (y, GroupNorm statistics of y) -- the tail of a ResnetBlock, or conv1 + the statistics norm2 needs, in one pass.
    ``f16`` (an F16Gemm: U3, u_scale, bound[, wf2]): run the 16 / 36 GEMMs as ONE fp16 batched GEMM with fp32 accumulation over a K axis
    that carries the three products of two-term fp16 splits (see gqhip.h:wino_in_nhwc_f16x3): U3 [T, 3 Cin, Cout] fp16 =
    [U_h; U_l; U_h] of U * u_scale, bound >= max|x| (guarantees the scaled transform stays inside fp16's range)."""
    _need_nhwc("wino_conv3x3", x, c=4, h=2, w=2)
    B, C, H, W = x.shape
    T, cout = U.shape[0], U.shape[2]
    f4 = T == 36                                              # F(4x4,3x3): 6x6 tiles, 36 GEMMs
    if f4 and (H % 4 or W % 4):
        raise GqHipError("F(4x4,3x3) needs H, W multiples of 4")
    t = 4 if f4 else 2
    tiles = B * (H // t) * (W // t)
    # the operand V of the GEMMs: fp32 [T, tiles, C] (planes = 0), or -- f16 -- the two-term split of the transform times v_scale as [h | l]
    # (2 C wide, for our own GEMM kernel, which forms the three products itself: wino_gemm_f16x2, weights in operand order) or
    # as the three planes the library's K-concatenated GEMM wants (3 C wide)
    planes, v_scale, mscale = 0, 1.0, 1.0
    if f16 is not None:
        f16 = F16Gemm(*f16)
        # |B^T d B| <= amp * max|d| (amp = squared max abs row sum of B^T: 100 for F(4x4,3x3), 4 for F(2x2,3x3)); with gn, the
        # bound is that of SiLU(GroupNorm(x)), the tensor the transform actually sees
        v_scale = _pow2_scale(f16.bound, 100.0 if f4 else 4.0)
        use_own = f16.wf2 is not None and tiles % 256 == 0 and own_gemm_fits(T, tiles, cout, C)
        planes, mscale = 2 if use_own else 3, 1.0 / (v_scale * f16.u_scale)
    dev = x.device
    # 1. input transform (with the GroupNorm + SiLU of gn applied on the way)
    V = torch.empty((T, tiles, (planes or 1) * C), dtype=torch.float16 if planes else x.dtype, device=dev)
    _wino_in(lib(), x, V, gn, t, planes, v_scale)
    # 2. the 16 / 36 GEMMs [tiles, Cin] x [Cin, Cout], fp32 accumulation
    if planes == 2:
        M = torch.empty((T, tiles, cout), dtype=torch.float32, device=dev)
        _call("wino_gemm_f16x2", dev, V, f16.wf2, M, T, tiles, C, cout)
        del V                                                 # (this route has always freed its operand before y is taken)
    elif planes == 3:
        M = torch.bmm(V, f16.U3, out_dtype=torch.float32)         # ONE fp16 GEMM per tile position
    else:
        M = torch.bmm(V, U)                                   # hipBLASLt
    # 3. output transform (with bias, residual and the statistics of the result when asked for)
    if stats_groups:
        _need_residual("wino_conv3x3", residual, (B, cout, H, W))
        if not gn_nhwc_ok(cout, stats_groups):
            raise GqHipError("wino_conv3x3: the fused tail needs a GroupNorm-compatible Cout")
        y, stats = _out_and_stats(x, cout, H, W, stats_groups)
        _call("wino_out_res_nhwc_f32", dev, M, residual, bias, y, stats, B, H, W, cout, stats_groups, t, mscale)
        return y, stats
    y = _out_nhwc(x, cout, H, W)
    _call("wino4_out_nhwc_f32" if f4 else "wino_out_nhwc_f32", dev, M, y, B, H, W, cout, mscale)
    return y


def _wino_in(L, x, V, gn, t: int, planes: int, v_scale: float) -> None:
    """wino_conv3x3's input transform of F(t x t, 3x3) into V, by one of six entry points: fp32 (``planes`` 0), or the fp16
    operand of 2 | 3 planes scaled by v_scale; ``gn``: with the GroupNorm in front.  ``L``: the loaded library, as tests and
    tools that drive the transform alone have always passed it; the call goes through _call like every other."""
    B, C, H, W = x.shape
    f16_args = (t, v_scale) if planes else ()
    if gn is None:
        name = {0: "wino4_in_nhwc_f32" if t == 4 else "wino_in_nhwc_f32", 2: "wino_in_nhwc_f16x2", 3: "wino_in_nhwc_f16x3"}[planes]
        _call(name, x.device, x, V, B, H, W, C, *f16_args)
    else:
        name = {0: "wino4_in_gn_nhwc_f32" if t == 4 else "wino_in_gn_nhwc_f32", 2: "wino_in_gn_nhwc_f16x2",
                3: "wino_in_gn_nhwc_f16x3"}[planes]
        gn = GnFold(*gn)
        _call(name, x.device, x, gn.gamma, gn.beta, gn.pre_bias, gn.stats, V, B, H, W, C, gn.groups, gn.eps, bool(gn.silu), *f16_args)


_BMM_OUT_DTYPE = None


def bmm_out_dtype_ok(device) -> bool:
    """torch.bmm / torch.mm(..., out_dtype=torch.float32) on fp16 operands (fp32 accumulation AND fp32 result: what the fp16 x 3
    library-GEMM routes need) exists in recent PyTorch-ROCm only.  Probed once, on the device, with a 16 x 16 product; the conv
    stack takes its fp32-GEMM routes when it is missing (pit_hip/modules/unet.py) instead of raising a TypeError mid-forward."""
    global _BMM_OUT_DTYPE
    if _BMM_OUT_DTYPE is None:
        try:
            a = torch.ones(1, 16, 16, dtype=torch.float16, device=device)
            _BMM_OUT_DTYPE = bool(torch.bmm(a, a, out_dtype=torch.float32).dtype == torch.float32)
        except (TypeError, RuntimeError):
            _BMM_OUT_DTYPE = False
    return _BMM_OUT_DTYPE


ATTN_L_OK = (64, 256, 1024, 2304, 4096)   # token counts attn_softmax_split_f16x3 is instantiated for


def attention_scales(q_bound: float, v_bound: float):
    """(sq, sv): the powers of two that bring q, k (|.| <= q_bound) and v (<= v_bound) inside fp16's range for attention_f16x3."""
    # q k^T sums C products of scaled operands in fp32: keep sq^2 C q_bound^2 well inside fp32 (it always is: <= 2^30 C)
    return _pow2_scale(q_bound), _pow2_scale(v_bound)


def attention_operands(B: int, Ltok: int, C: int, device):
    """Uninitialised (Q3 [B, L, 3C], K3 [B, L, 3C], V3 [B, 3L, C]) fp16: the operands of attention_f16x3's two GEMMs."""
    return (torch.empty((B, Ltok, 3 * C), dtype=torch.float16, device=device),
            torch.empty((B, Ltok, 3 * C), dtype=torch.float16, device=device),
            torch.empty((B, 3 * Ltok, C), dtype=torch.float16, device=device))


def attention_from_operands(Q3, K3, V3, sq: float, sv: float):
    """attention_f16x3 from ready operands (attn_split_qkv_f16x3's, or those the q | k | v projection wrote itself:
    qkv_split_direct).  Returns (O_raw [B, L, C] fp32, post_scale)."""
    B, Ltok, C3 = Q3.shape
    C = C3 // 3
    if Ltok not in ATTN_L_OK:
        raise GqHipError("attention_f16x3: token count %d not in %s" % (Ltok, ATTN_L_OK))
    S = torch.bmm(Q3, K3.transpose(1, 2), out_dtype=torch.float32)
    P3 = torch.empty((B, Ltok, 3 * Ltok), dtype=torch.float16, device=Q3.device)
    _call("attn_softmax_split_f16x3", Q3.device, S, P3, B * Ltok, Ltok, float(C) ** -0.5 / (sq * sq))
    O = torch.bmm(P3, V3, out_dtype=torch.float32)
    return O, 1.0 / (16384.0 * sv)


def attention_f16x3(qkv, q_bound: float, v_bound: float):
    """softmax(q k^T C^-1/2) v for the fused projection qkv [B, L, 3C] fp32 (dense), single head: two library fp16 GEMMs with
    fp32 accumulation over K axes of two-term fp16 splits (gqhip.h:attn_split_qkv_f16x3) -- fp32-grade results at several
    times the rate of the fp32 GEMMs (a split-bf16 emulation on gfx950).  ``q_bound`` >= max(|q|, |k|), ``v_bound`` >= max|v|
    (rigorous bounds from the caller: GroupNorm bound x weight row sums).  Returns (O_raw [B, L, C] fp32, post_scale) with
    attention output = O_raw * post_scale (a power of two the consumer folds into its own scale)."""
    if not (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.is_contiguous() and qkv.shape[2] % 12 == 0):
        raise GqHipError("attention_f16x3 needs a dense fp32 HIP tensor [B, L, 3C], C % 4 == 0")
    B, Ltok, C3 = qkv.shape
    C = C3 // 3
    if Ltok not in ATTN_L_OK:
        raise GqHipError("attention_f16x3: token count %d not in %s" % (Ltok, ATTN_L_OK))
    sq, sv = attention_scales(q_bound, v_bound)
    Q3, K3, V3 = attention_operands(B, Ltok, C, qkv.device)
    _call("attn_split_qkv_f16x3", qkv.device, qkv, Q3, K3, V3, B, Ltok, C, sq, sv)
    return attention_from_operands(Q3, K3, V3, sq, sv)


def own_gemm_fits(positions: int, tiles: int, cout: int, cin: int = 256) -> bool:
    """Where wino_gemm_f16x2 replaces the library's K-concatenated GEMM: wherever its grid (128 x 256 tiles, two blocks per CU, at
    Cout % 256 == 0 and Cin % 64 == 0 -- the same number of rounds as the 256 x 256 tiles, one per CU, counted below -- else
    256 x 128) fills whole rounds of the chip reasonably (36 x 1024 tiles x 512 channels = 288 blocks = 1.125 rounds does
    not).  Alone the kernel is 1.05-1.21x the library at 256 input channels and at 16 x 4096 tiles, 0.91-0.95x at the two largest
    512-channel shapes (tools/wino_gemm2_bench.py) -- but its [h | l] operand also takes a third off what the input transform
    writes, so the step as a whole is faster with it everywhere (33.9 -> 33.4 ms)."""
    if cout % 256 == 0 and cin % 64 == 0:
        rounds = positions * (tiles // 256) * (cout // 256) / 256.0      # 8-wave blocks, one per CU
    else:
        rounds = positions * (tiles // 256) * (cout // 128) / 512.0      # 4-wave blocks, two per CU
    return rounds >= 1.0 and rounds / math.ceil(rounds) >= 0.85


def wino_weights_operand_order(h, l):
    """(U_h, U_l) [T, Cin, Cout] fp16 -> Wf [T, Cin/16, Cout/32, 2, 64, 8]: the B operands of v_mfma_f32_32x32x16_f16 as
    wino_gemm_f16x2 loads them (lane (c, hh) of column tile nt: k = 16 chunk + 8 hh .. + 7 of column 32 nt + c)."""
    T, cin, cout = h.shape
    planes = torch.stack([h, l], 0).reshape(2, T, cin // 16, 2, 8, cout // 32, 32)   # [pl, t, kc, hh, e, nt, c]
    return planes.permute(1, 2, 5, 0, 3, 6, 4).reshape(T, cin // 16, cout // 32, 2, 64, 8).contiguous()


def conv3_weights_f16(weight):
    """Operand-order fp16 x 3 weights of a [Cout, Cin, 3, 3] kernel for conv3x3_direct: (Wf [Cin/16, 9, Cout/32, 2, 64, 8]
    fp16, u_scale) -- see gqhip.h:conv3x3_gn_f16x3."""
    cout, cin, kk = weight.shape[0], weight.shape[1], weight.shape[2]
    if (cout % 128 if kk == 1 else cout not in (128, 256)) or cin % 16 or tuple(weight.shape[2:]) not in ((3, 3), (1, 1)):
        raise GqHipError("conv3_weights_f16 needs a [128 | 256, Cin % 16 == 0, 3, 3] or [Cout % 128 == 0, Cin % 16 == 0, 1, 1] kernel")
    hi, lo, u_scale = _split_f16(weight)
    planes = torch.stack([hi, lo], 0)                                    # [plane, n, k, ky, kx]
    # n = 32 tile + c, k = 16 chunk + 8 h + e  ->  [chunk, ky, kx, tile, plane, h, c, e]
    p7 = planes.reshape(2, cout // 32, 32, cin // 16, 2, 8, kk, kk).permute(3, 6, 7, 1, 0, 4, 2, 5)
    return p7.reshape(cin // 16, kk * kk, cout // 32, 2, 64, 8).contiguous(), u_scale


def conv3x3_direct(x, wf, u_scale: float, x_bound: float, gn, residual=None, bias=None, stats_groups: int = 0):
    """3x3 stride-1 padding-1 convolution Cin -> Cout (128 or 256) of SiLU(GroupNorm(x)) for a channels_last fp32 HIP tensor x, as
    a direct (implicit GEMM) fp16 x 3 convolution with the normalisation applied while the patch is staged
    (gqhip.h:conv3x3_gn_f16x3); ``wf, u_scale`` from conv3_weights_f16, ``x_bound`` >= max|activated tensor|, ``gn`` as in
    wino_conv3x3.  Returns y, or (y, statistics of y) when ``stats_groups`` > 0 (+ bias, + residual in either case)."""
    _need_nhwc("conv3x3_direct", x, c=32, h=8, w=32)
    if x.shape[1] > 512 or gn is None:
        raise GqHipError("conv3x3_direct needs C <= 512 and the GroupNorm that feeds the convolution")
    B, C, H, W = x.shape
    cout = wf.shape[2] * 32
    if wf.shape[0] * 16 != C:
        raise GqHipError("conv3x3_direct: weights are for %d input channels, x has %d" % (wf.shape[0] * 16, C))
    _need_residual("conv3x3_direct", residual, (B, cout, H, W))
    v_scale = _pow2_scale(x_bound)
    mscale = 1.0 / (v_scale * u_scale)
    gn = GnFold(*gn)
    y, ostats = _out_and_stats(x, cout, H, W, stats_groups)
    _call("conv3x3_gn_f16x3", x.device, x, gn.gamma, gn.beta, gn.pre_bias, gn.stats, gn.groups, gn.eps, bool(gn.silu), v_scale, wf,
          bias, residual, y, ostats, B, H, W, C, cout, max(stats_groups, 1), mscale)
    return _y_or_both(y, ostats)


def _conv1_args(x, wf, u_scale: float, scale, gn, post_scale: float, what: str, pre_bias=None):
    """Shared checks of the 1x1 routes (``gn``: a GnFold or None); returns _operand_scales' (device scales or None,
    v_scale, mscale).
    post_scale: x is post_scale^-1 times the tensor meant (a power of two its producer left pending)."""
    _need_nhwc(what, x, c=32, hw=128)
    if wf.shape[0] * 16 != x.shape[1] or wf.shape[1] != 1:
        raise GqHipError(what + ": weights do not match (need conv3_weights_f16 of a [Cout, %d, 1, 1] kernel)" % x.shape[1])
    if gn is not None and pre_bias is not None and pre_bias is not gn.pre_bias:
        raise GqHipError(what + ": with gn the pending bias is gn.pre_bias (the one its statistics include); pre_bias differs from it")
    if gn is not None and (torch.is_tensor(scale) or gn.silu or x.shape[1] > 512 or (x.shape[1] // gn.groups) % 4):
        raise GqHipError(what + ": the GroupNorm variant needs a host-side bound, no SiLU, C <= 512 and 4 | channels per group")
    if torch.is_tensor(scale) and post_scale != 1.0:
        raise GqHipError(what + ": post_scale needs a host-side scale bound")
    return _operand_scales(scale, u_scale, post_scale)


def conv1x1_direct(x, wf, u_scale: float, scale, residual=None, bias=None, stats_groups: int = 0, pre_bias=None,
                   post_scale: float = 1.0, gn=None):
    """1x1 convolution Cin -> Cout (128 | 256 | 512 | 1536) of a channels_last fp32 HIP tensor as an fp16 x 3 GEMM over its pixels
    with the split of x inside the kernel (gqhip.h:conv1x1_f16x3).  ``wf, u_scale`` from conv3_weights_f16 of the [Cout, Cin, 1, 1]
    kernel; ``pre_bias``: per-channel bias still pending on x (added before the split); ``scale``: a float bound >=
    max|x + pre_bias|, or the device float[2] of f16_scales(statistics of x + pre_bias, 1.0, u_scale).
    ``gn`` (a GnFold with silu False and the statistics of x + pre_bias) as for conv3x3_direct: the convolution's
    input is GroupNorm(x + pre_bias), normalised while it is staged (gqhip.h:conv1x1_gn_f16x3); ``scale`` then bounds the
    normalised tensor."""
    gn = None if gn is None else GnFold(*gn)
    sdev, v_scale, mscale = _conv1_args(x, wf, u_scale, scale, gn, post_scale, "conv1x1_direct", pre_bias)
    B, C, H, W = x.shape
    cout = wf.shape[2] * 32
    _need_residual("conv1x1_direct", residual, (B, cout, H, W))
    y, ostats = _out_and_stats(x, cout, H, W, stats_groups)
    if gn is not None:
        _call("conv1x1_gn_f16x3", x.device, x, gn.gamma, gn.beta, gn.pre_bias, gn.stats, gn.groups, gn.eps, wf, v_scale, mscale,
              bias, residual, y, ostats, B, H * W, C, cout, max(stats_groups, 1))
    else:
        _call("conv1x1_f16x3", x.device, x, pre_bias, wf, sdev, v_scale, mscale, bias, residual, y, ostats, B, H * W, C, cout,
              max(stats_groups, 1))
    return _y_or_both(y, ostats)


def qkv_split_direct(x, wf, u_scale: float, scale: float, sq: float, sv: float, bias=None, pre_bias=None, gn=None, out=None):
    """The attention block's q | k | v projection C -> 3C of conv1x1_direct (same arguments) whose epilogue writes the operands
    of attention_from_operands itself (gqhip.h:conv1x1_qkv_split_f16x3): (Q3, K3, V3), byte for byte those
    attn_split_qkv_f16x3(sq, sv) makes of the fp32 projection, which is never stored.  C % 128 == 0.  ``out``: the three
    operand tensors to fill (attention_operands' shapes, dense fp16) instead of fresh ones."""
    gn = None if gn is None else GnFold(*gn)
    _, v_scale, mscale = _conv1_args(x, wf, u_scale, float(scale), gn, 1.0, "qkv_split_direct", pre_bias)
    B, C, H, W = x.shape
    if wf.shape[2] * 32 != 3 * C or C % 128:
        raise GqHipError("qkv_split_direct: needs the [3C, C, 1, 1] projection, C % 128 == 0")
    gn = gn if gn is not None else _NO_GN._replace(pre_bias=pre_bias)
    Q3, K3, V3 = attention_operands(B, H * W, C, x.device) if out is None else out
    for t, shape in zip((Q3, K3, V3), ((B, H * W, 3 * C), (B, H * W, 3 * C), (B, 3 * H * W, C))):
        if not (t.is_cuda and t.dtype == torch.float16 and tuple(t.shape) == shape and t.is_contiguous()):
            raise GqHipError("qkv_split_direct: out must be dense fp16 [B, L, 3C], [B, L, 3C], [B, 3L, C]")
    _call("conv1x1_qkv_split_f16x3", x.device, x, gn.gamma, gn.beta, gn.pre_bias, gn.stats, gn.groups, gn.eps, wf, v_scale, mscale,
          bias, Q3, K3, V3, sq, sv, B, H * W, C)
    return Q3, K3, V3


def conv3s2_weights_f16(weight):
    """Operand-order fp16 x 3 weights of a [Cout, Cin, 3, 3] kernel for conv3x3s2_direct (stride 2): k-steps in the order
    (phase, chunk, tap of the phase) -- gqhip.h:conv3x3s2_f16x3.  Returns (Wf [9 Cin/16, Cout/32, 2, 64, 8], u_scale)."""
    cout, cin = weight.shape[0], weight.shape[1]
    if cout not in (128, 256, 512) or cin % 16 or tuple(weight.shape[2:]) != (3, 3):
        raise GqHipError("conv3s2_weights_f16 needs a [128 | 256 | 512, Cin % 16 == 0, 3, 3] kernel")
    hi, lo, u_scale = _split_f16(weight)
    planes = torch.stack([hi, lo], 0)                                    # [plane, n, k, ky, kx]
    std = planes.reshape(2, cout // 32, 32, cin // 16, 2, 8, 3, 3).permute(3, 6, 7, 1, 0, 4, 2, 5)   # [chunk, ky, kx, tile, plane, h, c, e]
    steps = []
    for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
        taps = [(dy, dx) for dy in range(2 if a == 0 else 1) for dx in range(2 if b == 0 else 1)]
        for chunk in range(cin // 16):
            for dy, dx in taps:
                steps.append(std[chunk, 2 * dy + a, 2 * dx + b])
    return torch.stack(steps, 0).reshape(9 * (cin // 16), cout // 32, 2, 64, 8).contiguous(), u_scale


def conv3x3s2_direct(x, wf, u_scale: float, scale, bias=None, stats_groups: int = 0):
    """The reference's Downsample convolution -- F.pad(x, (0, 1, 0, 1)) then 3x3 stride 2 -- of a channels_last fp32 HIP tensor
    as an fp16 x 3 convolution on the four phase images (gqhip.h:conv3x3s2_f16x3).  ``wf, u_scale`` from conv3s2_weights_f16;
    ``scale``: a float bound >= max|x| or the device float[2] of f16_scales.  Returns y [B, Cout, H/2, W/2] (+ bias), or
    (y, statistics of y)."""
    _need_nhwc("conv3x3s2_direct", x, c=16, h=16, w=64)
    B, C, H, W = x.shape
    cout = wf.shape[1] * 32
    if wf.shape[0] != 9 * (C // 16):
        raise GqHipError("conv3x3s2_direct: weights do not match the input channels")
    sdev, v_scale, mscale = _operand_scales(scale, u_scale)
    y, ostats = _out_and_stats(x, cout, H // 2, W // 2, stats_groups)
    _call("conv3x3s2_f16x3", x.device, x, wf, sdev, v_scale, mscale, bias, y, ostats, B, H, W, C, cout, max(stats_groups, 1))
    return _y_or_both(y, ostats)


def upconv_weights_f16(phase_matrix, cin: int, cout: int):
    """Operand-order fp16 x 3 weights of upconv2x_direct from the sub-pixel phase matrix [4 Cin, 4 Cout] (row (2u + v) Cin + ci,
    column (2a + b) Cout + co: Upsample._phase_weights): (Wf [4, 4 Cin/16, Cout/32, 2, 64, 8] fp16 -- [phase][chunk * 4 + tap]
    [column tile][plane][lane (hh, c)][e] = plane[tap, 16 chunk + 8 hh + e, phase, 32 tile + c] --, u_scale)."""
    if cout not in (128, 256, 512) or cin % 16 or tuple(phase_matrix.shape) != (4 * cin, 4 * cout):
        raise GqHipError("upconv_weights_f16 needs the [4 Cin, 4 Cout] phase matrix, Cin % 16 == 0, Cout in (128, 256, 512)")
    hi, lo, u_scale = _split_f16(phase_matrix)
    planes = torch.stack([hi, lo], 0).reshape(2, 4, cin // 16, 2, 8, 4, cout // 32, 32)   # [pl, tap, chunk, hh, e, phase, nt, c]
    wf = planes.permute(5, 2, 1, 6, 0, 3, 7, 4).reshape(4, 4 * (cin // 16), cout // 32, 2, 64, 8)
    return wf.contiguous(), u_scale


def upconv2x_direct(x, wf, u_scale: float, scale, bias=None, stats_groups: int = 0):
    """The reference's Upsample (nearest x2 + conv 3x3) of a channels_last fp32 HIP tensor as the direct sub-pixel fp16 x 3
    convolution (gqhip.h:upconv2x_f16x3).  ``wf, u_scale`` from upconv_weights_f16; ``scale``: a float bound >= max|x| or the
    device float[2] of f16_scales.  Returns y [B, Cout, 2H, 2W] (+ bias), or (y, statistics of y)."""
    _need_nhwc("upconv2x_direct", x, c=16, h=8, w=32)
    B, C, H, W = x.shape
    cout = wf.shape[2] * 32
    if wf.shape[0] != 4 or wf.shape[1] != 4 * (C // 16):
        raise GqHipError("upconv2x_direct: weights do not match the input channels")
    sdev, v_scale, mscale = _operand_scales(scale, u_scale)
    y, ostats = _out_and_stats(x, cout, 2 * H, 2 * W, stats_groups)
    _call("upconv2x_f16x3", x.device, x, wf, sdev, v_scale, mscale, bias, y, ostats, B, H, W, C, cout, max(stats_groups, 1))
    return _y_or_both(y, ostats)


def conv3x3_gn_small(x, w_ohwi, bias, gn):
    """conv3x3(SiLU(GroupNorm(x))) into 1..4 channels (gqhip.h:conv3x3_gn_small_f32): x channels_last fp32 [B, Cin, H, W],
    w_ohwi [Cout, 3, 3, Cin] fp32 contiguous, ``gn``: a GnFold."""
    _need_nhwc("conv3x3_gn_small", x, c=32, h=16, w=16)
    B, C, H, W = x.shape
    cout = w_ohwi.shape[0]
    if tuple(w_ohwi.shape) != (cout, 3, 3, C) or not w_ohwi.is_contiguous() or w_ohwi.dtype != torch.float32:
        raise GqHipError("conv3x3_gn_small: weights must be fp32 [Cout, 3, 3, Cin] contiguous")
    gn = GnFold(*gn)
    y = _out_nhwc(x, cout, H, W)
    _call("conv3x3_gn_small_f32", x.device, x, gn.gamma, gn.beta, gn.pre_bias, gn.stats, gn.groups, gn.eps, bool(gn.silu), w_ohwi,
          bias, y, B, H, W, C, cout)
    return y


def checksum_table(tensors):
    """Device table for checksum_tensors: one {pointer, 32-bit words} entry per tensor (dense fp32 / int32 HIP tensors)."""
    dev = tensors[0].device
    rows = []
    for t in tensors:
        if not (t.is_cuda and t.element_size() == 4 and t.data_ptr() % 16 == 0 and t.device == dev):
            raise GqHipError("checksum_table needs 16-byte aligned 4-byte-element tensors on one HIP device")
        rows += [t.data_ptr(), t.numel()]
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def checksum_tensors(table, out):
    """out[t] (int64, device) = content hash of tensor t of ``table`` (gqhip.h:gqhip_checksum_tensors); asynchronous."""
    _call("gqhip_checksum_tensors", table.device, table, table.numel() // 2, out)
    return out


def conv_f32_ok(cin: int, cout: int, H: int, W: int, gn: bool) -> bool:
    """Shapes conv3x3_f32 tiles (gqhip.h)."""
    return cout % 4 == 0 and (cin % 64 == 0 and (not gn or cin <= 1024) or (not gn and cin in (8, 16, 32)))


def conv_f32_weights(weight):
    """[Cout, Cin, 3, 3] fp32 -> the operand order of conv3x3_f32: [ceil(Cout/32)][9][Cin/8][64][4], element
    (t, tap, g, 32 h + j, m) = w[32 t + j][8 g + 4 h + m][tap // 3][tap % 3], zero rows beyond Cout."""
    cout, cin = weight.shape[0], weight.shape[1]
    if cin % 8 or tuple(weight.shape[2:]) != (3, 3):
        raise GqHipError("conv_f32_weights needs a [Cout, Cin % 8 == 0, 3, 3] weight")
    nt = (cout + 31) // 32
    w = weight.detach().float().reshape(cout, cin, 9)
    if nt * 32 != cout:
        w = torch.cat([w, w.new_zeros(nt * 32 - cout, cin, 9)], 0)
    return w.reshape(nt, 32, cin // 8, 2, 4, 9).permute(0, 5, 2, 3, 1, 4).contiguous()


def conv3x3_f32(x, wk, cout: int, bias=None, gn=None):
    """3x3 convolution (stride 1, padding 1) of a channels_last fp32 HIP tensor on the fp32 matrix cores with a fixed summation
    order (gqhip.h:conv3x3_f32: bit-reproducible).  ``wk`` from conv_f32_weights; ``gn`` (a GnFold): the input is
    act(GroupNorm(x + pre_bias)), applied while the patch is staged."""
    _need_nhwc("conv3x3_f32", x)
    B, C, H, W = x.shape
    if not conv_f32_ok(C, cout, H, W, gn is not None) or wk.numel() != ((cout + 31) // 32) * 9 * (C // 8) * 256:
        raise GqHipError(f"conv3x3_f32: shape {tuple(x.shape)} -> {cout} channels is not tiled by the kernel")
    y = _out_nhwc(x, cout, H, W)
    gn = _NO_GN if gn is None else GnFold(*gn)
    _call("conv3x3_f32", x.device, x, gn.gamma, gn.beta, gn.pre_bias, gn.stats, gn.groups, gn.eps, bool(gn.silu), wk, bias, y,
          B, H, W, C, cout)
    return y


def conv_cin_small_ok(cin: int, cout: int, H: int, W: int) -> bool:
    """Shapes conv3x3_cin_small_f32 tiles (gqhip.h): the encoder's conv_in."""
    return 1 <= cin <= 4 and cout == 128 and H % 8 == 0 and W % 32 == 0 and H >= 8 and W >= 32


def conv_cin_small_weights(weight):
    """[128, Cin <= 4, 3, 3] fp32 -> [9 Cin, 128]: row tap * Cin + ci, column co."""
    cout, cin = weight.shape[0], weight.shape[1]
    return weight.detach().float().permute(2, 3, 1, 0).reshape(9 * cin, cout).contiguous()


def conv3x3_cin_small(x, wk, bias=None, stats_groups: int = 0):
    """The encoder's conv_in on libgqhip (gqhip.h:conv3x3_cin_small_f32): 3x3 / stride 1 / pad 1, Cin <= 4 -> 128 channels of a
    channels_last fp32 HIP image, fp32 FMAs in a fixed order, bias added; ``stats_groups`` = 32: returns (y, statistics of y)."""
    _need_nhwc("conv3x3_cin_small", x)
    B, C, H, W = x.shape
    if not conv_cin_small_ok(C, wk.shape[1], H, W) or wk.shape[0] != 9 * C or stats_groups not in (0, 32):
        raise GqHipError(f"conv3x3_cin_small: shape {tuple(x.shape)} is not tiled by the kernel")
    y, ostats = _out_and_stats(x, 128, H, W, 32 if stats_groups else 0)
    _call("conv3x3_cin_small_f32", x.device, x, wk, bias, y, ostats, B, H, W, C, 128, 32)
    return _y_or_both(y, ostats)


def f16_scales(stats, amp: float, u_scale: float):
    """Device float[2] = (v_scale, 1 / (v_scale * u_scale)) for an fp16 x 3 GEMM whose activation operand x has the
    GroupNorm statistics ``stats`` (n_bg records of GNSTAT_WORDS int64: gqhip_gnstat_t): v_scale = the largest power of two with
    amp * sqrt(max sum of squares) * v_scale <= 32768.  Computed on the device (no sync)."""
    if not (stats.is_cuda and stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() % GNSTAT_WORDS == 0):
        raise GqHipError("f16_scales needs the statistics tensor of add_bias_stats / wino_conv3x3")
    out = torch.empty(2, dtype=torch.float32, device=stats.device)
    _call("f16_scales_from_gn_stats", stats.device, stats, stats.numel() // GNSTAT_WORDS, amp, u_scale, out)
    return out


def upsample2x_nhwc(x):
    """Nearest x2 upsample of a channels_last fp32 HIP tensor [B, C, H, W] -> [B, C, 2H, 2W] (channels_last)."""
    _need_nhwc("upsample2x_nhwc", x, c=4)
    B, C, H, W = x.shape
    y = _out_nhwc(x, C, 2 * H, 2 * W)
    _call("upsample2x_nhwc_f32", x.device, x, y, B, H, W, C)
    return y


def index_histogram(idx, n: int):
    idx = _dev(idx, torch.int64, "indices")
    hist = torch.empty(n, dtype=torch.int32, device=idx.device)
    _call("gq_index_histogram", idx.device, idx, idx.numel(), n, hist)
    return hist


def indices_to_u16(idx):
    idx = _dev(idx, torch.int64, "indices")
    out = torch.empty(idx.shape, dtype=torch.uint16, device=idx.device)
    _call("gq_indices_to_u16", idx.device, idx, out, idx.numel())
    return out


def indices_from_u16(u16):
    if not (u16.is_cuda and u16.dtype == torch.uint16):
        raise GqHipError("expected a uint16 HIP tensor")
    u16 = u16.contiguous()
    out = torch.empty(u16.shape, dtype=torch.int64, device=u16.device)
    _call("gq_indices_from_u16", u16.device, u16, out, u16.numel())
    return out


def _zeroed_ws(ws_cache: dict, key, need: int, device):
    """The zero-in / zero-out scratch of a metric call, kept in the caller's dict under ``key``: zeroed once, left zero by every
    call that uses it."""
    ws = ws_cache.get(key)
    if ws is None:
        ws = ws_cache[key] = torch.zeros(max(need, 8), dtype=torch.uint8, device=device)
    return ws


def _image_pair_ok(x, x_rec, need_items: bool) -> bool:
    """fp32 HIP images [B, C, H, W] of one shape, one device and one dense layout (NCHW or channels_last); ``need_items``: B >= 1
    and a non-empty image as well."""
    if not (x.is_cuda and x_rec.is_cuda and x.device == x_rec.device and x.dtype == torch.float32 and x_rec.dtype == torch.float32
            and x.dim() == 4 and x.shape == x_rec.shape and (not need_items or (x.shape[0] > 0 and x[0].numel() > 0))):
        return False
    la, lb = image_layout(x), image_layout(x_rec)
    return la is not None and la == lb


def step_record_ok(x, x_rec, idx) -> bool:
    """The record kernels apply: _image_pair_ok images, int64 indices on a HIP device.  (Images on two devices are refused like
    everything else the kernels do not take; this predicate used to pass them on.)"""
    return idx.is_cuda and idx.dtype == torch.int64 and _image_pair_ok(x, x_rec, False)


def ssim_ok(x, x_rec) -> bool:
    """gq_ssim_f32 applies: _image_pair_ok images, B >= 1."""
    return _image_pair_ok(x, x_rec, True)


def step_record(x, x_rec, idx, rec, ws_cache: dict, n_metrics: int = 1, index_bits: Optional[int] = None,
                n_codes: Optional[int] = None):
    """rec[:] = [ B x n_metrics metric words | index words ] of one rank's step (gqhip.h: gq_step_record*_f32; eval.py:152-154,
    165-178).  n_metrics 1: per-image PSNR(x, x_rec; zero_mean) as fp32 bits, ONE launch; 3: (PSNR, SSIM, MS-SSIM), the PSNR words
    those of n_metrics 1 bit for bit.  ``index_bits`` None: idx as uint16 pairs; else the bit-packed stream of that width and the
    violations word (indices outside [0, n_codes)) behind it.  ``ws_cache``: the caller's dict that keeps the (zeroed, self-
    resetting) workspace between calls."""
    B, C, H, W = x.shape
    bits = index_bits is not None
    if n_metrics == 1:
        kind, shape = "gq_step_record", (B, C * H * W)
        image = shape
    elif n_metrics == 3:
        kind, shape, image = "gq_step_record_ssim", (B, C, H, W), (B, C, H, W, image_layout(x))
    else:
        raise GqHipError(f"step_record: n_metrics is 1 or 3, not {n_metrics}")
    kind += "_bits" if bits else ""
    wire = (index_bits, n_codes) if bits else ()
    idx = idx.contiguous()      # (any memory order of the SAME logical [B, K, h, w] order is fine for the caller; contiguous = logical order)
    need = getattr(lib(), kind + "_workspace_bytes")(*shape)
    ws = _zeroed_ws(ws_cache, ("bits" if bits else "u16", n_metrics, x.device, B, C, H, W), need, x.device)
    _call(kind + "_f32", x.device, x, x_rec, idx, rec, *image, idx.numel(), *wire, ws, ws.numel())
    return rec


def image_quality(x, x_rec, zero_mean: bool, msssim: bool, ws_cache: dict):
    """Per-image (SSIM, MS-SSIM or None) as fp32 [B] tensors on x's device (gqhip.h: gq_ssim_f32; pit/evaluations/ssim.py:5-63).
    MS-SSIM is NaN when a side is under 256.  ``ws_cache``: the caller's dict that keeps the self-resetting workspace."""
    B, C, H, W = x.shape
    layout = image_layout(x)
    ssim = torch.empty(B, dtype=torch.float32, device=x.device)
    ms = torch.empty(B, dtype=torch.float32, device=x.device) if msssim else None
    ws = _zeroed_ws(ws_cache, ("ssim", x.device, B, C, H, W), lib().gq_ssim_workspace_bytes(B, C, H, W), x.device)
    _call("gq_ssim_f32", x.device, x, x_rec, B, C, H, W, layout, bool(zero_mean), ssim, ms, ws, ws.numel())
    return ssim, ms


def _words_out(t, n_words: int, what: str):
    """A caller's int32 output of ``n_words`` contiguous words on a HIP device (a slice of a record, say)."""
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n_words):
        raise GqHipError(f"{what} must be {n_words} contiguous int32 words on a HIP device")
    return t


def indices_pack_bits(idx, index_bits: int, n_codes: int, out=None, violations=None):
    """The bit-packed index stream of ``idx`` (int64, any shape, logical order): int32 [ceil(count index_bits / 32)] (gqhip.h:
    gq_indices_pack_bits).  ``out``: write the words there; ``violations``: a one-element int32 tensor that receives the number of
    indices outside [0, n_codes).  No host read."""
    idx = _dev(idx, torch.int64, "indices")
    n_words = (idx.numel() * index_bits + 31) // 32
    out = torch.empty(n_words, dtype=torch.int32, device=idx.device) if out is None else _words_out(out, n_words, "out")
    if violations is not None:
        _words_out(violations, 1, "violations")
    _call("gq_indices_pack_bits", idx.device, idx, out, idx.numel(), index_bits, n_codes, violations)
    return out


def _packed_records(records, what: str):
    if not (records.is_cuda and records.dtype == torch.int32 and records.dim() == 2):
        raise GqHipError(f"{what}: records must be an int32 [n_records, words] tensor on a HIP device")
    return records if records.is_contiguous() else records.contiguous()


def indices_unpack_bits(records, offset_words: int, count: int, index_bits: int):
    """int64 [n_records, count]: the ``count`` indices of ``index_bits`` bits that start ``offset_words`` into each row of the
    int32 [n_records, words] tensor ``records`` (gqhip.h: gq_indices_unpack_bits)."""
    records = _packed_records(records, "indices_unpack_bits")
    out = torch.empty((records.shape[0], count), dtype=torch.int64, device=records.device)
    _call("gq_indices_unpack_bits", records.device, records, out, records.shape[0], records.shape[1], offset_words, count, index_bits)
    return out


def index_histogram_packed(records, offset_words: int, count: int, index_bits: int, hist):
    """hist (int64 [n], HIP) += the counts of the packed indices of ``records`` (as in indices_unpack_bits); values >= n are skipped
    (gqhip.h: gq_index_histogram_packed).  The int64 indices are never formed."""
    records = _packed_records(records, "index_histogram_packed")
    if not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.dim() == 1 and hist.device == records.device):
        raise GqHipError("index_histogram_packed: hist must be a contiguous int64 [n] tensor on the records' device")
    _call("gq_index_histogram_packed", records.device, records, records.shape[0], records.shape[1], offset_words, count, index_bits,
          hist.numel(), hist)
    return hist


def moments_state_words(D: int) -> int:
    """fp64 words of the moments state of D features, [outer: D D | sum: D | count: 1] (gqhip.h: gq_moments_state_bytes)."""
    need = lib().gq_moments_state_bytes(D)
    if need < 0:
        raise GqHipError(f"unsupported shape D={D}")
    return need // 8


def moments_update(x, state):
    """state += the raw moments of the rows of ``x`` (gqhip.h: gq_moments_update_f32), in ascending row order, bit for bit what a
    sequential fp64 loop gives.  ``x``: fp32 [rows, D] on a HIP device with unit inner stride (a column slice of a wider tensor
    passes: its row stride goes to the library); there is no silent ``.float()``, the exactness argument needs fp32 inputs.
    ``state``: contiguous fp64 with D D + D + 1 elements on the same device, zeroed once by its owner.  Returns ``state``."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"moments_update: x must be a float32 [rows, D] tensor with unit inner stride, got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))} strides {getattr(x, 'stride', tuple)()}")
    rows, D = x.shape
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or not state.is_contiguous() \
            or state.numel() != D * D + D + 1:
        raise ValueError(f"moments_update: state must be a contiguous float64 tensor of D D + D + 1 = {D * D + D + 1} elements, got "
                         f"{getattr(state, 'dtype', type(state))} {tuple(getattr(state, 'shape', ()))}")
    if not (x.is_cuda and state.is_cuda and x.device == state.device):
        raise GqHipError(f"moments_update: x and state must be on one HIP device (got {x.device}, {state.device}); "
                         "the HIP path has no CPU fallback")
    if rows == 0:                                       # an empty tensor has no pointer to hand over
        return state
    row_stride = x.stride(0) if rows > 1 else max(x.stride(0), D)      # the stride of a one-row view is arbitrary
    if row_stride < D:
        raise ValueError(f"moments_update: x must not overlap its own rows (row stride {row_stride} < D = {D})")
    _call("gq_moments_update_f32", x.device, x, rows, D, row_stride, state)
    return state


MHA_HEAD_DIMS = (64,)    # head dims gq_mha_fwd_f32 is built for


def _mha_qkv(qkv: torch.Tensor, heads: int, who: str):
    """The validation every attention wrapper shares: qkv [B, L, 3E] fp32 on a HIP device, 16-byte aligned, a built head dim."""
    qkv = _dev(qkv, torch.float32, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] % 3 != 0 or heads < 1 or (qkv.shape[2] // 3) % heads != 0:
        raise GqHipError(f"{who}: qkv must be [B, L, 3E] with E divisible by heads={heads}, got {tuple(qkv.shape)}")
    B, L, E3 = qkv.shape
    E = E3 // 3
    if E // heads not in MHA_HEAD_DIMS:
        raise GqHipError(f"{who}: head dim {E // heads} is not built (built: {MHA_HEAD_DIMS})")
    if qkv.data_ptr() % 16 != 0:
        qkv = qkv.clone()
    return qkv, B, L, E


def mha_fwd(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v per (batch, head) from the in-projection output ``qkv`` [B, L, 3E] fp32 on a HIP device,
    read in place; returns [B, L, E] with the heads concatenated (gqhip.h: gq_mha_fwd_f32; pit/modules/vit.py:142-151)."""
    qkv, B, L, E = _mha_qkv(qkv, heads, "mha_fwd")
    out = torch.empty(B, L, E, dtype=torch.float32, device=qkv.device)
    need = lib().gq_mha_workspace_bytes(B, L, E, heads)         # 0 today: no scratch; otherwise per call, as in mha_bwd
    ws = torch.empty(need, dtype=torch.uint8, device=qkv.device) if need > 0 else None
    _call("gq_mha_fwd_f32", qkv.device, qkv, out, B, L, E, heads, ws)
    return out


def mha_fwd_lse(qkv: torch.Tensor, heads: int):
    """``mha_fwd`` for training: (out [B, L, E], lse [B, heads, L]) -- the same ``out`` bit for bit, and per query row the
    log-sum-exp of its scores in the kernel's units (times ln 2: of q k^T / sqrt(d)), which ``mha_bwd`` recomputes the softmax
    from (gqhip.h: gq_mha_fwd_lse_f32)."""
    qkv, B, L, E = _mha_qkv(qkv, heads, "mha_fwd_lse")
    out = torch.empty(B, L, E, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B, heads, L, dtype=torch.float32, device=qkv.device)
    _call("gq_mha_fwd_lse_f32", qkv.device, qkv, out, lse, B, L, E, heads, None)
    return out, lse


def mha_bwd(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, heads: int) -> torch.Tensor:
    """The gradient of ``qkv`` [B, L, 3E] (dq | dk | dv in qkv's layout) from ``out``, ``lse`` of ``mha_fwd_lse(qkv, heads)`` and
    ``dout``, the gradient of ``out`` (gqhip.h: gq_mha_bwd_f32; two kernels, no atomics, bit-reproducible)."""
    qkv, B, L, E = _mha_qkv(qkv, heads, "mha_bwd")
    out, lse = _dev(out, torch.float32, "out"), _dev(lse, torch.float32, "lse")
    dout = _dev(dout, torch.float32, "dout").contiguous()            # autograd hands out expanded (stride 0) gradients
    if tuple(out.shape) != (B, L, E) or tuple(dout.shape) != (B, L, E) or tuple(lse.shape) != (B, heads, L):
        raise GqHipError(f"mha_bwd: out / dout must be {(B, L, E)} and lse {(B, heads, L)}, got {tuple(out.shape)}, "
                         f"{tuple(dout.shape)}, {tuple(lse.shape)}")
    out, lse = out.contiguous(), lse.contiguous()
    if out.data_ptr() % 16 != 0:
        out = out.clone()
    if dout.data_ptr() % 16 != 0:
        dout = dout.clone()
    dqkv = torch.empty(B, L, 3 * E, dtype=torch.float32, device=qkv.device)
    # delta lives for this call only: from the caching allocator, so that calls on different streams never share it
    ws = torch.empty(max(lib().gq_mha_bwd_workspace_bytes(B, L, E, heads), 8), dtype=torch.uint8, device=qkv.device)
    _call("gq_mha_bwd_f32", qkv.device, qkv, out, lse, dout, dqkv, B, L, E, heads, ws)
    return dqkv


def profile_enable(on: bool) -> None:
    lib().gqhip_profile_enable(1 if on else 0)


def profile_reserve(pairs: int) -> None:
    """Pre-create event pairs so that profiled launches create nothing (call outside the timed region)."""
    _check(lib().gqhip_profile_reserve(int(pairs)), "gqhip_profile_reserve")


def profile_collect() -> Tuple[int, float]:
    n = ctypes.c_int(0)
    ms = ctypes.c_double(0.0)
    lib().gqhip_profile_collect(ctypes.byref(n), ctypes.byref(ms))
    return n.value, ms.value


def debug_enable(on: bool) -> None:
    lib().gqhip_debug_enable(1 if on else 0)


FILTER_KINDS = {"auto": 0, "fp32": 1, "bf16": 2, "mixed": 3}


def set_filter(kind: str) -> None:
    """"auto": fp16 + fp8 MFMA filter at dim 16 (Gaussian score), split-bf16 at the other MFMA dims and for VQ (other dims use
    the exhaustive kernel either way); "fp32": always the fp32 MFMA filter; "bf16": split-bf16 wherever it applies.
    Process-wide; indices are identical whichever runs (the exact re-rank decides)."""
    if kind not in FILTER_KINDS:
        raise GqHipError(f"unknown filter {kind!r} (expected one of {sorted(FILTER_KINDS)})")
    _check(lib().gqhip_set_filter(FILTER_KINDS[kind]), "gqhip_set_filter")


def get_filter() -> str:
    k = lib().gqhip_get_filter()
    return next(name for name, v in FILTER_KINDS.items() if v == k)


ODD_DIMS_KINDS = {"exhaustive": 0, "padded": 1}


def set_odd_dims(kind: str) -> None:
    """Route of the codebook dims 5-7, 9-15, 17-31: "exhaustive" (default): every code scored per row; "padded": zero-padded to the
    next filter dim (8, 16, 32) and run through filter + re-rank, which scores with the true dim.  Process-wide; every output is the
    same bits either way.  The workspace size depends on it (a ``Workspace`` asks the library on every call and grows by itself)."""
    if kind not in ODD_DIMS_KINDS:
        raise GqHipError(f"unknown odd-dims route {kind!r} (expected one of {sorted(ODD_DIMS_KINDS)})")
    _check(lib().gqhip_set_odd_dims(ODD_DIMS_KINDS[kind]), "gqhip_set_odd_dims")


def get_odd_dims() -> str:
    k = lib().gqhip_get_odd_dims()
    return next(name for name, v in ODD_DIMS_KINDS.items() if v == k)


LOW_DIMS_KINDS = {"exhaustive": 0, "search": 1}


def set_low_dims(kind: str) -> None:
    """Route of the Gaussian arg-max at codebook dims 1-3: "exhaustive" (default): every code scored per row; "search": with 4096
    to 2^20 codes, a pruned exact search over a cell index kept in the codebook cache (csrc/gq_lowdim.h).  Process-wide; every output
    is the same bits either way.  The cache size depends on it (a ``Workspace`` asks the library on every call)."""
    if kind not in LOW_DIMS_KINDS:
        raise GqHipError(f"unknown low-dims route {kind!r} (expected one of {sorted(LOW_DIMS_KINDS)})")
    _check(lib().gqhip_set_low_dims(LOW_DIMS_KINDS[kind]), "gqhip_set_low_dims")


def get_low_dims() -> str:
    k = lib().gqhip_get_low_dims()
    return next(name for name, v in LOW_DIMS_KINDS.items() if v == k)


WIDE_DIMS_KINDS = {"exhaustive": 0, "filter": 1}


def set_wide_dims(kind: str) -> None:
    """Route of the codebook dims 33-64: "exhaustive" (default): every code scored per row; "filter": with the filter selection
    "auto", filter + re-rank at dim 64 (dims 33-63 zero-padded to it; the re-rank scores with the true dim).  Process-wide; every
    output is the same bits either way.  The workspace size depends on it (a ``Workspace`` asks the library on every call and grows
    by itself)."""
    if kind not in WIDE_DIMS_KINDS:
        raise GqHipError(f"unknown wide-dims route {kind!r} (expected one of {sorted(WIDE_DIMS_KINDS)})")
    _check(lib().gqhip_set_wide_dims(WIDE_DIMS_KINDS[kind]), "gqhip_set_wide_dims")


def get_wide_dims() -> str:
    k = lib().gqhip_get_wide_dims()
    return next(name for name, v in WIDE_DIMS_KINDS.items() if v == k)


def low_dim_search_applies(n: int, dim: int) -> bool:
    """Whether a GQ call with ``n`` codes of width ``dim`` and a codebook cache runs the dims 1-3 search under the current selection."""
    return bool(lib().gqhip_low_dim_search_applies(n, dim))


def filter_dim(n: int, dim: int) -> int:
    """The dim the filter runs at for (n, dim) under the current selections; 0: the exhaustive kernel."""
    return int(lib().gqhip_filter_dim(n, dim))


def debug_plan(rows: int, n: int, dim: int) -> dict:
    out = (_i64 * 8)()
    _check(lib().gqhip_debug_plan(rows, n, dim, out), "gqhip_debug_plan")
    keys = ("rec_offset", "nsplit", "gt", "tiles_per_split", "bf16", "ef_coeff", "rt", "waves")
    return dict(zip(keys, (int(v) for v in out)))


def debug_records(ws: Workspace, rows: int, n: int, dim: int):
    """Candidate records the filter left in the workspace, decoded from their 16-byte form (csrc/gq_common.h:Rec):
    (m [sets, rows, 4] fp32: m1 and the re-rank's view m1 - gap of m2..m4; ids [sets, rows, 3] int32: GLOBAL half-group ids)."""
    pl = debug_plan(rows, n, dim)
    sets = pl["nsplit"]
    raw = ws.buf[pl["rec_offset"]: pl["rec_offset"] + sets * rows * 16].reshape(sets, rows, 16)
    m1 = raw[..., 0:4].contiguous().view(torch.float32)                                   # [sets, rows, 1]
    gaps = raw[..., 4:10].contiguous().view(torch.float16).to(torch.float64)               # [sets, rows, 3]
    m = torch.cat([m1.to(torch.float64), m1.to(torch.float64) - gaps], dim=-1).to(torch.float32)
    local = raw[..., 10:16].contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    halves = 2 if pl["bf16"] in (2, 3) else 1                                              # one set per (split, lane half)
    split = torch.arange(sets, device=raw.device, dtype=torch.int32) // halves
    base2 = 2 * ((split * pl["tiles_per_split"]) // pl["gt"])
    return m, local + base2[:, None, None]


def debug_grid(ws: Workspace) -> dict:
    """Grid search statistics of the last call on ``ws`` (counted only while ``debug_enable(True)``; synchronous)."""
    out = (_i64 * 4)()
    cptr = None if ws.cache_buf is None else ws.cache_buf.data_ptr()
    _check(lib().gqhip_debug_grid(ws.buf.data_ptr(), cptr, out), "gqhip_debug_grid")
    # out[0]: visited sub-leaves (1/4096 of the codebook each); "leaves": the same in leaves (four sub-leaves, 1/1024 of the codebook)
    return {"sub_leaves": out[0], "leaves": out[0] / 4.0, "exact_codes": out[1], "scanned_rows": out[2], "index_current": out[3]}


def debug_counters(ws: Workspace) -> Tuple[int, int]:
    fb, rr = _i64(0), _i64(0)
    _check(lib().gqhip_debug_counters(ws.buf.data_ptr(), ctypes.byref(fb), ctypes.byref(rr)), "gqhip_debug_counters")
    return fb.value, rr.value
