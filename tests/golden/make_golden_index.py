"""Pins the codebook index the one-block builders write (csrc/gq_index.h: dims 4 / 8 for gq_grid.h, dims 1-3 for gq_lowdim.h): per case
the sha256 of its deterministic parts -- the header words (magic, n, dim, stale, max_sub, the slice hashes, dims 4 / 8: the thresholds),
the start arrays, every level of boxes and the original indices sorted inside each bucket (their order in a bucket is a race).

    GQHIP_LIB=<libgqhip.so of the commit to record> python tests/golden/make_golden_index.py      # needs the MI355X

writes tests/golden/index_digests.json.  The committed file was recorded with the library built at the commit BEFORE the two builders
were made one (point GQHIP_LIB at such a build to regenerate it), so it holds the thresholds, and with them the fp64 summation
order of the moments, to what they were.  tests/test_gpu_index.py imports the layout model, the cases and the books from here.

The dim-8 index exists only under GQHIP_GRID=48, which the library reads once per process: its cases run in one child process
(`--dump FILE`), here and in the test."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
FIXTURE = os.path.join(HERE, "index_digests.json")

ROWS = 64
BOOKS = ("randn", "clustered")
GRID_DIMS, LOW_DIMS = (4, 8), (1, 2, 3)
CASES = tuple((d, n, b) for d in GRID_DIMS for n in (16384, 16384 + 37) for b in BOOKS) + \
        tuple((d, n, b) for d in LOW_DIMS for n in (4096, 4096 + 33) for b in BOOKS)
MAGIC = {"grid": 0x47514733, "low": 0x47514C31}
BUCKETS, PAD = 4096, 16
HDR_BYTES, WS_CBSUM = 4096, 4096       # GridHdr; byte offset of WsHeader::cbsum in the workspace
PARTS = 256                            # slice hashes


def case_id(case):
    return "dim%d-n%d-%s" % case


def kind_of(dim):
    return "grid" if dim in GRID_DIMS else "low"


def cap_of(n, dim):
    """bucket size above which gqhip_cb_cache_degenerate answers 1"""
    return 255 if kind_of(dim) == "grid" else max(n // 256, 256)


def _align(v):
    return (v + 255) // 256 * 256


def layout(n, dim):
    """grid_layout / low_layout: {region: (byte offset, element count)}, "total", and "levels": the box regions from the buckets up with
    the fan-in of each level above the first"""
    box = 2 * dim * 4
    if kind_of(dim) == "grid":
        regions = [("box1", 16 * box, "f"), ("box2", 256 * box, "f"), ("box3", 1024 * box, "f"), ("leaf_start", _align((1024 + PAD) * 4), "i"),
                   ("start", _align((BUCKETS + PAD) * 4), "i"), ("sbox", BUCKETS * box, "f")]
        levels = (("sbox", 0), ("box3", 4), ("box2", 4), ("box1", 16))
    else:
        regions = [("cbox", _align(256 * box), "f"), ("box", _align(BUCKETS * box), "f"), ("start", _align((BUCKETS + PAD) * 4), "i")]
        levels = (("box", 0), ("cbox", 16))
    regions += [("scb", _align(n * dim * 4), "f"), ("sidx", _align(n * 4), "i")]
    out, off = {"levels": levels}, HDR_BYTES
    for name, size, _ in regions:
        out[name] = off
        off += size
    out["total"] = off
    return out


def parse(raw, n, dim):
    """the cache's bytes -> its words by name"""
    L = layout(n, dim)
    assert raw.dtype == np.uint8 and raw.size >= L["total"]
    i32 = lambda off, cnt: raw[off:off + 4 * cnt].view(np.int32)
    f32 = lambda off, cnt: raw[off:off + 4 * cnt].view(np.float32)
    p = {"magic": int(raw[0:4].view(np.uint32)[0]), "n": int(i32(4, 1)[0]), "dim": int(i32(8, 1)[0]), "stale": int(i32(12, 1)[0]),
         "max_sub": int(i32(16, 1)[0]), "thr": f32(64, 64).reshape(8, 8), "blk_sum": raw[320:320 + 8 * PARTS].view(np.uint64),
         "start": i32(L["start"], BUCKETS + PAD), "scb": f32(L["scb"], n * dim).reshape(n, dim), "sidx": i32(L["sidx"], n)}
    nodes = BUCKETS
    p["boxes"] = []
    for name, fan in L["levels"]:
        nodes = nodes // fan if fan else nodes
        p["boxes"].append(f32(L[name], nodes * 2 * dim).reshape(nodes, 2, dim))
    if kind_of(dim) == "grid":
        p["leaf_start"] = i32(L["leaf_start"], 1024 + PAD)
    return p


def sorted_sidx(p):
    """the original indices, ascending inside every bucket (valid once `start` is known to be monotone from 0 to n)"""
    bucket = np.repeat(np.arange(BUCKETS), np.diff(p["start"][:BUCKETS + 1]))
    return p["sidx"][np.lexsort((p["sidx"], bucket))]


def deterministic_parts(p, dim):
    """{name: bytes} of what two builds of the same codebook must agree on"""
    words = np.array([p["magic"], p["n"], p["dim"], p["stale"], p["max_sub"]], dtype=np.int64)
    out = {"header": words.tobytes() + p["blk_sum"].tobytes() + (p["thr"].tobytes() if kind_of(dim) == "grid" else b""),
           "start": p["start"].tobytes() + (p["leaf_start"].tobytes() if "leaf_start" in p else b""),
           "sidx_sorted": sorted_sidx(p).tobytes()}
    for k, b in enumerate(p["boxes"]):
        out["boxes%d" % k] = b.tobytes()
    return out


def digests(p, dim):
    return {k: hashlib.sha256(v).hexdigest() for k, v in deterministic_parts(p, dim).items()}


def book(kind, n, dim):
    import torch

    g = torch.Generator().manual_seed(3300 + 10 * dim + BOOKS.index(kind) + (n & 1))
    cb = torch.randn(n, dim, generator=g)
    if kind == "clustered":             # 90 % of the codes in a ball of radius 1e-3: empty buckets and one that is overfull
        k = int(0.9 * n)
        d = torch.randn(k, dim, generator=g)
        cb[:k] = 0.3 + 1e-3 * torch.rand(k, 1, generator=g) * d / d.norm(dim=1, keepdim=True)
    return cb.contiguous()


def rows_of(dim):
    import torch

    g = torch.Generator().manual_seed(33 + dim)
    return 0.9 * torch.randn(ROWS, dim, generator=g), torch.rand(ROWS, dim, generator=g) * 0.5 + 0.1


def observe(case):
    """One arg-max call on a fresh workspace, then one on the same workspace with its cache filled with 0xFF: the cache's bytes, the
    workspace header's slice hashes, gqhip_cb_cache_degenerate's answer and the indices, after each.  In a process where the case's
    search applies."""
    import torch

    from pit_hip import _lib

    dim, n, kind = case
    prev = _lib.get_low_dims()
    _lib.set_low_dims("search")
    try:
        assert _lib.lib().gqhip_cb_cache_bytes(n, dim) == layout(n, dim)["total"], case
        cb = book(kind, n, dim).to("cuda:0")
        mu, sd = (t.to("cuda:0") for t in rows_of(dim))
        ws = _lib.Workspace()
        out = {}
        for call in ("first", "rebuilt"):
            if call == "rebuilt":
                ws.cache_buf.fill_(0xFF)
            idx, _ = _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
            torch.cuda.synchronize()
            out[call + "_cache"] = ws.cache_buf.cpu().numpy().copy()
            out[call + "_cbsum"] = ws.buf[WS_CBSUM:WS_CBSUM + 8 * PARTS].cpu().numpy().view(np.uint64).copy()
            out[call + "_degenerate"] = np.int64(_lib.lib().gqhip_cb_cache_degenerate(ws.cache_buf.data_ptr(), n, dim))
            out[call + "_idx"] = idx.cpu().numpy()
        return out
    finally:
        _lib.set_low_dims(prev)


@functools.lru_cache(maxsize=None)
def _dim8_child(tmp):
    """every dim-8 case, observed by one child process under GQHIP_GRID=48"""
    path = os.path.join(tmp, "index_dim8.npz")
    env = dict(os.environ, GQHIP_GRID="48")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], env=env, check=True, timeout=120)
    with np.load(path) as z:
        flat = {k: z[k] for k in z.files}
    return {case: {k.split("__", 1)[1]: v for k, v in flat.items() if k.startswith(case_id(case) + "__")} for case in CASES if case[0] == 8}


def observe_any(case, tmp):
    """observe(), through the child process where this one cannot run the case's search"""
    from pit_hip import _lib

    if case[0] == 8 and not _lib.lib().gqhip_grid_search_applies(case[1], 8):
        return _dim8_child(str(tmp))[case]
    return observe(case)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        flat = {}
        for case in CASES:
            if case[0] == 8:
                flat.update({case_id(case) + "__" + k: v for k, v in observe(case).items()})
        np.savez(sys.argv[2], **flat)
    else:
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            table = {}
            for case in CASES:
                dim, n, _ = case
                table[case_id(case)] = digests(parse(observe_any(case, tmp)["first_cache"], n, dim), dim)
        with open(FIXTURE, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {FIXTURE}: {len(table)} cases")
