"""Which kernel serves which layer: the ordered list of library calls one forward of the conv stack makes, per case.

For the duration of a forward every work-doing public function of pit_hip._lib and every library entry point the stack can fall
back to (F.conv2d, F.group_norm, F.interpolate, F.scaled_dot_product_attention, torch.bmm / matmul / addmm) is replaced by a
recorder.  Per call it keeps the name, the shapes of the tensor arguments (those inside the ``gn`` / ``f16`` tuples too), which
optional arguments are None and the int / bool / str arguments -- no floats (bounds and scales follow the weights) and no
pointers.  Arguments are bound to the callee's signature first, so positional / keyword spelling and spelled-out defaults do
not show.  Every case runs twice: the first forward builds the weight caches ("cold"), the second is the steady state
("warm"); the SHA-256 of both outputs is kept so that two trees can be compared bit for bit.

    python tools/convstack/route_trace.py --out DIR       # DIR/route_trace.json (everything), DIR/route_trace.txt (diffable)
    python tools/convstack/route_trace.py --fixture FILE  # the committed summary: tests/golden/convstack_routes.json

The cases (seeds and configs of tests/test_gpu_convstack_routes.py): the TOY encoder / decoder in both layouts with every switch
turned off one at a time; the FULL encoder / decoder, channels_last, at 256 x 256 with batch 1 and 16 and at two sizes no tile
divides; a bare ResnetBlock(128, 256) with a pending bias, in eval mode and with dropout in train mode.
"""
import argparse
import contextlib
import hashlib
import inspect
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pit_hip import _lib  # noqa: E402
from pit_hip.modules import unet as U  # noqa: E402

DEV = "cuda:0"
TOY = dict(attn_type="vanilla", ch=128, out_ch=3, in_channels=3, resolution=64, z_channels=16, double_z=True, ch_mult=[1, 2, 4, 4],
           num_res_blocks=2, attn_resolutions=[8], dropout=0.0)
FULL = dict(attn_type="vanilla", double_z=True, z_channels=16, resolution=256, in_channels=3, out_ch=3, ch=128,
            ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[32], dropout=0.0)
SWITCHES = ["default", "FUSED_GN", "DEFER_BIAS", "WINOGRAD", "FUSED_WINO_TAIL", "WINOGRAD_F4", "WINOGRAD_F16X3", "WINOGRAD_OWN_GEMM",
            "DIRECT_CONV", "DIRECT_CONV_S2", "DIRECT_CONV_1X1", "FUSED_CONV_OUT", "CONV_F32", "FUSED_WINO_GN", "FUSED_WINO_GN_F4",
            "DIRECT_UPCONV", "FUSED_QKV", "FUSED_ADD_STATS", "STATS_ARENA", "CONV_IN_SMALL", "ATTN_F16X3", "ATTN_FUSED_PROJ"]
FULL_SIZES = [(1, 256, 256), (16, 256, 256), (1, 40, 24), (2, 264, 200)]
LISTED = ("full/encoder/cl/16x256x256", "full/decoder/cl/16x256x256")   # cases whose whole call list goes into the fixture

# host-side questions about a shape or the build: they launch nothing, and how often a route asks them is not part of the route
NOT_RECORDED = {"lib", "build", "image_layout", "gn_nhwc_ok", "conv_f32_ok", "conv_cin_small_ok", "own_gemm_fits", "bmm_out_dtype_ok"}
LIBRARY = [(F, "F", n) for n in ("conv2d", "group_norm", "interpolate", "scaled_dot_product_attention")] + \
          [(torch, "torch", n) for n in ("bmm", "matmul", "addmm")]


def _targets():
    own = [(_lib, "_lib", n) for n, f in sorted(vars(_lib).items())
           if inspect.isfunction(f) and f.__module__ == _lib.__name__ and not n.startswith("_") and n not in NOT_RECORDED]
    return own + [(o, p, n) for o, p, n in LIBRARY if hasattr(o, n)]


def _show(v):
    if isinstance(v, torch.Tensor):
        dt = "" if v.dtype == torch.float32 else ":" + str(v.dtype).replace("torch.", "")
        return "T" + "x".join(str(s) for s in v.shape) + dt
    if v is None or isinstance(v, (bool, int, str)):
        return repr(v)
    if isinstance(v, float):
        return "f"
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_show(e) for e in v) + ")"
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    return type(v).__name__


def _recorder(label, fn, trace):
    try:
        sig = inspect.signature(fn)
    except (TypeError, ValueError):      # builtins without a signature: as called
        sig = None

    def recorded(*a, **k):
        if sig is not None:
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            args = [f"{n}={_show(v)}" for n, v in bound.arguments.items()]
        else:
            args = [_show(v) for v in a] + [f"{n}={_show(v)}" for n, v in k.items()]
        trace.append(f"{label}({', '.join(args)})")
        return fn(*a, **k)

    return recorded


@contextlib.contextmanager
def recording(trace):
    """Every target replaced by a recorder that appends to ``trace``; restored on exit."""
    saved = [(o, n, getattr(o, n)) for o, _, n in _targets()]
    try:
        for (o, p, n), (_, _, fn) in zip(_targets(), saved):
            setattr(o, n, _recorder(f"{p}.{n}", fn, trace))
        yield trace
    finally:
        for o, n, fn in saved:
            setattr(o, n, fn)


@contextlib.contextmanager
def switched_off(name):
    if name == "default":
        yield
        return
    old = getattr(U, name)
    setattr(U, name, False)
    try:
        yield
    finally:
        setattr(U, name, old)


def _digest(y):
    return hashlib.sha256(y.detach().float().contiguous().cpu().numpy().tobytes()).hexdigest()


def _run(forward):
    """[(trace, output digest)] of the cold and the warm forward."""
    runs = []
    for _ in range(2):
        with recording([]) as trace, torch.no_grad():
            torch.manual_seed(99)       # (the dropout case draws a mask)
            y = forward()
        torch.cuda.synchronize()
        runs.append((trace, _digest(y)))
    return runs


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def cases():
    """Yields (name, [(trace, digest) cold, (trace, digest) warm])."""
    torch.manual_seed(1234)
    enc, dec = U.Encoder(**TOY).eval().to(DEV), U.Decoder(**TOY).eval().to(DEV)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    zin = torch.randn(2, 16, 8, 8, generator=g).to(DEV)
    for tag, fmt in (("cl", torch.channels_last), ("nchw", torch.contiguous_format)):
        enc, dec = enc.to(memory_format=fmt), dec.to(memory_format=fmt)
        xf, zf = x.contiguous(memory_format=fmt), zin.contiguous(memory_format=fmt)
        for off in SWITCHES:
            with switched_off(off):
                yield f"toy/encoder/{tag}/{off}", _run(lambda: enc(xf))
                yield f"toy/decoder/{tag}/{off}", _run(lambda: dec(zf))
    del enc, dec

    torch.manual_seed(1234)
    enc = U.Encoder(**FULL).eval().to(DEV).to(memory_format=torch.channels_last)
    dec = U.Decoder(**FULL).eval().to(DEV).to(memory_format=torch.channels_last)
    for B, H, W in FULL_SIZES:
        g = torch.Generator().manual_seed(B * 1000 + H + W)
        xf = _cl((torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(DEV))
        zf = _cl(torch.randn(B, 16, H // 8, W // 8, generator=g).to(DEV))
        yield f"full/encoder/cl/{B}x{H}x{W}", _run(lambda: enc(xf))
        yield f"full/decoder/cl/{B}x{H}x{W}", _run(lambda: dec(zf))
    del enc, dec

    torch.manual_seed(7)
    blk = U.ResnetBlock(128, 256, 0.0).eval().to(DEV).to(memory_format=torch.channels_last)
    U.mark_winograd(blk)
    xb = _cl(torch.randn(2, 128, 16, 32, device=DEV))
    pb = torch.randn(128, device=DEV)
    yield "block/128to256/cl/pending_bias", _run(lambda: blk(xb, pb))
    blk.dropout.p = 0.1
    blk.train()
    yield "block/128to256/cl/pending_bias/dropout_train", _run(lambda: blk(xb, pb))


def _sha1(trace):
    return hashlib.sha1("\n".join(trace).encode()).hexdigest()


def _counts(trace):
    out = {}
    for line in trace:
        name = line.split("(", 1)[0]
        out[name] = out.get(name, 0) + 1
    return dict(sorted(out.items()))


def environment():
    return {"torch": torch.__version__, "bmm_out_dtype_ok": bool(_lib.bmm_out_dtype_ok(torch.device(DEV)))}


def summary(results):
    """What the fixture holds: per case the warm forward's {entry: count} and the SHA-1 of its ordered call list (the whole
    list for the cases of LISTED), and the environment the routes were taken under.  No output digests."""
    out = {"environment": environment(), "cases": {}}
    for name, runs in results:
        trace = runs[1][0]
        ent = {"counts": _counts(trace), "sha1": _sha1(trace)}
        if name in LISTED:
            ent["calls"] = trace
        out["cases"][name] = ent
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="DIR", help="write route_trace.json (traces + output digests) and route_trace.txt")
    ap.add_argument("--fixture", metavar="FILE", help="write the committed summary")
    args = ap.parse_args()
    results = list(cases())
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        full = {"environment": environment(),
                "cases": {n: {"cold": r[0][0], "warm": r[1][0], "sha256": [r[0][1], r[1][1]]} for n, r in results}}
        with open(os.path.join(args.out, "route_trace.json"), "w") as f:
            json.dump(full, f, indent=1)
        with open(os.path.join(args.out, "route_trace.txt"), "w") as f:
            for n, r in results:
                for which, (trace, _) in zip(("cold", "warm"), r):
                    f.writelines(f"{n} [{which}] {line}\n" for line in trace)
    if args.fixture:
        with open(args.fixture, "w") as f:
            json.dump(summary(results), f, indent=1)
            f.write("\n")
    s = summary(results)
    print(f"route_trace: {len(results)} cases, {sum(sum(c['counts'].values()) for c in s['cases'].values())} calls in the warm "
          f"forwards, environment {s['environment']}")


if __name__ == "__main__":
    main()
