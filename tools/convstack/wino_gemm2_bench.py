"""The Winograd GEMMs of the 256- / 512-channel levels alone, at the step's shapes: libgqhip's wino_gemm_f16x2 on the [h | l]
operand vs the library route (ONE hipBLASLt fp16 GEMM over K' = 3 Cin of [h | h | l]); error of both against fp64 on a slice.
--tilings w8,w4 (GQHIP_WGEMM values, "auto" = the default dispatch) times those tilings of the own kernel ALTERNATELY in this one
process, --rounds times each, and prints median / min / max per shape and tiling instead of the comparison with the library."""
import argparse, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd"))
from pit_hip import _lib
ap = argparse.ArgumentParser()
ap.add_argument("--tilings", default="", help="comma-separated GQHIP_WGEMM values (128, w8, w4, auto) to time alternately")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=1000, help="launches per timed window of --tilings (a window of ~0.3 s)")
args = ap.parse_args()
tilings = [t for t in args.tilings.split(",") if t]
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)

def timed(fn, iters=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters

def knob(t):
    if t == "auto": os.environ.pop("GQHIP_WGEMM", None)
    else: os.environ["GQHIP_WGEMM"] = t

L = _lib.lib()
for name, P, tiles, cin, cout in (("dec L1 F4 256->256", 36, 16384, 256, 256), ("dec L2 F4 512->512", 36, 4096, 512, 512),
                                  ("enc L2 F2 512->512", 16, 16384, 512, 512), ("enc L3 F2 512->512", 16, 4096, 512, 512),
                                  ("dec L3 F4 512->512", 36, 1024, 512, 512), ("dec L1 F4 512->256", 36, 16384, 512, 256),
                                  ("enc L2 F2 256->512", 16, 16384, 256, 512)):
    V = torch.randn(P, tiles, cin, generator=g).to(dev)
    U = (torch.randn(P, cin, cout, generator=g) / 11.3).to(dev)
    vh = V.half(); vl = (V - vh.float()).half()
    uh = U.half(); ul = (U - uh.float()).half()
    V2 = torch.cat([vh, vl], 2).contiguous()
    Wf = _lib.wino_weights_operand_order(uh, ul)
    M = torch.empty(P, tiles, cout, device=dev)
    def own():
        _lib._check(L.wino_gemm_f16x2(V2.data_ptr(), Wf.data_ptr(), M.data_ptr(), P, tiles, cin, cout,
                                      torch.cuda.current_stream().cuda_stream), "wg2")
    fl = 6.0 * P * tiles * cin * cout
    gb_own = (V2.numel() * 2 + M.numel() * 4) / 1e9
    if tilings:
        runs, outs = {t: [] for t in tilings}, {}
        for rnd in range(args.rounds + 1):               # round 0 warms clocks and caches up and is dropped
            for t in tilings:
                knob(t)
                us = timed(own, args.iters) * 1e3
                if rnd: runs[t].append(us)
        for t in tilings:
            knob(t); own(); outs[t] = M.clone()
        knob("auto")
        same = all(torch.equal(outs[t], outs[tilings[0]]) for t in tilings)
        for t in tilings:
            r = runs[t]
            print(f"{name:20s} {P:2d} x {tiles:5d} x {cin} -> {cout}  {t:4s} median {statistics.median(r):6.1f} us  min {min(r):6.1f}  max {max(r):6.1f}  "
                  f"({fl/statistics.median(r)/1e6:5.0f} TFLOP/s executed, {gb_own/statistics.median(r)*1e3:4.2f} TB/s; runs {' '.join('%.1f' % x for x in r)}; M bit-equal {same})", flush=True)
        del V, U, V2, M, outs
        continue
    V3 = torch.cat([vh, vh, vl], 2).contiguous(); U3 = torch.cat([uh, ul, uh], 1).contiguous()
    t_own = timed(own); t_lib = timed(lambda: torch.bmm(V3, U3, out_dtype=torch.float32))
    own(); ref = torch.bmm(V3, U3, out_dtype=torch.float32)
    r64 = torch.bmm(V[:1, :512].double(), U[:1].double()); sc = torch.bmm(V[:1, :512].abs().double(), U[:1].abs().double())
    e_own = float(((M[:1, :512].double() - r64).abs() / sc).max()); e_lib = float(((ref[:1, :512].double() - r64).abs() / sc).max())
    gb_lib = (V3.numel() * 2 + M.numel() * 4) / 1e9
    print(f"{name:20s} own {t_own*1e3:6.0f} us = {fl/t_own/1e9:5.0f} TFLOP/s executed, {gb_own/t_own:4.2f} TB/s (err {e_own:.1e}, fits {_lib.own_gemm_fits(P, tiles, cout)}) | "
          f"library {t_lib*1e3:6.0f} us = {fl/t_lib/1e9:5.0f} TFLOP/s, {gb_lib/t_lib:4.2f} TB/s (err {e_lib:.1e}) | {t_lib/t_own:4.2f}x", flush=True)
    del V, U, V2, V3, M, ref
