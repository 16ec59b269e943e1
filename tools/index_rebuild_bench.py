"""What a rebuild of the codebook index costs (csrc/gq_index.h): the durations of the kernels around the search loops -- the code blocks of
gq_prep_kernel / gq_low_hash_kernel and the one-block builders -- when every call has to rebuild, as a VQ training step with a cache does.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/index_rebuild_bench.py --dim 4 --n 65536 [--calls 24]
    python tools/index_rebuild_bench.py --table LABEL=DIR [LABEL=DIR ...]        # several runs per label: median and range of the averages

The run fills the cache with 0xFF before each call (one rebuild per call); no counters in the same run.  GQHIP_LIB selects the build.
The table reads each run's *kernel_stats.csv (Name, Calls, TotalDurationNs, AverageNs, ...), keeps the kernels named in KERNELS and prints,
per label and kernel, the median and the range of the runs' average durations."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vq-vae-from-gaussian-vae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNELS = ("gq_prep_kernel", "gq_low_hash_kernel", "gq_grid_build_kernel", "gq_low_build_kernel")


def run(dim, n, calls, rows):
    import torch

    from pit_hip import _lib

    if dim < 4:
        _lib.set_low_dims("search")
    g = torch.Generator().manual_seed(dim)
    cb = torch.randn(n, dim, generator=g).cuda()
    mu = (0.9 * torch.randn(rows, dim, generator=g)).cuda()
    sd = (torch.rand(rows, dim, generator=g) * 0.5 + 0.1).cuda()
    ws = _lib.Workspace()
    _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
    assert ws.cache_buf is not None, "no codebook cache at this shape"
    for _ in range(calls):
        ws.cache_buf.fill_(0xFF)
        _lib.gq_argmax(mu, sd, cb, 1.0, ws=ws)
    torch.cuda.synchronize()
    print(f"dim {dim} n {n}: {calls} rebuilding calls of {rows} rows")


def averages(directory):
    """{kernel of KERNELS: average duration in us} of one run (instantiations of a kernel: weighted by their calls)"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row["Name"]:
                    calls, total = out.get(k, (0, 0.0))
                    out[k] = (calls + int(row["Calls"]), total + float(row["TotalDurationNs"]))
    return {k: total / calls / 1e3 for k, (calls, total) in out.items()}


def table(pairs):
    runs = {}
    for pair in pairs:
        label, directory = pair.split("=", 1)
        runs.setdefault(label, []).append(averages(directory))
    for label, rs in runs.items():
        for k in KERNELS:
            v = sorted(r[k] for r in rs if k in r)
            if v:
                print(f"{label:28s} {k:22s} median {statistics.median(v):8.2f} us  range {v[0]:8.2f} .. {v[-1]:8.2f}  ({len(v)} runs: "
                      + " ".join(f"{x:.2f}" for x in v) + ")")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=4)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--table", nargs="+")
    a = ap.parse_args()
    table(a.table) if a.table else run(a.dim, a.n, a.calls, a.rows)
