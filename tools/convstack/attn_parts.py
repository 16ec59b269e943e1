"""Device-event timings of the attention block's projection launches alone, at the step's shape (16 x 32 x 32 x 512): gn_apply, the
q | k | v projection plain / with GroupNorm in its staging / with the split epilogue, attn_split_qkv, proj_out -- each 1x1 launch on
both tilings (GQHIP_CONV1_TILE), three alternating rounds of 200 back-to-back calls.  python tools/convstack/attn_parts.py
(profiles/r13/attn_parts_events.txt)."""
import os, sys, time
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "vq-vae-from-gaussian-vae_amd"))
import torch
from pit_hip import _lib
from pit_hip.modules import unet as U

dev = "cuda:0"
B, C, H, W = 16, 512, 32, 32
torch.manual_seed(0)
cl = lambda t: t.contiguous(memory_format=torch.channels_last)
x = cl(torch.randn(B, C, H, W, device=dev))
norm = torch.nn.GroupNorm(32, C, eps=1e-6).to(dev)
w = torch.randn(3 * C, C, 1, 1, device=dev) * C ** -0.5
bias = torch.randn(3 * C, device=dev)
wf, us = _lib.conv3_weights_f16(w)
pw = torch.randn(C, C, 1, 1, device=dev) * C ** -0.5
pwf, pus = _lib.conv3_weights_f16(pw)
pbias = torch.randn(C, device=dev)
st = _lib.gn_stats(x, 32)
gn = (norm.weight, norm.bias, 32, 1e-6, False, st, None)
bound = U._gn_act_bound(norm, x)
y = _lib.gn_apply(x, norm.weight, norm.bias, 32, 1e-6, False, st)
qkv = _lib.conv1x1_direct(y, wf, us, bound, bias=bias).permute(0, 2, 3, 1).reshape(B, H * W, 3 * C)
ops = _lib.attention_operands(B, H * W, C, dev)
a = cl(torch.randn(B, C, H, W, device=dev))

def split():
    _lib._check(_lib.lib().attn_split_qkv_f16x3(qkv.data_ptr(), ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), B, H * W, C, 64.0, 64.0, _lib._stream()), "s")

cases = {
    "gn_apply": lambda: _lib.gn_apply(x, norm.weight, norm.bias, 32, 1e-6, False, st),
    "qkv_proj": lambda: _lib.conv1x1_direct(y, wf, us, bound, bias=bias),
    "qkv_proj_gn": lambda: _lib.conv1x1_direct(x, wf, us, bound, bias=bias, gn=gn),
    "attn_split_qkv": split,
    "qkv_split": lambda: _lib.qkv_split_direct(y, wf, us, bound, 64.0, 64.0, bias=bias, out=ops),
    "qkv_split_gn": lambda: _lib.qkv_split_direct(x, wf, us, bound, 64.0, 64.0, bias=bias, gn=gn, out=ops),
    "proj_out": lambda: _lib.conv1x1_direct(a, pwf, pus, 4.0, residual=x, bias=pbias, stats_groups=32),
}
tiled = ("qkv_proj", "qkv_proj_gn", "qkv_split", "qkv_split_gn", "proj_out")
N = 200
def timeit(fn):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / N
res = {}
for rep in range(3):
    for name, fn in cases.items():
        for tile in (("256", "128") if name in tiled else (None,)):
            if tile: os.environ["GQHIP_CONV1_TILE"] = tile
            else: os.environ.pop("GQHIP_CONV1_TILE", None)
            res.setdefault((name, tile), []).append(timeit(fn))
print("us per call (3 alternating rounds of %d back-to-back calls, device events; includes launch gaps)" % N)
for (name, tile), v in res.items():
    print("%-16s tile %-4s  %s" % (name, tile or "-", "  ".join("%7.1f" % t for t in v)))
