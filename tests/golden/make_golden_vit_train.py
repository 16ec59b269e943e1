"""ViT training-gradient golden (same rules as make_golden_vit.py: build container only, imports /root/reference, stores DATA).

The reference's pit/modules/vit.py is imported with the same script-local stand-in for timm.models.layers as make_golden_vit.py.
The weights and the input of g21_vit_d64_tail.npz (fp16-exact, stored there) are loaded into the REFERENCE's TransformerEncoder
in train() mode; loss = (enc(x) * w).sum() with a seeded w; autograd gives the gradients.

  g23_vit_train_grads.npz   w [2, 81, 32] fp32,
                            g32.<name>  the reference's fp32 gradients,
                            g64.<name>  the same from the reference module in fp64 (weights, x and w cast up),
                            for <name> in transformer.resblocks.0.attn.in_proj_weight, ...in_proj_bias,
                            transformer.resblocks.0.ln_1.weight, positional_embedding.
"""
import collections.abc
import json
import os
import sys
import types
from itertools import repeat

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)


# ---- stand-in for timm.models.layers (timm's definitions) ----
def _to_2tuple(x):
    if isinstance(x, collections.abc.Iterable) and not isinstance(x, str):
        return tuple(x)
    return tuple(repeat(x, 2))


def _trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


class _DropPath(nn.Module):
    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        r = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        return x * (r.div_(keep) if keep > 0.0 and self.scale_by_keep else r)


_layers = types.ModuleType("timm.models.layers")
_layers.to_2tuple, _layers.trunc_normal_, _layers.DropPath = _to_2tuple, _trunc_normal_, _DropPath
sys.modules.setdefault("timm", types.ModuleType("timm"))
sys.modules.setdefault("timm.models", types.ModuleType("timm.models"))
sys.modules["timm.models.layers"] = _layers

from pit.modules.vit import TransformerEncoder as RefEnc  # noqa: E402

NAMES = ("transformer.resblocks.0.attn.in_proj_weight", "transformer.resblocks.0.attn.in_proj_bias",
         "transformer.resblocks.0.ln_1.weight", "positional_embedding")

d = np.load(os.path.join(HERE, "g21_vit_d64_tail.npz"))
params = json.loads(str(d["params"]))["enc"]
sd = {k[4:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("enc.")}
x = torch.from_numpy(d["x"])
w = torch.randn(d["z"].shape, generator=torch.Generator().manual_seed(23))

out = {"w": w.numpy()}
for tag, dt in (("g32", torch.float32), ("g64", torch.float64)):
    enc = RefEnc(**params)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dt).train()
    loss = (enc(x.to(dt)) * w.to(dt)).sum()
    loss.backward()
    named = dict(enc.named_parameters())
    for n in NAMES:
        out[f"{tag}.{n}"] = named[n].grad.numpy().copy()
    print(tag, float(loss), {n.split(".")[-1]: float(named[n].grad.abs().max()) for n in NAMES})
path = os.path.join(HERE, "g23_vit_train_grads.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
