"""ViT backbone goldens (same rules as make_golden*.py: build container only, imports /root/reference, stores DATA).

The reference's pit/modules/vit.py is imported with a script-local stand-in for timm.models.layers (to_2tuple, trunc_normal_,
DropPath -- timm is not installed; the three are restated here exactly as timm defines them).  Tiny encoders / decoders are
built with a seeded init and run on CPU in eval(), then composed with the reference's GaussianQuantRegularizer(format="blc",
backend="torch") as encoder -> regularizer -> decoder (the reference engine itself imports Lightning and cannot be loaded).

  g21_vit_<case>.npz   params (encoder / decoder kwargs as JSON), enc.<key> / dec.<key> (state_dicts), x (input images),
                       z (encoder output), indices, zhat (reference regularizer), gap (the reference's top-2 score gap per
                       quantised row, from the oracle), rec (decoder output on zhat), n_samples.  One layer, mlp_ratio 2,
                       dim_ffn_output 256; every parameter is rounded to an fp16 value after the seeded init and stored as
                       fp16 (exact: the models are fp32, the values just fit in fp16), so that each file stays under 1 MiB.
      d64_tail       width 128, heads 2 (head dim 64), 72 x 72 image, patch 8: 81 tokens (not a multiple of 64), group 16
      block_causal   the same shapes with mask_type "block-causal", mask_block_size 9 (the mask is not all-enabled), group 16
      group4         width 128, heads 2, 64 x 64 image (64 tokens), z_channels 16, group 4 (four codes per token)
  g21_vit_keys.json    the reference's ordered state_dict keys and shapes of the full bsqvit_gq_0.25 encoder and decoder.
  bsqvit_gq_{0.25,0.50,1.00}.yaml   copies of the shipped configs (settings only) for the CPU tests.
"""
import json
import os
import shutil
import sys
import types
from itertools import repeat
import collections.abc

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)


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

from pit.modules.vit import TransformerDecoder as RefDec, TransformerEncoder as RefEnc  # noqa: E402
from pit.quantization.gaussian import GaussianQuantRegularizer as RefGQ  # noqa: E402

from oracle import gq_oracle as O  # noqa: E402

torch.set_grad_enabled(False)
N_SAMPLES = 4096


def case(tag, image, group, mask_type="none", mask_block_size=-1, seed=0):
    params = dict(image_size=image, patch_size=8, width=128, layers=1, heads=2, mlp_ratio=2, double_z=True, z_channels=16,
                  drop_rate=0.0, mask_type=mask_type, mask_block_size=mask_block_size)
    dec_params = dict(params, dim_ffn_output=256)
    torch.manual_seed(seed)
    enc = RefEnc(**params).eval()
    dec = RefDec(**dec_params).eval()
    # non-zero biases / LayerNorm affines, so that every parameter matters
    g = torch.Generator().manual_seed(seed + 100)
    for m in (enc, dec):
        for n, p in m.named_parameters():
            if n.endswith("bias") or ".ln" in n or n.startswith("ln"):
                p.add_(0.02 * torch.randn(p.shape, generator=g))
            p.copy_(p.half().float())   # fp16-representable: stored as fp16 (exact), the file stays under 1 MiB
    x = torch.rand(2, 3, image, image, generator=g) * 2 - 1
    z = enc(x)
    reg = RefGQ("blc", N_SAMPLES, group=group, backend="torch").eval()
    zhat, info = reg(z)
    rec = dec(zhat)
    # the reference's top-2 score gap per quantised row (rows in the order of info["indices"].reshape(-1))
    b, l, c2 = z.shape
    c = c2 // 2
    mu, logvar = z.chunk(2, 2)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    mu_r = mu.reshape(b, l, group, c // group).permute(0, 1, 3, 2).reshape(-1, group).contiguous().numpy()
    sd_r = std.reshape(b, l, group, c // group).permute(0, 1, 3, 2).reshape(-1, group).contiguous().numpy()
    oi, _, best, second = O.argmax_rows(mu_r, sd_r, reg.prior_samples.numpy(), 1.0, with_gap=True)
    ind = info["indices"].numpy()
    assert np.mean(oi != ind.reshape(-1)) < 1e-2, tag
    out = {"params": np.array(json.dumps(dict(enc=params, dec=dec_params))), "x": x.numpy(), "z": z.numpy(),
           "indices": ind.astype(np.int32), "zhat": zhat.numpy(), "gap": (best - second).astype(np.float32),
           "rec": rec.numpy(), "n_samples": np.array(N_SAMPLES)}
    for pre, m in (("enc.", enc), ("dec.", dec)):
        for k, v in m.state_dict().items():
            assert torch.equal(v.half().float(), v)
            out[pre + k] = v.numpy().astype(np.float16)
    np.savez_compressed(os.path.join(HERE, f"g21_vit_{tag}.npz"), **out)
    print(tag, "z", tuple(z.shape), "indices", tuple(ind.shape), "rec", tuple(rec.shape))


case("d64_tail", 72, 16, seed=1)
case("block_causal", 72, 16, mask_type="block-causal", mask_block_size=9, seed=2)
case("group4", 64, 4, seed=3)

# full-size key list of bsqvit_gq_0.25 (encoder_config params; the decoder reuses them, configs/bsqvit_gq_0.25.yaml)
full = dict(double_z=True, z_channels=16, image_size=256, patch_size=8, width=768, layers=12, heads=12, mlp_ratio=4,
            drop_rate=0.0)
keys = {}
for pre, cls in (("encoder", RefEnc), ("decoder", RefDec)):
    m = cls(**full)
    keys[pre] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
with open(os.path.join(HERE, "g21_vit_keys.json"), "w") as f:
    json.dump(keys, f, indent=0)
for g in ("0.25", "0.50", "1.00"):
    shutil.copyfile(os.path.join(REF, "configs", f"bsqvit_gq_{g}.yaml"), os.path.join(HERE, f"bsqvit_gq_{g}.yaml"))
print("keys", {k: len(v) for k, v in keys.items()})
