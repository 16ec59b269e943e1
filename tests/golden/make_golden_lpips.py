"""LPIPS head and loss goldens (same rules as make_golden*.py: build container only, imports /root/reference, stores DATA).

  g30_lpips_head.npz   per case of tests/lpips_ref.py:CASES, with the reference's own normalize_tensor, NetLinLayer.model and
                       spatial_average (a keep mask applied as nn.Dropout applies one: diff * mask * scale) in fp32 and fp64:
                       out [B] of both, grad_f1 of both at lpips_ref.grad_sample's elements (the whole gradient of the table is
                       3.4 MB in fp64), and out_ref_err / grad_ref_err = the fp32 run's error against the fp64 run over ALL finite
                       elements, in lpips_ref's unit.  grad_nan = how many gradient elements the reference leaves NaN (pixels
                       whose f1 is all zero: sqrt's backward at 0).
  g31_lpips_loss.npz   the reference's real LPIPS and GeneralLPIPSWithDiscriminator at B = 2, 32 x 32, eval-mode LPIPS, train-mode
                       loss, weights from lpips_ref.fill_state, a one-conv stand-in decoder whose weight is `last_layer`:
                       optimizer_idx 0 and 1 in fp32 and fp64 -- loss, every log scalar, d_weight, the gradient of the stand-in
                       decoder's input, the gradient of the discriminator's first conv; LPIPS alone: its output and input gradient.
  g31_lpips_keys.json  state_dict key names and shapes of the reference's LPIPS and loss module.

torchvision is not installed: torchvision.models.vgg16 is stood in by a VGG16-shaped `features` stack (its values are replaced by
lpips_ref's weights), and LPIPS.load_from_pretrained (a download) is patched out."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

import lpips_ref as R  # noqa: E402


def _vgg16_stand_in(pretrained=False, **_):
    layers, cin = [], 3
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"):
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    m = nn.Module()
    m.features = nn.Sequential(*layers)
    return m


if "torchvision" not in sys.modules:
    tv, tvm, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.utils")
    tvm.vgg16 = _vgg16_stand_in
    tv.models, tv.utils = tvm, tvu
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.utils": tvu})

from pit.modules.lpips.loss import lpips as ref_lpips  # noqa: E402

ref_lpips.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
from pit.modules.losses.discriminator_loss import GeneralLPIPSWithDiscriminator as RefLoss  # noqa: E402

SEED_LPIPS, SEED_DISC, SEED_IMAGES = R.SEED_LPIPS, R.SEED_DISC, R.SEED_IMAGES


def head(f0, f1, w, keep, g, dtype):
    f0, f1 = torch.from_numpy(f0).to(dtype), torch.from_numpy(f1).to(dtype).requires_grad_()
    lin = ref_lpips.NetLinLayer(f0.shape[1], use_dropout=False).to(dtype)
    lin.model[-1].weight.data.copy_(torch.from_numpy(w).to(dtype).reshape(1, -1, 1, 1))
    diff = (ref_lpips.normalize_tensor(f0) - ref_lpips.normalize_tensor(f1)) ** 2
    if keep is not None:
        diff = diff * (torch.from_numpy(keep).to(dtype) * R.KEEP_SCALE)
    out = ref_lpips.spatial_average(lin.model(diff), keepdim=True).reshape(-1)
    (grad,) = torch.autograd.grad(out, f1, torch.from_numpy(g).to(dtype))
    return out.detach(), grad


def make_head():
    store = {}
    for shape, near, masked in R.CASES:
        cid = R.case_id(shape, near, masked)
        f0, f1, w, keep, g = R.case_inputs(shape, near, masked)
        o32, g32 = head(f0, f1, w, keep, g, torch.float32)
        o64, g64 = head(f0, f1, w, keep, g, torch.float64)
        _, _, uo, ug = R.head_ref(f0, f1, w, keep, R.KEEP_SCALE, g)
        fin = torch.isfinite(g64) & torch.isfinite(g32)
        sel = R.grad_sample(g64.numel())
        store[cid + "/out_f32"], store[cid + "/out_f64"] = o32.numpy(), o64.numpy()
        store[cid + "/grad_f32"], store[cid + "/grad_f64"] = g32.reshape(-1).numpy()[sel], g64.reshape(-1).numpy()[sel]
        store[cid + "/out_ref_err"] = np.float64(R.err_units(o32, o64, uo))
        store[cid + "/grad_ref_err"] = np.float64(R.err_units(g32[fin], g64[fin], ug[fin]))
        store[cid + "/grad_nan"] = np.int64((~torch.isfinite(g64)).sum())
        print(cid, "out err %.2f" % store[cid + "/out_ref_err"], "grad err %.1f" % store[cid + "/grad_ref_err"],
              "nan", int(store[cid + "/grad_nan"]))
    np.savez_compressed(os.path.join(HERE, "g30_lpips_head.npz"), **{k.replace("/", "."): v for k, v in store.items()})


def build_loss(dtype):
    loss = RefLoss(disc_start=0)
    loss.perceptual_loss.load_state_dict(R.fill_state(loss.perceptual_loss.state_dict(), SEED_LPIPS))
    loss.discriminator.load_state_dict(R.fill_state(loss.discriminator.state_dict(), SEED_DISC))
    loss = loss.to(dtype).train()
    loss.perceptual_loss.eval()
    return loss


def make_loss():
    store = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        x, h, wd = (t.to(dtype) for t in R.images(SEED_IMAGES))
        dec = nn.Conv2d(h.shape[1], 3, 3, padding=1, bias=False).to(dtype)
        dec.weight.data.copy_(wd)
        for opt in (0, 1):
            loss = build_loss(dtype)
            hh = h.clone().requires_grad_()
            val, log = loss(x, dec(hh), regularization_log={}, optimizer_idx=opt, global_step=1, last_layer=dec.weight, split="train")
            store[f"opt{opt}.loss_{tag}"] = val.detach().numpy()
            for k, v in log.items():
                store[f"opt{opt}.log.{k.replace('/', '.')}_{tag}"] = v.detach().numpy()
            if opt == 0:
                store[f"opt0.grad_h_{tag}"] = torch.autograd.grad(val, hh)[0].numpy()
            else:
                store[f"opt1.grad_disc0_{tag}"] = torch.autograd.grad(val, loss.discriminator.main[0].weight)[0].numpy()
        lp = build_loss(dtype).perceptual_loss
        hh = h.clone().requires_grad_()
        out = lp(x, dec(hh))
        gvec = torch.tensor([1.0, -0.5], dtype=dtype).reshape(-1, 1, 1, 1)
        store[f"lpips.out_{tag}"] = out.detach().reshape(-1).numpy()
        store[f"lpips.grad_h_{tag}"] = torch.autograd.grad((out * gvec).sum(), hh)[0].numpy()
    np.savez_compressed(os.path.join(HERE, "g31_lpips_loss.npz"), **store)
    loss = build_loss(torch.float32)
    keys = {"lpips": [[k, list(v.shape)] for k, v in loss.perceptual_loss.state_dict().items()],
            "loss": [[k, list(v.shape)] for k, v in loss.state_dict().items()]}
    json.dump(keys, open(os.path.join(HERE, "g31_lpips_keys.json"), "w"), indent=0)


if __name__ == "__main__":
    torch.manual_seed(0)
    make_head()
    make_loss()
    for f in ("g30_lpips_head.npz", "g31_lpips_loss.npz", "g31_lpips_keys.json"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
