"""LPIPS (VGG16) with its five comparison heads on the fused HIP kernels (reference pit/modules/lpips/loss/lpips.py).

The module tree is the reference's, so ``state_dict`` keys are identical: ``scaling_layer.{shift,scale}``, ``net.slice1.0.weight``
.. ``net.slice5.28.bias`` (torchvision's vgg16 ``features`` indices, rebuilt here from plain torch layers: torchvision is not
needed), ``lin0.model.1.weight`` .. ``lin4.model.1.weight`` (``nn.Dropout`` at index 0 with ``use_dropout``).  All frozen.

Nothing is downloaded, ever.  Weights arrive through ``load_state_dict``, an enclosing module's ``load_state_dict`` (the engine's
``init_from_ckpt``: ``loss.perceptual_loss.*``), ``load_from_pretrained`` (local files) or -- tests -- ``pretrained=False``, which
declares the constructor's random weights to be the weights.  Until both parts (``net.*`` and ``lin*``) have arrived ``forward``
raises: a seeded-random perceptual loss must never train silently.

The VGG runs in torch.  Each head -- unit-normalise both feature maps over C, squared difference, the `lin` layer's dropout and
1x1 convolution, spatial mean -- is ONE library call forward (``lpips_head_f32``) and one per wanted gradient backward
(``lpips_head_backward_f32``) when the features are HIP fp32 tensors dense in one of the library's layouts ([B, C, H, W]
contiguous = "bchw", channels_last = "blc" with no copy) and ``_fused.train_fused()`` holds; otherwise, and with
GQHIP_TRAIN_FUSED=0, the reference's op sequence runs.  Where a reconstruction pixel's features are all zero the fused gradient is
the limit (finite), torch's is NaN (csrc/lpips_head.h).

Dropout: the reference builds ``LPIPS().eval()`` and nothing stops a later ``model.train()`` from switching the `lin` dropouts
back on; that quirk is kept.  A level whose ``nn.Dropout`` is in training mode draws its keep mask with torch (uint8,
``bernoulli_(1 - p)``), hands it to the kernel with ``keep_scale = 1 / (1 - p)`` and saves it for the backward."""
from __future__ import annotations

import os
from collections import namedtuple

import torch
import torch.nn as nn

from .... import _lib
from ....quantization._fused import train_fused

VggOutputs = namedtuple("VggOutputs", ["relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3"])
# torchvision vgg16().features[0 .. 29]: channel counts, "M" = 2x2 max pool; each conv is followed by a ReLU
_VGG16 = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))


def _vgg16_features():
    layers, cin = [], 3
    for v in _VGG16:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return layers


class vgg16(nn.Module):
    """The five slices of VGG16's feature stack, under torchvision's layer indices."""

    def __init__(self, requires_grad: bool = False, pretrained: bool = True):
        super().__init__()
        feats = _vgg16_features()
        self.N_slices = len(_SLICES)
        for k, (lo, hi) in enumerate(_SLICES, start=1):
            seq = nn.Sequential()
            for i in range(lo, hi):
                seq.add_module(str(i), feats[i])
            setattr(self, f"slice{k}", seq)
        if not requires_grad:
            for prm in self.parameters():
                prm.requires_grad = False

    def forward(self, X):
        outs, h = [], X
        for k in range(1, self.N_slices + 1):
            h = getattr(self, f"slice{k}")(h)
            outs.append(h)
        return VggOutputs(*outs)


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-0.030, -0.088, -0.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([0.458, 0.448, 0.450])[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


class NetLinLayer(nn.Module):
    """(dropout,) 1x1 convolution to ``chn_out`` channels, no bias"""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers.append(nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False))
        self.model = nn.Sequential(*layers)


def normalize_tensor(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def spatial_average(x, keepdim=True):
    return x.mean([2, 3], keepdim=keepdim)


def _library_view(f):
    """(f as the library reads it, layout) for a dense [B, C, H, W] tensor, or (None, None)"""
    if f.is_contiguous():
        return f.reshape(f.shape[0], f.shape[1], -1), "bchw"
    if f.is_contiguous(memory_format=torch.channels_last):
        return f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, f.shape[1]), "blc"
    return None, None


class LpipsHeadFn(torch.autograd.Function):
    """One level's comparison head: one forward library call, one backward call per feature map that wants a gradient.  Re-entrant:
    the backward keeps only the saved tensors and frees nothing (calculate_adaptive_weight differentiates the graph before the
    real backward).  ``f0``, ``f1``, ``keep`` are in the library layout ``cfg[0]``."""

    @staticmethod
    def forward(ctx, f0, f1, w, keep, cfg):
        layout, keep_scale, ws = cfg
        out = _lib.lpips_head(f0, f1, w, layout, keep, keep_scale, ws)
        ctx.cfg = cfg
        ctx.save_for_backward(f0, f1, w, keep)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        f0, f1, w, keep = ctx.saved_tensors
        layout, keep_scale, _ = ctx.cfg
        g = g.contiguous()
        g0 = _lib.lpips_head_backward(f1, f0, w, g, layout, keep, keep_scale) if ctx.needs_input_grad[0] else None
        g1 = _lib.lpips_head_backward(f0, f1, w, g, layout, keep, keep_scale) if ctx.needs_input_grad[1] else None
        return g0, g1, None, None, None


class LPIPS(nn.Module):
    def __init__(self, use_dropout: bool = True, pretrained: bool = True):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = [64, 128, 256, 512, 512]
        self.net = vgg16(pretrained=pretrained, requires_grad=False)
        for k, c in enumerate(self.chns):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        for prm in self.parameters():
            prm.requires_grad = False
        self._have = {"net": not pretrained, "lin": not pretrained}    # which parts' weights have arrived
        self._ws = _lib.LpipsHeadWorkspace()

    # ---- weights -----------------------------------------------------------------------------------------------------------------
    @property
    def weights_loaded(self) -> bool:
        return all(self._have.values())

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # runs for this module under its own and under any enclosing module's load_state_dict: a part has arrived when the
        # dictionary holds every one of its keys
        own = list(self.state_dict().keys())
        for part in self._have:
            keys = [k for k in own if k.startswith(part)]
            if keys and all(prefix + k in state_dict for k in keys):
                self._have[part] = True
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def load_from_pretrained(self, lin_path: str, vgg_path: str = None):
        """Local files only.  ``lin_path``: the reference's ``vgg.pth`` (the ``lin*`` weights); ``vgg_path``: a torchvision
        ``vgg16`` state_dict, whose ``features.N.*`` become ``net.sliceK.N.*``.  Without ``vgg_path`` the ``net.*`` weights still
        have to arrive some other way before ``forward`` runs."""
        for path in (lin_path, vgg_path):
            if path is not None and not os.path.isfile(path):
                raise FileNotFoundError(f"LPIPS weights not found at {path} (nothing is downloaded)")
        sd = dict(torch.load(lin_path, map_location="cpu"))
        if vgg_path is not None:
            for k, v in torch.load(vgg_path, map_location="cpu").items():
                if k.startswith("features."):
                    n = int(k.split(".")[1])
                    slice_no = next(i for i, (lo, hi) in enumerate(_SLICES, start=1) if lo <= n < hi)
                    sd[f"net.slice{slice_no}.{k[len('features.'):]}"] = v
        return self.load_state_dict(sd, strict=False)

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def _head(self, f0, f1, lin):
        conv = lin.model[-1]
        if f0.is_cuda and f0.dtype == f1.dtype == torch.float32 and conv.out_channels == 1 and f0.shape[1] <= 512 and train_fused():
            (v0, l0), (v1, l1) = _library_view(f0), _library_view(f1)
            if l0 is not None and l0 == l1:
                drop = lin.model[0] if len(lin.model) > 1 else None
                keep, keep_scale = None, 1.0
                if drop is not None and drop.training and drop.p > 0:
                    keep = torch.empty(v0.shape, dtype=torch.uint8, device=v0.device).bernoulli_(1 - drop.p)
                    keep_scale = 1.0 / (1.0 - drop.p)
                out = LpipsHeadFn.apply(v0, v1, conv.weight.reshape(-1), keep, (l0, keep_scale, self._ws))
                return out.reshape(-1, 1, 1, 1)
        return spatial_average(lin.model((normalize_tensor(f0) - normalize_tensor(f1)) ** 2), keepdim=True)

    def forward(self, input, target):
        if not self.weights_loaded:
            missing = ", ".join(f"{k}.*" for k, v in self._have.items() if not v)
            raise RuntimeError(f"LPIPS has no weights for {missing}: load a checkpoint that carries them (load_state_dict, "
                               "load_from_pretrained, the engine's init_from_ckpt), or construct with pretrained=False to use "
                               "the random ones on purpose")
        outs0, outs1 = self.net(self.scaling_layer(input)), self.net(self.scaling_layer(target))
        val = None
        for kk in range(len(self.chns)):
            res = self._head(outs0[kk], outs1[kk], getattr(self, f"lin{kk}"))
            val = res if val is None else val + res
        return val
