"""BSQ-ViT encoder / decoder as ``torch.nn`` modules with libgqhip's fused attention on the hot path.

Port of the reference's ``pit/modules/vit.py`` (bsq-vit's transcoder/models/transformer.py and attention_mask.py, MIT
License, Copyright (c) 2024 Yue Zhao): the same classes, constructor keywords, defaults and module tree, so that
``state_dict()`` keys and shapes equal the reference's (``transformer.resblocks.{i}.attn.in_proj_weight``, ``mlp.c_fc``,
``conv1``, ``quant_embed``, ``post_quant_embed``, ``ffn.0``, ``conv_out`` ...) and a reference checkpoint loads unchanged.
``nn.MultiheadAttention`` stays the parameter container.  timm's ``to_2tuple``, ``trunc_normal_`` and ``DropPath`` are
restated locally; einops' patterns are spelled as the reshape / permute / reshape they expand to.

Two routes through every attention layer:
- the HIP route: CUDA fp32 input, grad disabled (or ``HIP_ATTN_TRAIN`` on, see below), ``mask_type`` "none", a head dim libgqhip is built for (64), no attention
  dropout or drop path in training.  The tokens stay batch-first [B, L, E]: ``F.linear(ln_1(x), in_proj_weight,
  in_proj_bias)`` -> ``_lib.mha_fwd`` (one fused kernel, S never written) -> ``out_proj``.  LayerNorm, the MLP, GELU and the
  residual adds stay ATen ops.
- otherwise (CPU, autograd, masks, other head dims, ``HIP_ATTN = False``) the reference's exact op sequence: permute to
  seq-first, ``self.attn(x, x, x, need_weights=False)``, permute back -- bit-identical to the reference on CPU.

Training on the HIP route is opt-in (``HIP_ATTN_TRAIN = True`` or ``GQHIP_ATTN_TRAIN=1`` in the environment at import): with grad
enabled the attention core then is ``_MhaFn`` -- ``_lib.mha_fwd_lse`` forward (the same ``out`` bits, plus the row log-sum-exp),
``_lib.mha_bwd`` backward (csrc/gq_attn_bwd.h) -- and everything around it stays autograd's.  Off (the default), every grad-enabled
call takes torch's route exactly as before.
"""
from __future__ import annotations

import collections.abc
import os
from collections import OrderedDict
from itertools import repeat
from typing import Callable, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

HIP_ATTN = True   # route unmasked fp32 inference attention through libgqhip's fused kernel (False: torch's MHA everywhere)
HIP_ATTN_TRAIN = os.environ.get("GQHIP_ATTN_TRAIN", "") == "1"   # also with grad enabled (fused forward + backward); default off


# ---- timm.models.layers, restated ---------------------------------------------------------------------------------------------
def to_2tuple(x):
    if isinstance(x, collections.abc.Iterable) and not isinstance(x, str):
        return tuple(x)
    return tuple(repeat(x, 2))


def trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):
    # timm's default bounds are absolute (+-2), as torch's
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


def drop_path(x, drop_prob: float = 0.0, training: bool = False, scale_by_keep: bool = True):
    if drop_prob == 0.0 or not training:
        return x
    keep_prob = 1 - drop_prob
    shape = (x.shape[0],) + (1,) * (x.ndim - 1)
    random_tensor = x.new_empty(shape).bernoulli_(keep_prob)
    if keep_prob > 0.0 and scale_by_keep:
        random_tensor.div_(keep_prob)
    return x * random_tensor


class DropPath(nn.Module):
    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x):
        return drop_path(x, self.drop_prob, self.training, self.scale_by_keep)


# ---- attention masks (vit.py:38-80) ---------------------------------------------------------------------------------------------
def get_attention_mask(sequence_length, device, mask_type="block-causal", **kwargs):
    if mask_type.lower() == "none" or mask_type is None:
        return None
    elif mask_type.lower() == "block-causal":
        return _block_caulsal_mask_impl(sequence_length, device, **kwargs)
    elif mask_type.lower() == "causal":
        return _caulsal_mask_impl(sequence_length, device, **kwargs)
    else:
        raise NotImplementedError(f"Mask type {mask_type} not implemented")


def _block_caulsal_mask_impl(sequence_length, device, block_size=16, **kwargs):
    """Block-causal mask (True = disabled)."""
    assert sequence_length % block_size == 0, "for block causal masks sequence length must be divisible by block size"
    blocks = torch.ones(sequence_length // block_size, block_size, block_size, device=device)
    block_diag_enable_mask = torch.block_diag(*blocks)
    causal_enable_mask = torch.ones(sequence_length, sequence_length, device=device).tril_(0)
    disable_mask = (block_diag_enable_mask + causal_enable_mask) < 0.5
    return disable_mask


def _caulsal_mask_impl(sequence_length, device, **kwargs):
    """Causal mask (-inf above the diagonal)."""
    return torch.triu(torch.full((sequence_length, sequence_length), float("-inf"), dtype=torch.float32, device=device),
                      diagonal=1)


def _hip_route(x: torch.Tensor, transformer: "Transformer", mask_type) -> bool:
    """The fused HIP attention applies to every block of ``transformer`` for input ``x`` (see the module docstring)."""
    if not (HIP_ATTN and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
        return False
    if torch.is_grad_enabled():
        if not HIP_ATTN_TRAIN:
            return False
        if transformer.training and transformer.grad_checkpointing and transformer.selective_checkpointing:
            return False    # selective checkpointing stays on torch's route
    if not (mask_type is None or str(mask_type).lower() == "none") or len(transformer.resblocks) == 0:
        return False
    from .. import _lib

    for r in transformer.resblocks:
        a = r.attn
        if a.embed_dim % a.num_heads != 0 or a.embed_dim // a.num_heads not in _lib.MHA_HEAD_DIMS or a.in_proj_weight is None:
            return False
        if r.training and (a.dropout > 0.0 or isinstance(r.drop_path, DropPath) and r.drop_path.drop_prob > 0.0):
            return False
    return True


class _MhaFn(torch.autograd.Function):
    """The attention core on libgqhip under autograd: qkv [B, L, 3E] -> out [B, L, E]; the backward recomputes P from lse."""

    @staticmethod
    def forward(ctx, qkv, heads):
        from .. import _lib

        out, lse = _lib.mha_fwd_lse(qkv, heads)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _lib

        qkv, out, lse = ctx.saved_tensors
        return _lib.mha_bwd(qkv, out, lse, dout, ctx.heads), None


# ---- blocks (vit.py:83-279) -----------------------------------------------------------------------------------------------------
class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5, inplace=False):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x.mul_(self.gamma) if self.inplace else x * self.gamma


class ResidualAttentionBlock(nn.Module):
    def __init__(
        self,
        d_model: int,
        n_head: int,
        mlp_ratio: float = 4.0,
        ls_init_value: float = None,
        drop: float = 0.0,
        attn_drop: float = 0.0,
        drop_path: float = 0.0,
        act_layer: Callable = nn.GELU,
        norm_layer: Callable = nn.LayerNorm,
        use_preln: bool = True,
    ):
        super().__init__()

        self.ln_1 = norm_layer(d_model)
        self.attn = nn.MultiheadAttention(d_model, n_head, dropout=attn_drop)
        self.ls_1 = LayerScale(d_model, ls_init_value) if ls_init_value is not None else nn.Identity()

        self.ln_2 = norm_layer(d_model)
        mlp_width = int(d_model * mlp_ratio)
        self.mlp = nn.Sequential(
            OrderedDict(
                [
                    ("c_fc", nn.Linear(d_model, mlp_width)),
                    ("gelu", act_layer()),
                    ("c_proj", nn.Linear(mlp_width, d_model)),
                    ("drop2", nn.Dropout(drop)),
                ]
            )
        )
        self.ls_2 = LayerScale(d_model, ls_init_value) if ls_init_value is not None else nn.Identity()

        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

        self.use_preln = use_preln

    def attention(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False):
        attn_mask = attn_mask.to(x.dtype) if attn_mask is not None else None
        return self.attn(x, x, x, need_weights=False, attn_mask=attn_mask, is_causal=is_causal)[0]

    def attention_hip(self, x: torch.Tensor) -> torch.Tensor:
        """Unmasked self-attention of batch-first x [B, L, E] through libgqhip (the HIP route)."""
        from .. import _lib

        a = self.attn
        qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)
        if torch.is_grad_enabled() and qkv.requires_grad:
            o = _MhaFn.apply(qkv, a.num_heads)
        else:
            o = _lib.mha_fwd(qkv, a.num_heads)
        return F.linear(o, a.out_proj.weight, a.out_proj.bias)

    def checkpoint_forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False):
        state = x
        if self.use_preln:
            x = checkpoint(self.ln_1, x, use_reentrant=False)
            x = self.attention(x, attn_mask, is_causal)
            x = checkpoint(self.ls_1, x, use_reentrant=False)
            state = state + self.drop_path(x)
            x = checkpoint(self.ln_2, state, use_reentrant=False)
            x = self.mlp(x)
            x = checkpoint(self.ls_2, x, use_reentrant=False)
            state = state + self.drop_path(x)
        else:
            x = self.attention(x, attn_mask, is_causal)
            x = state + self.drop_path(x)
            state = checkpoint(self.ln_1, x, use_reentrant=False)
            x = self.mlp(state)
            state = state + self.drop_path(x)
            state = checkpoint(self.ln_2, state, use_reentrant=False)
        return state

    def forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False,
                selective_checkpointing: bool = False):
        if selective_checkpointing:
            return self.checkpoint_forward(x, attn_mask, is_causal=is_causal)
        if self.use_preln:
            x = x + self.drop_path(self.ls_1(self.attention(self.ln_1(x), attn_mask=attn_mask, is_causal=is_causal)))
            x = x + self.drop_path(self.ls_2(self.mlp(self.ln_2(x))))
        else:
            x = x + self.drop_path(self.attention(x, attn_mask=attn_mask, is_causal=is_causal))
            x = self.ln_1(x)
            x = x + self.drop_path(self.mlp(x))
            x = self.ln_2(x)
        return x

    def forward_hip(self, x: torch.Tensor) -> torch.Tensor:
        """forward() without a mask on batch-first x [B, L, E], attention through libgqhip."""
        if self.use_preln:
            x = x + self.drop_path(self.ls_1(self.attention_hip(self.ln_1(x))))
            x = x + self.drop_path(self.ls_2(self.mlp(self.ln_2(x))))
        else:
            x = x + self.drop_path(self.attention_hip(x))
            x = self.ln_1(x)
            x = x + self.drop_path(self.mlp(x))
            x = self.ln_2(x)
        return x


class Transformer(nn.Module):
    def __init__(
        self,
        width: int,
        layers: int,
        heads: int,
        mlp_ratio: float = 4.0,
        ls_init_value: float = None,
        drop: float = 0.0,
        attn_drop: float = 0.0,
        drop_path: float = 0.0,
        act_layer: nn.Module = nn.GELU,
        norm_layer: nn.Module = nn.LayerNorm,
        use_preln: bool = True,
    ):
        super().__init__()
        self.width = width
        self.layers = layers
        self.grad_checkpointing = False
        self.selective_checkpointing = False
        self.grad_checkpointing_params = {"use_reentrant": False}
        if attn_drop == 0 and drop_path == 0 and drop_path == 0:
            self.grad_checkpointing_params.update({"preserve_rng_state": False})
        else:
            self.grad_checkpointing_params.update({"preserve_rng_state": True})

        self.resblocks = nn.ModuleList(
            [
                ResidualAttentionBlock(
                    width,
                    heads,
                    mlp_ratio,
                    ls_init_value=ls_init_value,
                    drop=drop,
                    attn_drop=attn_drop,
                    drop_path=drop_path,
                    act_layer=act_layer,
                    norm_layer=norm_layer,
                    use_preln=use_preln,
                )
                for _ in range(layers)
            ]
        )

    def forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False):
        for r in self.resblocks:
            if self.training and self.grad_checkpointing and not torch.jit.is_scripting():
                if not self.selective_checkpointing:
                    x = checkpoint(r, x, attn_mask, is_causal=is_causal, **self.grad_checkpointing_params)
                else:
                    x = r(x, attn_mask=attn_mask, is_causal=is_causal, selective_checkpointing=True)
            else:
                x = r(x, attn_mask=attn_mask)
        return x

    def forward_hip(self, x: torch.Tensor) -> torch.Tensor:
        """Unmasked forward of batch-first x [B, L, E] (the HIP route), whole-block checkpointing as in forward()."""
        for r in self.resblocks:
            if self.training and self.grad_checkpointing and torch.is_grad_enabled():
                x = checkpoint(r.forward_hip, x, **self.grad_checkpointing_params)
            else:
                x = r.forward_hip(x)
        return x


def _run_transformer(transformer: Transformer, x: torch.Tensor, mask_type, mask_block_size: int, grid_size) -> torch.Tensor:
    """vit.py:431-441 / :598-608 on batch-first tokens x [B, L, E]: the HIP route when it applies, else the reference's ops."""
    if _hip_route(x, transformer, mask_type):
        return transformer.forward_hip(x)
    x = x.permute(1, 0, 2)
    block_size = grid_size[0] * grid_size[1] if mask_block_size <= 0 else mask_block_size
    attn_mask = get_attention_mask(x.size(0), x.device, mask_type=mask_type, block_size=block_size)
    x = transformer(x, attn_mask, is_causal=mask_type == "causal")
    return x.permute(1, 0, 2)


def _patchify(x: torch.Tensor, sh: int, sw: int) -> torch.Tensor:
    # rearrange "b c (hh sh) (ww sw) -> b (hh ww) (c sh sw)"
    b, c, H, W = x.shape
    x = x.reshape(b, c, H // sh, sh, W // sw, sw).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(b, (H // sh) * (W // sw), c * sh * sw)


def _patchify_video(x: torch.Tensor, sh: int, sw: int, frames_in_batch: bool) -> torch.Tensor:
    # rearrange "b c t (hh sh) (ww sw) -> b (t hh ww) (c sh sw)"  /  "-> (b t) (hh ww) (c sh sw)"
    b, c, t, H, W = x.shape
    hh, ww = H // sh, W // sw
    x = x.reshape(b, c, t, hh, sh, ww, sw).permute(0, 2, 3, 5, 1, 4, 6)
    if frames_in_batch:
        return x.reshape(b * t, hh * ww, c * sh * sw)
    return x.reshape(b, t * hh * ww, c * sh * sw)


class TransformerEncoder(nn.Module):
    def __init__(
        self,
        image_size: int,
        patch_size: int,
        width: int,
        layers: int,
        heads: int,
        mlp_ratio: float,
        double_z: bool,
        z_channels: int,
        num_frames: int = 1,
        cross_frames: bool = True,
        ls_init_value: float = None,
        drop_rate: float = 0.0,
        attn_drop_rate: float = 0.0,
        drop_path_rate: float = 0.0,
        ln_pre: bool = True,
        ln_post: bool = True,
        act_layer: str = "gelu",
        norm_layer: str = "layer_norm",
        mask_type: Union[str, None] = "none",
        mask_block_size: int = -1,
    ):
        super().__init__()
        self.image_size = to_2tuple(image_size)
        self.patch_size = to_2tuple(patch_size)
        self.grid_size = (self.image_size[0] // self.patch_size[0], self.image_size[1] // self.patch_size[1])
        self.patches_per_frame = self.grid_size[0] * self.grid_size[1]
        self.mask_type = mask_type
        self.mask_block_size = mask_block_size

        if act_layer.lower() == "gelu":
            self.act_layer = nn.GELU
        else:
            raise ValueError(f"Unsupported activation function: {act_layer}")
        if norm_layer.lower() == "layer_norm":
            self.norm_layer = nn.LayerNorm
        else:
            raise ValueError(f"Unsupported normalization: {norm_layer}")

        self.conv1 = nn.Linear(in_features=3 * self.patch_size[0] * self.patch_size[1], out_features=width, bias=not ln_pre)

        scale = width**-0.5
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid_size[0] * self.grid_size[1], width))
        assert num_frames >= 1
        self.num_frames = num_frames
        self.cross_frames = cross_frames
        if num_frames > 1 and cross_frames:
            self.temporal_positional_embedding = nn.Parameter(torch.zeros(num_frames, width))
        else:
            self.temporal_positional_embedding = None

        self.ln_pre = self.norm_layer(width) if ln_pre else nn.Identity()

        self.transformer = Transformer(
            width,
            layers,
            heads,
            mlp_ratio,
            ls_init_value=ls_init_value,
            drop=drop_rate,
            attn_drop=attn_drop_rate,
            drop_path=drop_path_rate,
            act_layer=self.act_layer,
            norm_layer=self.norm_layer,
        )

        self.ln_post = self.norm_layer(width)

        if double_z:
            self.quant_embed = nn.Linear(in_features=width, out_features=z_channels * 2)
        else:
            self.quant_embed = nn.Linear(in_features=width, out_features=z_channels)
        self.init_parameters()

    def init_parameters(self):
        if self.positional_embedding is not None:
            nn.init.normal_(self.positional_embedding, std=0.02)
        trunc_normal_(self.conv1.weight, std=0.02)
        for block in self.transformer.resblocks:
            for n, p in block.named_parameters():
                if "weight" in n:
                    if "ln" not in n:
                        trunc_normal_(p, std=0.02)
                elif "bias" in n:
                    nn.init.zeros_(p)
                else:
                    raise NotImplementedError(f"Unknown parameters named {n}")

    @torch.jit.ignore
    def set_grad_checkpointing(self, enable=True, selective=False):
        self.transformer.grad_checkpointing = enable
        self.transformer.selective_checkpointing = selective

    def forward(self, x):
        if self.num_frames == 1:
            x = _patchify(x, self.patch_size[0], self.patch_size[1])
            x = self.conv1(x)
            x = x + self.positional_embedding.to(x.dtype)
        elif self.cross_frames:
            num_frames = x.shape[2]
            assert num_frames <= self.num_frames, "Number of frames should be less or equal to the model setting"
            x = _patchify_video(x, self.patch_size[0], self.patch_size[1], frames_in_batch=False)
            x = self.conv1(x)
            tile_pos_embed = self.positional_embedding.repeat(num_frames, 1)
            tile_tem_embed = self.temporal_positional_embedding[:num_frames].repeat_interleave(self.patches_per_frame, 0)
            total_pos_embed = tile_pos_embed + tile_tem_embed
            x = x + total_pos_embed.to(x.dtype).squeeze(0)
        else:
            x = _patchify_video(x, self.patch_size[0], self.patch_size[1], frames_in_batch=True)
            x = self.conv1(x)
            x = x + self.positional_embedding.to(x.dtype)

        x = self.ln_pre(x)
        x = _run_transformer(self.transformer, x, self.mask_type, self.mask_block_size, self.grid_size)
        x = self.ln_post(x)
        x = self.quant_embed(x)

        return x


class TransformerDecoder(nn.Module):
    def __init__(
        self,
        image_size: int,
        patch_size: int,
        width: int,
        layers: int,
        heads: int,
        mlp_ratio: float,
        double_z: bool,
        z_channels: int,
        num_frames: int = 1,
        cross_frames: bool = True,
        ls_init_value: float = None,
        drop_rate: float = 0.0,
        attn_drop_rate: float = 0.0,
        drop_path_rate: float = 0.0,
        ln_pre: bool = True,
        ln_post: bool = True,
        act_layer: str = "gelu",
        norm_layer: str = "layer_norm",
        use_ffn_output: bool = True,
        dim_ffn_output: int = 3072,
        logit_laplace: bool = False,
        mask_type: Union[str, None] = "none",
        mask_block_size: int = -1,
    ):
        super().__init__()
        self.image_size = to_2tuple(image_size)
        self.patch_size = to_2tuple(patch_size)
        self.grid_size = (self.image_size[0] // self.patch_size[0], self.image_size[1] // self.patch_size[1])
        self.patches_per_frame = self.grid_size[0] * self.grid_size[1]
        self.mask_type = mask_type
        self.mask_block_size = mask_block_size

        if act_layer.lower() == "gelu":
            self.act_layer = nn.GELU
        else:
            raise ValueError(f"Unsupported activation function: {act_layer}")
        if norm_layer.lower() == "layer_norm":
            self.norm_layer = nn.LayerNorm
        else:
            raise ValueError(f"Unsupported normalization: {norm_layer}")

        self.use_ffn_output = use_ffn_output
        out_features = 3 * self.patch_size[0] * self.patch_size[1] * (1 + logit_laplace)
        if use_ffn_output:
            self.ffn = nn.Sequential(nn.Linear(width, dim_ffn_output), nn.Tanh())
            self.conv_out = nn.Linear(in_features=dim_ffn_output, out_features=out_features)
        else:
            self.ffn = nn.Identity()
            self.conv_out = nn.Linear(in_features=width, out_features=out_features)

        scale = width**-0.5
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid_size[0] * self.grid_size[1], width))
        assert num_frames >= 1
        self.num_frames = num_frames
        self.cross_frames = cross_frames
        if num_frames > 1 and cross_frames:
            self.temporal_positional_embedding = nn.Parameter(torch.zeros(num_frames, width))
        else:
            self.temporal_positional_embedding = None

        self.ln_pre = self.norm_layer(width) if ln_pre else nn.Identity()

        self.transformer = Transformer(
            width,
            layers,
            heads,
            mlp_ratio,
            ls_init_value=ls_init_value,
            drop=drop_rate,
            attn_drop=attn_drop_rate,
            drop_path=drop_path_rate,
            act_layer=self.act_layer,
            norm_layer=self.norm_layer,
        )

        self.ln_post = self.norm_layer(width) if ln_post else nn.Identity()

        self.post_quant_embed = nn.Linear(in_features=z_channels, out_features=width)

        self.init_parameters()

    def init_parameters(self):
        if self.positional_embedding is not None:
            nn.init.normal_(self.positional_embedding, std=0.02)

        for block in self.transformer.resblocks:
            for n, p in block.named_parameters():
                if "weight" in n:
                    if "ln" not in n:
                        trunc_normal_(p, std=0.02)
                elif "bias" in n:
                    nn.init.zeros_(p)
                else:
                    raise NotImplementedError(f"Unknown parameters named {n}")
        if self.use_ffn_output:
            trunc_normal_(self.ffn[0].weight, std=0.02)
        trunc_normal_(self.conv_out.weight, std=0.02)

    def get_last_layer(self, **kwargs):
        return self.conv_out.weight

    @torch.jit.ignore
    def set_grad_checkpointing(self, enable=True, selective=False):
        self.transformer.grad_checkpointing = enable
        self.transformer.selective_checkpointing = selective

    def forward(self, x):
        x = self.post_quant_embed(x)

        num_frames = self.num_frames
        if self.num_frames == 1 or not self.cross_frames:
            x = x + self.positional_embedding.to(x.dtype)
        else:
            num_frames = x.shape[1] // self.patches_per_frame
            assert num_frames <= self.num_frames, "Number of frames should be less or equal to the model setting"
            tile_pos_embed = self.positional_embedding.repeat(num_frames, 1)
            tile_tem_embed = self.temporal_positional_embedding[:num_frames].repeat_interleave(self.patches_per_frame, 0)
            total_pos_embed = tile_pos_embed + tile_tem_embed
            x = x + total_pos_embed.to(x.dtype).squeeze(0)
        x = self.ln_pre(x)
        x = _run_transformer(self.transformer, x, self.mask_type, self.mask_block_size, self.grid_size)
        x = self.ln_post(x)
        x = self.ffn(x)
        x = self.conv_out(x)
        hh, ww = self.grid_size
        sh, sw = self.patch_size
        if self.num_frames == 1:
            # rearrange "b (hh ww) (c sh sw) -> b c (hh sh) (ww sw)"
            b = x.shape[0]
            x = x.reshape(b, hh, ww, -1, sh, sw).permute(0, 3, 1, 4, 2, 5)
            x = x.reshape(b, x.shape[1], hh * sh, ww * sw)
        else:
            # rearrange "b (t hh ww) (c sh sw) -> b c t (hh sh) (ww sw)" / "(b t) (hh ww) (c sh sw) -> b c t (hh sh) (ww sw)"
            # (t: the frames counted above with cross_frames, else the model setting)
            b = x.shape[0] if self.cross_frames else x.shape[0] // num_frames
            x = x.reshape(b, num_frames, hh, ww, -1, sh, sw).permute(0, 4, 1, 2, 5, 3, 6)
            x = x.reshape(b, x.shape[1], num_frames, hh * sh, ww * sw)

        return x
