"""GeneralLPIPSWithDiscriminator (reference pit/modules/losses/discriminator_loss.py): L1 + LPIPS reconstruction loss, the
adaptive-weight generator loss and the discriminator loss, with the reference's constructor arguments, ``forward_keys``, log keys
and ``state_dict`` keys (``perceptual_loss.*``, ``logvar``, ``discriminator.*``).  The LPIPS heads run on the fused HIP kernels
(pit_hip.modules.lpips.loss.lpips); everything else is plain torch.

The LPIPS weights are never downloaded: they arrive with the engine checkpoint (``loss.perceptual_loss.*``) or through
``perceptual_loss.load_from_pretrained`` / ``load_state_dict``; until then the first ``forward`` raises.

Refused, clearly: the VF-alignment branch (``zp`` / ``aux_feature`` in the regularization log; the engine refuses ``use_vf``),
``log_images`` (needs matplotlib and torchvision), ``dims > 2`` and ``scale_input_to_tgt_size``."""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from ...util import instantiate_from_config
from ..lpips.loss.lpips import LPIPS
from ..lpips.model.model import weights_init
from ..lpips.vqperceptual import hinge_d_loss, vanilla_d_loss


class GeneralLPIPSWithDiscriminator(nn.Module):
    def __init__(self, disc_start: int, logvar_init: float = 0.0, disc_num_layers: int = 3, disc_in_channels: int = 3,
                 disc_factor: float = 1.0, disc_weight: float = 1.0, perceptual_weight: float = 1.0, disc_loss: str = "hinge",
                 scale_input_to_tgt_size: bool = False, dims: int = 2, learn_logvar: bool = False,
                 regularization_weights: Union[None, Dict[str, float]] = None, additional_log_keys: Optional[List[str]] = None,
                 discriminator_config: Optional[Dict] = None, vf_weight=0.1, adaptive_vf=True, cos_margin=0.5,
                 distmat_margin=0.25, distmat_weight=1.0, cos_weight=1.0):
        super().__init__()
        if dims > 2:
            raise NotImplementedError(f"dims={dims}: the per-frame (video) perceptual loss is not implemented")
        if scale_input_to_tgt_size:
            raise NotImplementedError("scale_input_to_tgt_size is not implemented")
        assert disc_loss in ["hinge", "vanilla"]
        self.dims = dims
        self.scale_input_to_tgt_size = scale_input_to_tgt_size
        self.perceptual_loss = LPIPS().eval()
        self.perceptual_weight = perceptual_weight
        # accepted for the reference's configs; the branch that reads them is refused in forward
        self.vf_weight, self.adaptive_vf, self.cos_margin = vf_weight, adaptive_vf, cos_margin
        self.distmat_margin, self.distmat_weight, self.cos_weight = distmat_margin, distmat_weight, cos_weight
        self.logvar = nn.Parameter(torch.full((), logvar_init), requires_grad=learn_logvar)
        self.learn_logvar = learn_logvar
        if discriminator_config is None:
            discriminator_config = {"target": "pit.modules.lpips.model.model.NLayerDiscriminator",
                                    "params": {"input_nc": disc_in_channels, "n_layers": disc_num_layers, "use_actnorm": False}}
        self.discriminator = instantiate_from_config(discriminator_config).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.regularization_weights = regularization_weights if regularization_weights is not None else {}
        self.forward_keys = ["optimizer_idx", "global_step", "last_layer", "enc_last_layer", "split", "regularization_log"]
        self.additional_log_keys = set(additional_log_keys if additional_log_keys is not None else [])
        self.additional_log_keys.update(set(self.regularization_weights.keys()))

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        return self.discriminator.parameters()

    def get_trainable_autoencoder_parameters(self) -> Iterator[nn.Parameter]:
        if self.learn_logvar:
            yield self.logvar
        yield from ()

    def log_images(self, inputs, reconstructions):
        raise NotImplementedError("log_images needs matplotlib and torchvision; it is not implemented")

    def calculate_adaptive_weight(self, nll_loss: torch.Tensor, g_loss: torch.Tensor, last_layer: torch.Tensor) -> torch.Tensor:
        nll_grads = torch.autograd.grad(nll_loss, last_layer, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
        d_weight = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight

    def get_nll_loss(self, rec_loss: torch.Tensor, weights: Optional[Union[float, torch.Tensor]] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        nll_loss = rec_loss / torch.exp(self.logvar) + self.logvar
        weighted_nll_loss = nll_loss if weights is None else weights * nll_loss
        weighted_nll_loss = torch.sum(weighted_nll_loss) / weighted_nll_loss.shape[0]
        nll_loss = torch.sum(nll_loss) / nll_loss.shape[0]
        return nll_loss, weighted_nll_loss

    def forward(self, inputs: torch.Tensor, reconstructions: torch.Tensor, *, regularization_log: Dict[str, torch.Tensor],
                optimizer_idx: int, global_step: int, last_layer: torch.Tensor, enc_last_layer=None, split: str = "train",
                weights: Union[None, float, torch.Tensor] = None) -> Tuple[torch.Tensor, dict]:
        if "zp" in regularization_log and "aux_feature" in regularization_log:
            raise NotImplementedError("the VF-alignment loss (zp / aux_feature in the regularization log) is not implemented")
        rec_loss = torch.abs(inputs.contiguous() - reconstructions.contiguous())
        if self.perceptual_weight > 0:
            p_loss = self.perceptual_loss(inputs.contiguous(), reconstructions.contiguous())
            rec_loss = rec_loss + self.perceptual_weight * p_loss
        nll_loss, weighted_nll_loss = self.get_nll_loss(rec_loss, weights)
        running = global_step >= self.discriminator_iter_start or not self.training

        if optimizer_idx == 0:      # generator update
            if running:
                logits_fake = self.discriminator(reconstructions.contiguous())
                g_loss = -torch.mean(logits_fake)
                d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer) if self.training \
                    else torch.tensor(1.0)
            else:
                d_weight = torch.tensor(0.0)
                g_loss = torch.tensor(0.0, requires_grad=True)
            loss = weighted_nll_loss + d_weight * self.disc_factor * g_loss
            log = dict()
            for k in regularization_log:
                if k in self.regularization_weights:
                    loss = loss + self.regularization_weights[k] * regularization_log[k]
                if k in self.additional_log_keys:
                    log[f"{split}/{k}"] = regularization_log[k].detach().float().mean()
            log.update({f"{split}/loss/total": loss.clone().detach().mean(),
                        f"{split}/loss/nll": nll_loss.detach().mean(),
                        f"{split}/loss/rec": rec_loss.detach().mean(),
                        f"{split}/loss/g": g_loss.detach().mean(),
                        f"{split}/scalars/logvar": self.logvar.detach(),
                        f"{split}/scalars/d_weight": d_weight.detach()})
            return loss, log
        if optimizer_idx == 1:      # discriminator update
            logits_real = self.discriminator(inputs.contiguous().detach())
            logits_fake = self.discriminator(reconstructions.contiguous().detach())
            d_loss = self.disc_factor * self.disc_loss(logits_real, logits_fake) if running \
                else torch.tensor(0.0, requires_grad=True)
            log = {f"{split}/loss/disc": d_loss.clone().detach().mean(),
                   f"{split}/logits/real": logits_real.detach().mean(),
                   f"{split}/logits/fake": logits_fake.detach().mean()}
            return d_loss, log
        raise NotImplementedError(f"Unknown optimizer_idx {optimizer_idx}")
