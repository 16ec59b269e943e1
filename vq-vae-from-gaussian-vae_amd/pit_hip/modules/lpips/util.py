"""ActNorm (reference pit/modules/lpips/util.py:47-128); plain torch.  The reference's download helpers have no counterpart:
nothing is downloaded (pit_hip.modules.lpips.loss.lpips)."""
import torch
import torch.nn as nn


class ActNorm(nn.Module):
    """Per-channel affine h = scale (x + loc), initialised from the first training batch to zero mean and unit variance."""

    def __init__(self, num_features, logdet=False, affine=True, allow_reverse_init=False):
        assert affine
        super().__init__()
        self.logdet = logdet
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.allow_reverse_init = allow_reverse_init
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))

    def initialize(self, input):
        with torch.no_grad():
            flat = input.permute(1, 0, 2, 3).contiguous().view(input.shape[1], -1)
            mean, std = flat.mean(1).view(1, -1, 1, 1), flat.std(1).view(1, -1, 1, 1)
            self.loc.data.copy_(-mean)
            self.scale.data.copy_(1 / (std + 1e-6))

    def _first_batch(self, t):
        if self.training and self.initialized.item() == 0:
            self.initialize(t)
            self.initialized.fill_(1)

    def forward(self, input, reverse=False):
        if reverse:
            return self.reverse(input)
        squeeze = input.dim() == 2
        if squeeze:
            input = input[:, :, None, None]
        _, _, height, width = input.shape
        self._first_batch(input)
        h = self.scale * (input + self.loc)
        if squeeze:
            h = h.squeeze(-1).squeeze(-1)
        if self.logdet:
            logdet = height * width * torch.sum(torch.log(torch.abs(self.scale)))
            return h, logdet * torch.ones(input.shape[0]).to(input)
        return h

    def reverse(self, output):
        if self.training and self.initialized.item() == 0 and not self.allow_reverse_init:
            raise RuntimeError("Initializing ActNorm in reverse direction is disabled by default. "
                               "Use allow_reverse_init=True to enable.")
        squeeze = output.dim() == 2
        if squeeze:
            output = output[:, :, None, None]
        self._first_batch(output)
        h = output / self.scale - self.loc
        return h.squeeze(-1).squeeze(-1) if squeeze else h
