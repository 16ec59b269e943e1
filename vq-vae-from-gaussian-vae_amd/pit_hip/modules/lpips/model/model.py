"""The PatchGAN discriminator (reference pit/modules/lpips/model/model.py), same ``main.N`` keys; plain torch."""
import torch.nn as nn

from ..util import ActNorm


def weights_init(m):
    name = m.__class__.__name__
    if "Conv" in name:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif "BatchNorm" in name:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class NLayerDiscriminator(nn.Module):
    """4x4 convolutions: ``n_layers`` of stride 2 (ndf, 2 ndf, .. capped at 8 ndf), one of stride 1, then one to a single-channel
    patch map; BatchNorm (conv without bias) or ActNorm (``use_actnorm``, conv with bias) and LeakyReLU(0.2) between them."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        norm_layer = ActNorm if use_actnorm else nn.BatchNorm2d
        use_bias = norm_layer is not nn.BatchNorm2d
        seq = [nn.Conv2d(input_nc, ndf, kernel_size=4, stride=2, padding=1), nn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=2 if n < n_layers else 1, padding=1, bias=use_bias),
                    norm_layer(ndf * mult), nn.LeakyReLU(0.2, True)]
        seq.append(nn.Conv2d(ndf * mult, 1, kernel_size=4, stride=1, padding=1))
        self.main = nn.Sequential(*seq)

    def forward(self, input):
        return self.main(input)
