"""Checker of the MelGAN decoder: the network restated in torch from its published definition (Kumar et al. 2019,
``Generator(input_size=80, ngf=32, n_residual_layers=3)``), with ``torch.nn.utils.weight_norm`` on every convolution, run on the CPU.
float64 is the truth, float32 is the reference's own arithmetic.  Nothing here comes from the code under test."""
import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils import weight_norm


def WNConv1d(*a, **k):
    return weight_norm(nn.Conv1d(*a, **k))


def WNConvTranspose1d(*a, **k):
    return weight_norm(nn.ConvTranspose1d(*a, **k))


class ResnetBlock(nn.Module):
    def __init__(self, dim, dilation=1):
        super().__init__()
        self.block = nn.Sequential(
            nn.LeakyReLU(0.2),
            nn.ReflectionPad1d(dilation),
            WNConv1d(dim, dim, kernel_size=3, dilation=dilation),
            nn.LeakyReLU(0.2),
            WNConv1d(dim, dim, kernel_size=1),
        )
        self.shortcut = WNConv1d(dim, dim, kernel_size=1)

    def forward(self, x):
        return self.shortcut(x) + self.block(x)


class Generator(nn.Module):
    def __init__(self, input_size=80, ngf=32, n_residual_layers=3):
        super().__init__()
        ratios = [8, 8, 2, 2]
        mult = int(2 ** len(ratios))
        model = [nn.ReflectionPad1d(3), WNConv1d(input_size, mult * ngf, kernel_size=7, padding=0)]
        for r in ratios:
            model += [
                nn.LeakyReLU(0.2),
                WNConvTranspose1d(mult * ngf, mult * ngf // 2, kernel_size=r * 2, stride=r, padding=r // 2 + r % 2, output_padding=r % 2),
            ]
            for j in range(n_residual_layers):
                model += [ResnetBlock(mult * ngf // 2, dilation=3 ** j)]
            mult //= 2
        model += [nn.LeakyReLU(0.2), nn.ReflectionPad1d(3), WNConv1d(ngf, 1, kernel_size=7, padding=0), nn.Tanh()]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        return self.model(x)


GAIN = 1.7


def synthetic_generator(seed=0, gain=GAIN):
    """torch default initialisation under ``torch.manual_seed(seed)``, every weight_g times ``gain``, biases uniform in +-0.1: at gain 1
    the output is the last layer's bias whatever the input, at 2 most of it is saturated; 1.7 keeps every layer visible at the output."""
    torch.manual_seed(seed)
    g = Generator()
    with torch.no_grad():
        for name, p in g.named_parameters():
            if name.endswith("weight_g"):
                p.mul_(gain)
            elif name.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    return g.eval()


def synthetic_mel(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.clip(torch.randn(B, 80, T, generator=g) - 2.0, -5.0, 1.0)


_cache = {}


def generators():
    """(float32 module, float64 module) of the synthetic network, built once."""
    if "g" not in _cache:
        g32 = synthetic_generator()
        g64 = synthetic_generator().double()
        _cache["g"] = (g32, g64)
    return _cache["g"]


def state_dict():
    return {k: v.clone() for k, v in generators()[0].state_dict().items()}


def decode(mel):
    """-> (float64 result, float32 result), each [B, 256 T] on the CPU; cached per input."""
    key = (tuple(mel.shape), float(mel.double().sum()), float(mel.double().abs().sum()))
    if key not in _cache:
        g32, g64 = generators()
        with torch.no_grad():
            _cache[key] = (g64(mel.double()).squeeze(1), g32(mel.float()).squeeze(1))
    return _cache[key]


def distances(got, ref64):
    got, ref64 = torch.as_tensor(got).double().cpu(), ref64.double()
    return float((got - ref64).norm() / ref64.norm()), float((got - ref64).abs().max())
