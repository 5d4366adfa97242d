"""fp32 CPU restatement of diffusers' AutoencoderKL ENCODER half (`Encoder` + `quant_conv` + `DiagonalGaussianDistribution`),
built from `oracle.vae_ref`'s blocks by import: the yardstick of the video-to-video tests.  Unpinned, like the decoder
oracle (diffusers is not installed: DESIGN §2); the key table is diffusers' own."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.vae_ref import MidBlockRef, ResnetBlock2DRef, VaeConfig


class DownsampleRef(nn.Module):
    """diffusers `Downsample2D(use_conv=True, padding=0)`: conv3x3 stride 2 on F.pad(x, (0, 1, 0, 1))."""

    def __init__(self, C):
        super().__init__()
        self.conv = nn.Conv2d(C, C, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class DownEncoderBlockRef(nn.Module):
    def __init__(self, cin, cout, n, groups, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2DRef(cin if j == 0 else cout, cout, groups) for j in range(n)])
        self.downsamplers = nn.ModuleList([DownsampleRef(cout)]) if downsample else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        return x


class EncoderRef(nn.Module):
    def __init__(self, cfg: VaeConfig):
        super().__init__()
        ch, g = cfg.block_out_channels, cfg.norm_num_groups
        self.conv_in = nn.Conv2d(cfg.out_channels, ch[0], 3, padding=1)
        blocks, prev = [], ch[0]
        for i, c in enumerate(ch):
            blocks.append(DownEncoderBlockRef(prev, c, cfg.layers_per_block, g, i != len(ch) - 1))
            prev = c
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = MidBlockRef(ch[-1], g)
        self.conv_norm_out = nn.GroupNorm(g, ch[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(ch[-1], 2 * cfg.latent_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        x = self.mid_block(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


class AutoencoderKLEncoderRef(nn.Module):
    """`encoder.*` + `quant_conv.*` of diffusers AutoencoderKL: encode(x) -> moments (n, 8, h, w)."""

    def __init__(self, cfg: VaeConfig = VaeConfig()):
        super().__init__()
        self.encoder = EncoderRef(cfg)
        self.quant_conv = nn.Conv2d(2 * cfg.latent_channels, 2 * cfg.latent_channels, 1)

    def moments(self, x):
        return self.quant_conv(self.encoder(x))


def posterior(moments, noise=None):
    """DiagonalGaussianDistribution: mean + exp(0.5 * clamp(logvar, -30, 20)) * noise (noise None: the mode)."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    if noise is None:
        return mean
    return mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise


def unit_map(u8):
    """uint8 (..., 3) HWC -> float32 NCHW in [-1, 1] (diffusers' video preprocessing), as fp16 values."""
    x = u8.float() / 255.0
    x = 2.0 * x - 1.0
    return x.half().float().permute(0, 3, 1, 2).contiguous()
