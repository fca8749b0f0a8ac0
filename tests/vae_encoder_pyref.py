"""From-scratch fp32 CPU mirror of AutoencoderKL.encode (GLIGEN/ldm/models/autoencoder.py:34-38): Encoder.forward
(model.py:428-459, no down-level attention) with the asymmetrically padded stride-2 Downsample (model.py:60-79), quant_conv and
DiagonalGaussianDistribution.sample() (distributions.py:24-36) with the noise given, times scale_factor.  Test infrastructure:
the ResnetBlock / AttnBlock pieces come from the decoder's oracle (oracle/vae_ref.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.vae_ref import _conv, _gn, attn_block, resnet_block


def encode(sd, x: torch.Tensor, ch_mult, num_res_blocks: int, noise: torch.Tensor, scale_factor: float = 0.18215):
    """Returns (z, mean): z = (mean + exp(clamp(logvar, -30, 20) / 2) * noise) * scale_factor."""
    h = _conv(sd, "encoder.conv_in", x, 1)
    nres = len(ch_mult)
    for lvl in range(nres):
        for i in range(num_res_blocks):
            h = resnet_block(sd, f"encoder.down.{lvl}.block.{i}", h)
        if lvl != nres - 1:
            p = f"encoder.down.{lvl}.downsample.conv"
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), sd[p + ".weight"], sd[p + ".bias"], stride=2)
    h = resnet_block(sd, "encoder.mid.block_1", h)
    h = attn_block(sd, "encoder.mid.attn_1", h)
    h = resnet_block(sd, "encoder.mid.block_2", h)
    h = _conv(sd, "encoder.conv_out", F.silu(_gn(sd, "encoder.norm_out", h)), 1)
    mean, logvar = torch.chunk(_conv(sd, "quant_conv", h), 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    return (mean + std * noise) * scale_factor, mean
