"""fp32 CPU restatement of the semantic-map grounding family (sem_grounding_net.py, sem_grounding_downsampler.py and the first-conv
concatenation of openaimodel_original.py:428-432), test infrastructure like tests/sp_ref.py, on which it stands: the ConvNeXt, the token
assembly and the UNet are sp_ref's, what is stated here is the family's own front end -- one-hot, nearest resize, in_conv / the two 4x4 convs.

The input is the uint8 class map [B, H, W]; the one-hot the reference is fed is built here on the fly (small maps only).  Pinned to the
reference's own outputs (tests/golden/sem_*.npz, tools/make_sem_goldens.py) by tests/test_sem_host.py.

``q``: sp_ref's optional rounding of every matrix operand (``sp_ref.fp16_operands``).  The in_conv is a gather of fp32 weights on the device,
so it is not rounded; the ConvNeXt behind it is.
"""
from __future__ import annotations

import dataclasses
from unittest import mock

import torch
import torch.nn.functional as F

import norel_ref
import sp_ref
from oracle import unet_ref

KEYS = ("sem", "mask")


def onehot(cmap: torch.Tensor, classes: int) -> torch.Tensor:
    """uint8 / integer [B, H, W] -> fp32 [B, classes, H, W] (gligen_inference.py:331-332)"""
    return F.one_hot(cmap.long(), classes).permute(0, 3, 1, 2).float().contiguous()


def in_conv(sd, cfg, cmap: torch.Tensor) -> torch.Tensor:
    """sem_grounding_net.py:46-47: interpolate(onehot, R) (nearest) -> Conv2d(classes, 3, 3, 1, 1) -> [B, 3, R, R]"""
    x = sp_ref.nearest_resize(onehot(cmap, cfg.sem_classes), cfg.sp_resize_input)
    return F.conv2d(x, sd["position_net.in_conv.weight"], sd["position_net.in_conv.bias"], padding=1)


def position_net(sd, cfg, cmap: torch.Tensor, mask: torch.Tensor, q=sp_ref._id) -> torch.Tensor:
    """sem_grounding_net.py:42-69: class map [B, H, W], mask [B] -> [B, T, out_dim]"""
    return sp_ref.position_net(sd, cfg, in_conv(sd, cfg, cmap), mask, q)       # (its nearest resize from R to R is the identity)


def downsampler(sd, cfg, cmap: torch.Tensor) -> torch.Tensor:
    """sem_grounding_downsampler.py:21-26: class map [B, H, W] -> [B, ds_out, R / 4, R / 4]"""
    R = cfg.ds_resize_input
    x = F.interpolate(onehot(cmap, cfg.sem_classes), (R, R), mode="nearest")
    x = F.silu(F.conv2d(x, sd["downsample_net.layers.0.weight"], sd["downsample_net.layers.0.bias"], stride=2, padding=1))
    return F.conv2d(x, sd["downsample_net.layers.2.weight"], sd["downsample_net.layers.2.bias"], stride=2, padding=1)


def first_conv_out(sd, cfg, x, cmap, first_conv=None) -> torch.Tensor:
    """input_blocks.0: the GLIGEN conv on cat([x, downsampler(class map)]), or the SD conv (``first_conv``) on the latent alone"""
    if first_conv is not None:
        return F.conv2d(x, first_conv["weight"], first_conv["bias"], padding=1)
    h = torch.cat([x, downsampler(sd, cfg, cmap)], dim=1)
    return F.conv2d(h, sd["input_blocks.0.0.weight"], sd["input_blocks.0.0.bias"], padding=1)


def unet_forward(sd, cfg, x, timesteps, context, grounding, extra_map, fuser_scale: float = 1.0, first_conv=None) -> torch.Tensor:
    """openaimodel_original.UNetModel.forward with the sem tokenizer and downsampler (sp_ref.unet_forward with this family's two stages).
    ``grounding``: class map and mask (null grounding: any map with mask 0, the reference's all-zero tensor has no class at all)."""
    objs = position_net(sd, cfg, grounding["sem"], grounding["mask"])
    h = x if first_conv is not None else torch.cat([x, downsampler(sd, cfg, extra_map)], dim=1)
    text = dataclasses.replace(cfg, grounding="text")
    with mock.patch.object(unet_ref, "position_net", lambda *a, **k: objs):
        return norel_ref.unet_forward(sd, text, h, timesteps, context, dict(boxes=None, masks=None, positive_embeddings=None),
                                      fuser_scale=fuser_scale, first_conv=first_conv)


def null_grounding(grounding):
    return {k: torch.zeros_like(grounding[k]) for k in KEYS}
