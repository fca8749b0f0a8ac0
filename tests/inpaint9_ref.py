"""fp32 CPU mirror of an inpaint_mode UNet forward (openaimodel.py:436-439), test infrastructure like tests/ti_ref.py:
``h = cat([x, inpainting_extra_input], dim=1)`` and then oracle.unet_ref.unet_forward, which convolves whatever channel count ``x`` and
``input_blocks.0.0.weight`` have.  The text_image family goes through tests/ti_ref.py the same way.

Pinned to the reference's own outputs (tests/golden/ip9_*.npz, tools/make_inpaint9_goldens.py) by tests/test_inpaint9_host.py.
"""
from __future__ import annotations

import torch

import ti_ref
from oracle import unet_ref


def cat_extra(x, extra):
    """[B, 4, h, w] and [1|B, 5, h, w] -> [B, 9, h, w]"""
    return torch.cat([x, extra.expand(x.shape[0], -1, -1, -1)], dim=1)


def unet_forward(sd, cfg, x, extra, timesteps, context, relations, grounding, fuser_scale: float = 1.0) -> torch.Tensor:
    """``grounding``: the three tensors of the text family (boxes, masks, positive_embeddings) or the six of ti_ref.KEYS; null grounding =
    zeros.  There is no first-conv override: an inpaint_mode model's conv is not restorable (openaimodel.py:296, :406-408)."""
    h = cat_extra(x, extra)
    if cfg.grounding == "text_image":
        return ti_ref.unet_forward(sd, cfg, h, timesteps, context, relations, grounding, fuser_scale=fuser_scale)
    return unet_ref.unet_forward(sd, cfg, h, timesteps, context, relations, grounding["boxes"], grounding["masks"],
                                 grounding["positive_embeddings"], fuser_scale=fuser_scale)


def null_grounding(grounding):
    return {k: torch.zeros_like(v) for k, v in grounding.items()}
