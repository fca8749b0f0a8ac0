"""fp32 CPU restatement of the text_image PositionNet (text_image_grounding_net.py:41-65), test infrastructure like oracle/unet_ref.py,
on which it is built: ``fourier_embed`` comes from there, and ``unet_forward`` runs ``oracle.unet_ref.unet_forward`` with its
``position_net`` patched for the call -- the UNet handles the 2 * max_objs tokens unchanged (openaimodel.py:425).

Pinned to the reference's own outputs (tests/golden/ti_*.npz, tools/make_ti_goldens.py) by tests/test_ti_host.py.
"""
from __future__ import annotations

from unittest import mock

import torch
import torch.nn.functional as F

from oracle import unet_ref

KEYS = ("boxes", "masks", "text_masks", "image_masks", "text_embeddings", "image_embeddings")


def position_net(sd, boxes, masks, text_masks, image_masks, text_embeddings, image_embeddings, num_freqs: int = 8) -> torch.Tensor:
    p = "position_net"
    m, tm, im = masks.unsqueeze(-1), text_masks.unsqueeze(-1), image_masks.unsqueeze(-1)
    xyxy = unet_ref.fourier_embed(boxes, num_freqs)
    te = text_embeddings * tm + (1 - tm) * sd[p + ".null_text_feature"].view(1, 1, -1)
    ie = image_embeddings * im + (1 - im) * sd[p + ".null_image_feature"].view(1, 1, -1)
    xy = xyxy * m + (1 - m) * sd[p + ".null_position_feature"].view(1, 1, -1)

    def mlp(chain, h):
        h = F.silu(F.linear(h, sd[f"{p}.{chain}.0.weight"], sd[f"{p}.{chain}.0.bias"]))
        h = F.silu(F.linear(h, sd[f"{p}.{chain}.2.weight"], sd[f"{p}.{chain}.2.bias"]))
        return F.linear(h, sd[f"{p}.{chain}.4.weight"], sd[f"{p}.{chain}.4.bias"])
    return torch.cat([mlp("linears_text", torch.cat([te, xy], -1)), mlp("linears_image", torch.cat([ie, xy], -1))], dim=1)


def unet_forward(sd, cfg, x, timesteps, context, relations, grounding, fuser_scale: float = 1.0, first_conv=None) -> torch.Tensor:
    """UNetModel.forward with the text_image PositionNet; ``grounding``: the six tensors of KEYS (null grounding = all zero)."""
    objs = position_net(sd, *(grounding[k] for k in KEYS), cfg.fourier_freqs)
    with mock.patch.object(unet_ref, "position_net", lambda *a, **k: objs):
        return unet_ref.unet_forward(sd, cfg, x, timesteps, context, relations, grounding["boxes"], grounding["masks"],
                                     grounding["text_embeddings"], fuser_scale=fuser_scale, first_conv=first_conv)


def null_grounding(grounding):
    return {k: torch.zeros_like(grounding[k]) for k in KEYS}
