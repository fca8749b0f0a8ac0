"""fp32 CPU restatement of the UNet forward WITHOUT the rela_fuse chain -- the upstream GLIGEN transformer block
(attention_original.py:312-316: attn1 -> fuser -> attn2 -> ff) -- test infrastructure like tests/ti_ref.py, built on the pieces of
oracle/unet_ref.py: ``transformer_block`` below is made of its ``attention`` / ``gated_self_attention`` / ``feed_forward`` / ``_layer_norm``,
and ``unet_forward`` runs ``oracle.unet_ref.unet_forward`` (through tests/ti_ref.py / tests/inpaint9_ref.py for those families) with that
block patched in for the call.  No ``relations``, no box rectangles.

Pinned to the reference's own pre-modification UNet (tests/golden/norel_*.npz, tools/make_norel_goldens.py) by tests/test_norel_host.py; it
serves the shapes that have no golden.
"""
from __future__ import annotations

from unittest import mock

import torch

import inpaint9_ref
import ti_ref
from oracle import unet_ref


def transformer_block(sd, p, x, context, objs, relations, boxes, masks, h, w, heads, fuser_scale):
    """attention_original.py:312-316 (the signature of oracle.unet_ref.transformer_block; relations / boxes / masks / h / w are not read)"""
    n1 = unet_ref._layer_norm(sd, p + ".norm1", x)
    x = unet_ref.attention(sd, p + ".attn1", n1, n1, n1, heads) + x
    x = unet_ref.gated_self_attention(sd, p + ".fuser", x, objs, heads, fuser_scale)
    x = unet_ref.attention(sd, p + ".attn2", unet_ref._layer_norm(sd, p + ".norm2", x), context, context, heads) + x
    x = unet_ref.feed_forward(sd, p + ".ff", unet_ref._layer_norm(sd, p + ".norm3", x)) + x
    return x


def unet_forward(sd, cfg, x, timesteps, context, grounding, fuser_scale: float = 1.0, first_conv=None, extra=None) -> torch.Tensor:
    """``grounding``: the three tensors of the text family (boxes, masks, positive_embeddings) or the six of ti_ref.KEYS; null grounding =
    zeros.  ``extra``: the inpainting_extra_input of an inpaint_mode config.  ``sd`` needs no ``*.rela_fuse.*`` tensor."""
    with mock.patch.object(unet_ref, "transformer_block", transformer_block):
        if cfg.inpaint_mode:
            return inpaint9_ref.unet_forward(sd, cfg, x, extra, timesteps, context, None, grounding, fuser_scale=fuser_scale)
        if cfg.grounding == "text_image":
            return ti_ref.unet_forward(sd, cfg, x, timesteps, context, None, grounding, fuser_scale=fuser_scale, first_conv=first_conv)
        return unet_ref.unet_forward(sd, cfg, x, timesteps, context, None, grounding["boxes"], grounding["masks"],
                                     grounding["positive_embeddings"], fuser_scale=fuser_scale, first_conv=first_conv)


def null_grounding(grounding):
    return {k: torch.zeros_like(v) for k, v in grounding.items()}


def make_eps_fn(sd, cfg, inp, guidance, first_conv_sd):
    """Guided epsilon for oracle.plms_ref.plms_sample with the sampler's side effects (fuser scale per step, the permanent first-conv switch on
    the first scale-0 step), as tests/test_oracle_golden.py::make_eps_fn does for the relation-aware model."""
    state = dict(sd_conv=False)
    g = {k: inp[k] for k in ("boxes", "masks", "positive_embeddings")}
    gn = null_grounding(g)

    def eps_fn(x, t, i, alpha):
        if alpha == 0:
            state["sd_conv"] = True
        fc = first_conv_sd if state["sd_conv"] else None
        e_c = unet_forward(sd, cfg, x, t, inp["context"], g, fuser_scale=alpha, first_conv=fc)
        e_u = unet_forward(sd, cfg, x, t, inp["uc"], gn, fuser_scale=alpha, first_conv=fc)
        return e_u + guidance * (e_c - e_u)
    return eps_fn
