"""fp32 CPU restatement of the spatial grounding families ({canny,hed,depth,normal}_grounding_net.py, convnext.py, *_grounding_downsampler.py
and the first-conv concatenation of openaimodel_original.py:428-432), test infrastructure like tests/kp_ref.py: ``unet_forward`` runs the
upstream-block UNet of tests/norel_ref.py with ``oracle.unet_ref.position_net`` patched for the call.

Pinned to the reference's own outputs (tests/golden/sp_*.npz, tools/make_sp_goldens.py) by tests/test_sp_host.py.

``q``: an optional rounding applied to every matrix operand (``fp16_operands``: fp16 storage, fp32 accumulate -- the arithmetic of the HIP
tokenizer stage, restated on the CPU to MEASURE what that arithmetic costs against fp32; tests/test_gpu_sp.py derives its bound from it).
"""
from __future__ import annotations

import dataclasses
from unittest import mock

import torch
import torch.nn.functional as F

import norel_ref
from oracle import unet_ref

KEYS = ("map", "mask")
BB = "position_net.convnext_tiny_backbone"
EPS = 1e-6


def fp16_operands(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def _id(t):
    return t


def nearest_resize(x: torch.Tensor, R: int) -> torch.Tensor:
    """F.interpolate(x, R) in its default mode: source index floor(dst * in / out)"""
    B, C, H, W = x.shape
    iy = (torch.arange(R) * H) // R
    ix = (torch.arange(R) * W) // R
    return x[:, :, iy][:, :, :, ix]


def _ln_last(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def _ln_first(x, w, b):
    """convnext.py's channels_first LayerNorm on NCHW, in its order of operations (biased variance, then the division)"""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + EPS)
    return w[:, None, None] * x + b[:, None, None]


def convnext(sd, x: torch.Tensor, depths, dims, q=_id) -> torch.Tensor:
    """convnext.py:108-112: [B, 3, R, R] -> [B, dims[3], R/32, R/32] (NCHW like the reference; the blocks normalise and multiply in NHWC)"""
    x = F.conv2d(q(x), q(sd[BB + ".downsample_layers.0.0.weight"]), sd[BB + ".downsample_layers.0.0.bias"], stride=4)
    x = _ln_first(x, sd[BB + ".downsample_layers.0.1.weight"], sd[BB + ".downsample_layers.0.1.bias"])
    for i in range(4):
        if i > 0:
            n = _ln_first(x, sd[BB + f".downsample_layers.{i}.0.weight"], sd[BB + f".downsample_layers.{i}.0.bias"])
            x = F.conv2d(q(n), q(sd[BB + f".downsample_layers.{i}.1.weight"]), sd[BB + f".downsample_layers.{i}.1.bias"], stride=2)
        for j in range(depths[i]):
            p = BB + f".stages.{i}.{j}"
            h = F.conv2d(x, sd[p + ".dwconv.weight"], sd[p + ".dwconv.bias"], padding=3, groups=dims[i]).permute(0, 2, 3, 1)
            h = _ln_last(h, sd[p + ".norm.weight"], sd[p + ".norm.bias"])
            h = q(F.linear(q(h), q(sd[p + ".pwconv1.weight"]), sd[p + ".pwconv1.bias"]))        # (stored as fp16 rows before the GELU)
            h = F.gelu(h)
            if q is _id:
                h = sd[p + ".gamma"] * F.linear(h, sd[p + ".pwconv2.weight"], sd[p + ".pwconv2.bias"])
            else:       # gamma folded into the weight BEFORE it is rounded, as the packed operand is
                g = sd[p + ".gamma"]
                h = F.linear(q(h), q(g[:, None] * sd[p + ".pwconv2.weight"]), g * sd[p + ".pwconv2.bias"])
            x = x + h.permute(0, 3, 1, 2)
    return x


def position_net(sd, cfg, map_: torch.Tensor, mask: torch.Tensor, q=_id) -> torch.Tensor:
    """*_grounding_net.py:38-62: [B, 3, S, S], [B] -> [B, T, out_dim]"""
    B = map_.shape[0]
    f = convnext(sd, nearest_resize(map_, cfg.sp_resize_input), cfg.convnext_depths, cfg.convnext_dims, q)
    objs = f.reshape(B, f.shape[1], -1).permute(0, 2, 1)     # token = y * (R / 32) + x
    m = mask.view(-1, 1, 1)
    objs = objs * m + sd["position_net.null_feature"].view(1, 1, -1) * (1 - m)
    objs = objs + sd["position_net.pos_embedding"]
    h = q(F.silu(F.linear(q(objs), q(sd["position_net.linears.0.weight"]), sd["position_net.linears.0.bias"])))
    h = q(F.silu(F.linear(h, q(sd["position_net.linears.2.weight"]), sd["position_net.linears.2.bias"])))
    return F.linear(h, q(sd["position_net.linears.4.weight"]), sd["position_net.linears.4.bias"])


def downsampler(sd, cfg, extra: torch.Tensor) -> torch.Tensor:
    """*_grounding_downsampler.py: [B, 3, S, S] -> [B, ds_out, side, side]"""
    x = extra[:, :cfg.ds_in]
    side = 64 if cfg.ds_kind == "bicubic" else cfg.ds_resize_input
    x = F.interpolate(x, (side, side), mode="bicubic")
    if cfg.ds_kind == "bicubic":
        return x
    x = F.silu(F.conv2d(x, sd["downsample_net.layers.0.weight"], sd["downsample_net.layers.0.bias"], stride=2, padding=1))
    return F.conv2d(x, sd["downsample_net.layers.2.weight"], sd["downsample_net.layers.2.bias"], stride=2, padding=1)


def first_conv_out(sd, cfg, x, extra_map, first_conv=None) -> torch.Tensor:
    """input_blocks.0 (openaimodel_original.py:428-432, :443-444): the GLIGEN conv on cat([x, downsampler(extra_map)]), or the SD conv
    (``first_conv``: weight and bias) on the latent alone"""
    if first_conv is not None:
        return F.conv2d(x, first_conv["weight"], first_conv["bias"], padding=1)
    h = torch.cat([x, downsampler(sd, cfg, extra_map)], dim=1)
    return F.conv2d(h, sd["input_blocks.0.0.weight"], sd["input_blocks.0.0.bias"], padding=1)


def unet_forward(sd, cfg, x, timesteps, context, grounding, extra_map, fuser_scale: float = 1.0, first_conv=None) -> torch.Tensor:
    """openaimodel_original.UNetModel.forward with a downsampler: the GLIGEN first conv reads cat([x, downsampler(extra_map)]), the SD conv
    (``first_conv``) the latent alone.  ``grounding``: map and mask (null grounding: a zero map with mask 0)."""
    objs = position_net(sd, cfg, grounding["map"], grounding["mask"])
    h = x if first_conv is not None else torch.cat([x, downsampler(sd, cfg, extra_map)], dim=1)
    text = dataclasses.replace(cfg, grounding="text")
    with mock.patch.object(unet_ref, "position_net", lambda *a, **k: objs):
        return norel_ref.unet_forward(sd, text, h, timesteps, context, dict(boxes=None, masks=None, positive_embeddings=None),
                                      fuser_scale=fuser_scale, first_conv=first_conv)


def null_grounding(grounding):
    return {k: torch.zeros_like(grounding[k]) for k in KEYS}
