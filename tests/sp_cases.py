"""Golden-vector case table of the spatial grounding families (GLIGEN's canny / hed / depth / normal checkpoints: a ConvNeXt tokenizer over a
map and a grounding downsampler concatenated into the first conv).  Shared by tools/make_sp_goldens.py (reference side, build container only)
and tests/test_sp_host.py / tests/test_gpu_sp.py.

Every case is data; inputs and weights are recipe tensors, the fixtures hold the reference's OUTPUTS only.  ``PositionNet`` hard-codes a
768-wide last ConvNeXt stage, so the small backbone is depths (1, 1, 2, 1), dims (96, 64, 128, 768): it keeps C = 96, the width that is not a
multiple of 64.  The UNet is the upstream one (``relation=False``), the only block the families run on.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import SPATIAL_FAMILIES, TINY, UNetConfig

MOD = "ldm.modules.diffusionmodules."
FAMILIES = tuple(SPATIAL_FAMILIES)                     # canny_grounding_net, hed_..., depth_..., normal_...
SMALL_DEPTHS, SMALL_DIMS = (1, 1, 2, 1), (96, 64, 128, 768)
KEYS = ("map", "mask")


def targets(family: str):
    """(grounding_tokenizer target, grounding_downsampler target) of a family ("canny", "hed", "depth", "normal")"""
    return MOD + f"{family}_grounding_net.PositionNet", MOD + f"{family}_grounding_downsampler.GroundingDownsampler"


def sp_cfg(base: UNetConfig, family: str, sp_resize: int, ds_resize: int = 64, out_dim=None) -> UNetConfig:
    """``base`` as a spatial config of one family on the small backbone"""
    _, kind, cin, cout = SPATIAL_FAMILIES[family + "_grounding_net"]
    return dataclasses.replace(base, relation=False, grounding="spatial", ds_kind=kind, ds_in=cin, ds_out=cout, ds_resize_input=ds_resize,
                               sp_resize_input=sp_resize, max_objs=(sp_resize // 32) ** 2, convnext_depths=SMALL_DEPTHS, convnext_dims=SMALL_DIMS,
                               pos_out_dim=base.pos_out_dim if out_dim is None else out_dim)


CANNY_TINY = sp_cfg(TINY, "canny", 64, 64)             # 12-channel first conv, 16 x 16 latent, 4 tokens
HED_TINY = sp_cfg(TINY, "hed", 64)                     # 5-channel first conv, 64 x 64 latent (hard-coded by the reference), 4 tokens

CASES = [
    # the tokenizer alone, out_dim 64 (small fixtures): T = 4 (resize 64 from a 96 x 96 map: nearest DOWN) and T = 64 (resize 256 from 128: UP);
    # sample 1 is masked out.  t4 holds the output of all four families' PositionNet classes (they are one computation)
    dict(name="sp_posnet_t4", kind="position_net", resize=64, S=96, B=2, out_dim=64),
    dict(name="sp_posnet_t64", kind="position_net", resize=256, S=128, B=2, out_dim=64),
    # the downsamplers: canny / depth (channel 0), normal (3 channels): bicubic 128 -> 64, two convs -> [B, 8, 16, 16]; hed: bicubic 512 -> 64
    dict(name="sp_ds_canny", kind="downsampler", family="canny", S=128, B=2, resize=64),
    dict(name="sp_ds_depth", kind="downsampler", family="depth", S=128, B=2, resize=64),
    dict(name="sp_ds_normal", kind="downsampler", family="normal", S=128, B=2, resize=64),
    dict(name="sp_ds_hed", kind="downsampler", family="hed", S=512, B=1, resize=None),
    # openaimodel_original.UNetModel with a downsampler (TINY width)
    dict(name="sp_unet_canny_s1", kind="unet", family="canny", S=96, B=2, h=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    dict(name="sp_unet_canny_s0_sd", kind="unet", family="canny", S=96, B=2, h=16, t=[21, 21], grounding="real", scale=0.0, sdconv=True),
    dict(name="sp_unet_canny_null", kind="unet", family="canny", S=96, B=2, h=16, t=[981, 981], grounding="null", scale=1.0, sdconv=False),
    dict(name="sp_unet_hed_s1", kind="unet", family="hed", S=128, B=1, h=64, t=[981], grounding="real", scale=1.0, sdconv=False),
    dict(name="sp_unet_hed_s0_sd", kind="unet", family="hed", S=128, B=1, h=64, t=[21], grounding="real", scale=0.0, sdconv=True),
    # names and shapes of the reference model's state dict (tiny canny)
    dict(name="sp_params", kind="params", family="canny"),
    # the reference's own prepare_batch_canny / _hed / _depth / _normal on a 96 x 64 test image
    dict(name="sp_prepare_batch", kind="prepare_batch", B=2),
]
UNET_CASES = [c for c in CASES if c["kind"] == "unet"]
POSNET_CASES = [c for c in CASES if c["kind"] == "position_net"]
DS_CASES = [c for c in CASES if c["kind"] == "downsampler"]


def h0_stride(case) -> int:
    """the UNet fixtures keep every h0_stride-th pixel (per axis) of the first conv's output: all of a 16 x 16 latent, 1 / 16 of a 64 x 64 one"""
    return max(1, case["h"] // 16)


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cfg_of(case) -> UNetConfig:
    k = case["kind"]
    if k == "position_net":
        return sp_cfg(TINY, "canny", case["resize"], out_dim=case["out_dim"])
    if k == "downsampler":
        return sp_cfg(TINY, case["family"], 64, case["resize"] or 64)
    return HED_TINY if case.get("family") == "hed" else CANNY_TINY


def map_input(name: str, B: int, S: int, seed: int = 4321) -> np.ndarray:
    """a map [B, 3, S, S] in [-1, 1] whose three channels differ (the reference's loaders give grey maps; the normal family reads all three)"""
    return recipe.uniform("in.map." + name, (B, 3, S, S), seed)


def case_inputs(case):
    """Numpy inputs of a case (weights excluded)."""
    cfg = cfg_of(case)
    B, S = case["B"], case["S"]
    out = dict(map=map_input(case["name"], B, S))
    if case["kind"] == "position_net":
        out["mask"] = np.array([1.0] + [0.0] * (B - 1), np.float32)
    if case["kind"] == "unet":
        out["mask"] = np.ones((B,), np.float32)
        out["x"] = recipe.normal("in.x", (B, cfg.in_channels, case["h"], case["h"]), 4321)
        out["context"] = recipe.normal("in.context", (B, 77, cfg.context_dim), 4321)
        out["uc"] = np.repeat(recipe.normal("in.uc", (1, 77, cfg.context_dim), 4321), B, axis=0)
    return out


def test_image() -> np.ndarray:
    """uint8 [64, 96, 3] (a 96 x 64 landscape image: the centre crop cuts 16 columns off each side), smooth enough to survive PIL's resize"""
    y, x = np.mgrid[0:64, 0:96]
    r = (x * 255 // 95).astype(np.uint8)
    g = (y * 255 // 63).astype(np.uint8)
    b = (((x // 8 + y // 8) % 2) * 200 + 20).astype(np.uint8)
    return np.stack([r, g, b], -1)
