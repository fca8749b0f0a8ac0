"""Golden-vector case table of the semantic-map grounding family (GLIGEN's checkpoint_generation_sem.pth: the ConvNeXt tokenizer behind an
in_conv over a one-hot class map, and a grounding downsampler over the same one-hot).  Shared by tools/make_sem_goldens.py (reference side,
build container only) and tests/test_sem_host.py / tests/test_gpu_sem.py, built like tests/sp_cases.py (whose small backbone it uses).

Every case is data; inputs and weights are recipe tensors, the fixtures hold the reference's OUTPUTS only.  The input of a case is a uint8 class
map; the reference is fed its float one-hot, which is never stored.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import TINY, UNetConfig

import sp_cases as sc

MOD = sc.MOD
KEYS = ("sem", "mask")
CLASSES = 152


def targets():
    """(grounding_tokenizer target, grounding_downsampler target) of the family"""
    return sc.targets("sem")


def sem_cfg(base: UNetConfig, sp_resize: int, ds_resize: int = 64, classes: int = CLASSES, out_dim=None) -> UNetConfig:
    """``base`` as a semantic-map config on the small backbone (the sem counterpart of sp_cases.sp_cfg)"""
    return dataclasses.replace(base, relation=False, grounding="spatial", ds_kind="sem", ds_in=classes, ds_out=8, ds_resize_input=ds_resize,
                               sp_resize_input=sp_resize, max_objs=(sp_resize // 32) ** 2, convnext_depths=sc.SMALL_DEPTHS,
                               convnext_dims=sc.SMALL_DIMS, pos_out_dim=base.pos_out_dim if out_dim is None else out_dim)


SEM_TINY = sem_cfg(TINY, 64, 64)                       # 12-channel first conv, 16 x 16 latent, 4 tokens: the engine shape of sc.CANNY_TINY

CASES = [
    # the tokenizer alone, out_dim 64: T = 4 (resize 64 from a 96 x 96 map: nearest DOWN), sample 1 masked out; 152 classes and 5
    dict(name="sem_posnet_c152", kind="position_net", resize=64, S=96, B=2, out_dim=64, classes=152),
    dict(name="sem_posnet_c5", kind="position_net", resize=64, S=96, B=2, out_dim=64, classes=5),
    # the downsampler: nearest 96 -> 64, gather conv -> 32, conv -> [2, 8, 16, 16]
    dict(name="sem_ds", kind="downsampler", S=96, B=2, resize=64, classes=152),
    # openaimodel_original.UNetModel with the sem tokenizer and downsampler (TINY width)
    dict(name="sem_unet_s1", kind="unet", S=96, B=2, h=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False, classes=152),
    dict(name="sem_unet_s0_sd", kind="unet", S=96, B=2, h=16, t=[21, 21], grounding="real", scale=0.0, sdconv=True, classes=152),
    dict(name="sem_unet_null", kind="unet", S=96, B=2, h=16, t=[981, 981], grounding="null", scale=1.0, sdconv=False, classes=152),
    # names and shapes of the reference model's state dict
    dict(name="sem_params", kind="params", classes=152),
    # the reference's own prepare_batch_sem on a 96 x 64 "L" test image
    dict(name="sem_prepare_batch", kind="prepare_batch", B=2, classes=152),
]
UNET_CASES = [c for c in CASES if c["kind"] == "unet"]
POSNET_CASES = [c for c in CASES if c["kind"] == "position_net"]
DS_CASES = [c for c in CASES if c["kind"] == "downsampler"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cfg_of(case) -> UNetConfig:
    k = case["kind"]
    if k == "position_net":
        return sem_cfg(TINY, case["resize"], classes=case["classes"], out_dim=case["out_dim"])
    if k == "downsampler":
        return sem_cfg(TINY, 64, case["resize"], classes=case["classes"])
    return SEM_TINY


def class_map(name: str, B: int, H: int, W: int, classes: int, seed: int = 4321) -> np.ndarray:
    """uint8 [B, H, W], random over all classes per pixel; pixel (0, 0) of every sample is class 0 and pixel (0, 1) class ``classes`` - 1"""
    u = recipe.uniform("in.sem." + name, (B, H, W), seed)
    m = np.minimum(np.floor((u.astype(np.float64) + 1.0) * 0.5 * classes), classes - 1).astype(np.uint8)
    m[:, 0, 0], m[:, 0, 1] = 0, classes - 1
    return m


def onehot(cmap: np.ndarray, classes: int) -> np.ndarray:
    """the reference's input: fp32 [B, classes, H, W] (built on the fly, never stored)"""
    return (cmap[:, None].astype(np.int64) == np.arange(classes).reshape(1, -1, 1, 1)).astype(np.float32)


def case_inputs(case):
    """Numpy inputs of a case (weights excluded): the class map ``sem`` uint8 [B, S, S] and what goes with it"""
    cfg = cfg_of(case)
    B, S = case["B"], case["S"]
    out = dict(sem=class_map(case["name"], B, S, S, case["classes"]))
    if case["kind"] == "position_net":
        out["mask"] = np.array([1.0] + [0.0] * (B - 1), np.float32)
    if case["kind"] == "unet":
        out["mask"] = np.ones((B,), np.float32)
        out["x"] = recipe.normal("in.x", (B, cfg.in_channels, case["h"], case["h"]), 4321)
        out["context"] = recipe.normal("in.context", (B, 77, cfg.context_dim), 4321)
        out["uc"] = np.repeat(recipe.normal("in.uc", (1, 77, cfg.context_dim), 4321), B, axis=0)
    return out


def test_image() -> np.ndarray:
    """uint8 [64, 96] (a 96 x 64 landscape "L" image of class ids: the centre crop cuts 16 columns off each side): 8 x 8 blocks of the classes
    0 .. 151 in a fixed scramble; the blocks at (0, 2) and (0, 3), inside the crop, are the classes 0 and 151"""
    y, x = np.mgrid[0:64, 0:96]
    m = (((x // 8) * 37 + (y // 8) * 101 + 5) % CLASSES).astype(np.uint8)
    m[0:8, 16:24], m[0:8, 24:32] = 0, CLASSES - 1
    return m
