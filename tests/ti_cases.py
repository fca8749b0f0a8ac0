"""Golden-vector case table of the text_image grounding family (GLIGEN's *_box_text_image checkpoints), shared by
tools/make_ti_goldens.py (reference side, build container only) and tests/test_ti_host.py / tests/test_gpu_ti.py.

Like tests/golden_cases.py every case is data; inputs and weights are recipe tensors, the fixtures hold the reference's OUTPUTS only.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import TINY

CTX = 768
MO = 30
TI_TINY = dataclasses.replace(TINY, grounding="text_image")

CASES = [
    # boxes 0..3 of each sample: text only, image only, both, grounded on neither (box alone); the rest padded
    dict(name="ti_posnet", kind="position_net", B=2, n_boxes=4),
    dict(name="ti_posnet_null", kind="position_net", B=2, n_boxes=0),
    dict(name="ti_unet_tiny_s1", kind="unet", B=2, h=16, w=16, t=[981, 981], scale=1.0, sdconv=False),
    dict(name="ti_unet_tiny_s0_sd", kind="unet", B=2, h=16, w=16, t=[21, 21], scale=0.0, sdconv=True),
    dict(name="ti_unet_tiny_s05", kind="unet", B=2, h=16, w=16, t=[401, 401], scale=0.5, sdconv=False),
    dict(name="ti_unet_tiny_rect", kind="unet", B=2, h=16, w=24, t=[601, 601], scale=1.0, sdconv=False),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def rnd(tag, shape, seed=7):
    return recipe.normal(f"golden.{tag}", tuple(shape), seed)


def unet_inputs(case, cfg=TI_TINY):
    """recipe.synth_inputs of a text_image config: six grounding tensors, 5 boxes per sample grounded in rotation on a phrase, an image,
    or both"""
    hw = case["h"] if case["h"] == case["w"] else (case["h"], case["w"])
    return recipe.synth_inputs(cfg, case["B"], hw, n_boxes=5, n_rel=3, seed=4321)


def case_inputs(case):
    k, nm = case["kind"], case["name"]
    if k == "position_net":
        B, nb = case["B"], case["n_boxes"]
        boxes = np.zeros((B, MO, 4), np.float32)
        masks = np.zeros((B, MO), np.float32)
        tm = np.zeros((B, MO), np.float32)
        im = np.zeros((B, MO), np.float32)
        te = np.zeros((B, MO, CTX), np.float32)
        ie = np.zeros((B, MO, CTX), np.float32)
        if nb:
            u = np.abs(recipe.uniform(f"golden.{nm}.boxes", (B, nb, 4), 7))
            boxes[:, :nb] = np.sort(u.reshape(B, nb, 2, 2), axis=2).reshape(B, nb, 4)
            masks[:, :nb] = 1
            # embeddings are left non-zero on EVERY valid box, so that a mask the blend ignores shows in the output
            te[:, :nb] = rnd(f"{nm}.text", (B, nb, CTX))
            ie[:, :nb] = rnd(f"{nm}.image", (B, nb, CTX))
            for i in range(nb):
                tm[:, i] = 1.0 if i % 4 in (0, 2) else 0.0
                im[:, i] = 1.0 if i % 4 in (1, 2) else 0.0
        return dict(boxes=boxes, masks=masks, text_masks=tm, image_masks=im, text_embeddings=te, image_embeddings=ie)
    if k == "unet":
        return unet_inputs(case)
    raise ValueError(k)
