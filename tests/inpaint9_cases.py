"""Golden-vector case table of the inpaint_mode UNet (GLIGEN's checkpoint_inpainting_text*.pth: a 9-channel first conv over
cat([x, z0 * mask, mask]), openaimodel.py:293-299, :436-439), shared by tools/make_inpaint9_goldens.py (reference side, build container
only) and tests/test_inpaint9_host.py / tests/test_gpu_inpaint9.py.

Like tests/golden_cases.py every case is data; inputs and weights are recipe tensors, the fixtures hold the reference's OUTPUTS only.
The inpainting extra of a UNet case is an INPUT: a recipe z0 and the mask of the case's own boxes, put together as
gligen_inference.py:406-407 does.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np

from layoutllm_t2i_amd import host, recipe
from layoutllm_t2i_amd.arch import TINY

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IP_TINY = dataclasses.replace(TINY, inpaint_mode=True)
IP_TI_TINY = dataclasses.replace(TINY, inpaint_mode=True, grounding="text_image")
TI_KEYS = ("boxes", "masks", "text_masks", "image_masks", "text_embeddings", "image_embeddings")

CASES = [
    dict(name="ip9_unet_tiny_s1", kind="unet", family="text", B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, restore=False),
    dict(name="ip9_unet_tiny_s05", kind="unet", family="text", B=2, h=16, w=16, t=[401, 401], grounding="real", scale=0.5, restore=False),
    dict(name="ip9_unet_tiny_null", kind="unet", family="text", B=2, h=16, w=16, t=[401, 401], grounding="null", scale=1.0, restore=False),
    # restore_first_conv_from_SD() has been called: the reference's non-restorable branch, the GLIGEN conv stays (openaimodel.py:406-408)
    dict(name="ip9_unet_tiny_s0_restore", kind="unet", family="text", B=2, h=16, w=16, t=[21, 21], grounding="real", scale=0.0, restore=True),
    # the smallest legal non-square latent of the tiny architecture (three levels: multiples of 8)
    dict(name="ip9_unet_tiny_rect", kind="unet", family="text", B=2, h=8, w=16, t=[601, 601], grounding="real", scale=1.0, restore=False),
    dict(name="ip9_ti_unet_tiny_s1", kind="unet", family="text_image", B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, restore=False),
    # the extra of gligen_inference.py:400-407 from a recipe z0 and the boxes of the inpaint_masks case (tests/golden/inpaint_masks.npz)
    dict(name="ip9_extra", kind="extra", hw=16),
    # the RNG order, x0 and mask of plms_inpaint_tiny; crosses scale-0 steps (alpha 0 from step 3 on)
    dict(name="ip9_plms_tiny", kind="plms", family="text", B=2, hw=16, S=10, guidance=7.5, alpha_type=[0.3, 0.0, 0.7]),
]
UNET_CASES = [c for c in CASES if c["kind"] == "unet"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cfg_of(case):
    return IP_TI_TINY if case.get("family") == "text_image" else IP_TINY


def z0_of(tag, h, w):
    """a recipe stand-in for the encoded input image, batch 1 (gligen_inference.py:404)"""
    return (recipe.normal(f"inpaint9.{tag}.z0", (1, 4, h, w), 5) * np.float32(0.8)).astype(np.float32)


def make_extra(z0, mask):
    """gligen_inference.py:406-407 in numpy: masked_z = z0 * mask, cat([masked_z, mask], dim=1); z0 [1, 4, h, w] broadcasts over the mask's batch"""
    z0, mask = np.asarray(z0, np.float32), np.asarray(mask, np.float32)
    return np.concatenate([z0 * mask, mask], axis=1)


def case_inputs(case):
    """Numpy inputs of a case (weights excluded); UNet cases carry ``extra`` [B, 5, h, w]."""
    k = case["kind"]
    if k == "unet":
        h, w = case["h"], case["w"]
        hw = h if h == w else (h, w)
        text_image = case["family"] == "text_image"
        inp = recipe.synth_inputs(cfg_of(case), case["B"], hw, n_boxes=5 if text_image else 4, n_rel=3, seed=4321)
        mask = host.draw_masks_from_boxes(inp["boxes"], hw).numpy()
        inp["extra"] = make_extra(z0_of(case["name"], h, w), mask)
        return inp
    if k == "extra":
        boxes = np.load(os.path.join(GOLD, "inpaint_masks.npz"))["boxes"]
        return dict(boxes=boxes, z0=z0_of(case["name"], case["hw"], case["hw"]))
    if k == "plms":
        g = np.load(os.path.join(GOLD, "plms_inpaint_tiny.npz"))
        inp = recipe.synth_inputs(IP_TINY, case["B"], case["hw"], n_boxes=4, n_rel=3, seed=4321)       # = the inputs of plms_tiny
        inp["x0"], inp["mask"] = g["x0"], g["mask"]
        inp["extra"] = make_extra(g["x0"], g["mask"])
        inp["noises"] = [g[f"noise_{i:03d}"] for i in range(len(g["draw_shapes"]))]
        inp["draw_shapes"] = g["draw_shapes"]
        return inp
    raise ValueError(k)
