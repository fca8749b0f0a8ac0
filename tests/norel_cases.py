"""Golden-vector case table of the UNet WITHOUT the rela_fuse chain (``UNetConfig.relation = False``): the upstream GLIGEN transformer block
(attention_original.py:312-316: attn1 -> fuser -> attn2 -> ff) that every public GLIGEN checkpoint was trained on.  Shared by
tools/make_norel_goldens.py (reference side, build container only) and tests/test_norel_host.py / tests/test_gpu_norel.py.

Like tests/golden_cases.py every case is data; inputs and weights are recipe tensors, the fixtures hold the reference's OUTPUTS only.  Recipe
tensors are pure functions of their name, so the weights are those of the relation-aware cases minus the ``*.rela_fuse.*`` tensors, and the
inputs are those of the sibling cases (unet_tiny_*, ti_unet_tiny_*, ip9_unet_tiny_*, plms_tiny) -- the ``relations`` among them are never read.
"""
from __future__ import annotations

import dataclasses

from layoutllm_t2i_amd import host, recipe
from layoutllm_t2i_amd.arch import TINY

import inpaint9_cases as ic

NR_TINY = dataclasses.replace(TINY, relation=False)
NR_TI_TINY = dataclasses.replace(TINY, relation=False, grounding="text_image")
NR_IP_TINY = dataclasses.replace(TINY, relation=False, inpaint_mode=True)
TI_KEYS = ic.TI_KEYS
TEXT_KEYS = ("boxes", "masks", "positive_embeddings")

CASES = [
    dict(name="norel_unet_tiny_cond", kind="unet", family="text", B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    dict(name="norel_unet_tiny_null", kind="unet", family="text", B=2, h=16, w=16, t=[401, 401], grounding="null", scale=1.0, sdconv=False),
    dict(name="norel_unet_tiny_s05", kind="unet", family="text", B=2, h=16, w=16, t=[601, 601], grounding="real", scale=0.5, sdconv=False),
    # fuser skipped: attn1's output goes straight to LayerNorm(norm2) -> attn2
    dict(name="norel_unet_tiny_s0_sd", kind="unet", family="text", B=2, h=16, w=16, t=[21, 21], grounding="real", scale=0.0, sdconv=True),
    # the smallest legal non-square latent of the tiny architecture (three levels: multiples of 8)
    dict(name="norel_unet_tiny_rect", kind="unet", family="text", B=2, h=8, w=16, t=[601, 601], grounding="real", scale=1.0, sdconv=False),
    dict(name="norel_ti_unet_tiny_s1", kind="unet", family="text_image", B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    dict(name="norel_ip9_unet_tiny_s1", kind="unet", family="inpaint", B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    # crosses scale-0 steps (alpha 0 from step 3 on) and the permanent first-conv switch
    dict(name="norel_plms_tiny", kind="plms", family="text", B=2, h=16, w=16, S=10, guidance=7.5, alpha_type=[0.3, 0.0, 0.7]),
]
UNET_CASES = [c for c in CASES if c["kind"] == "unet"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cfg_of(case):
    return {"text": NR_TINY, "text_image": NR_TI_TINY, "inpaint": NR_IP_TINY}[case["family"]]


def grounding_keys(cfg):
    return TI_KEYS if cfg.grounding == "text_image" else TEXT_KEYS


def case_inputs(case):
    """Numpy inputs of a case (weights excluded); an inpaint case carries ``extra`` [B, 5, h, w] (gligen_inference.py:406-407)."""
    h, w = case["h"], case["w"]
    hw = h if h == w else (h, w)
    cfg = cfg_of(case)
    inp = recipe.synth_inputs(cfg, case["B"], hw, n_boxes=5 if case["family"] == "text_image" else 4, n_rel=3, seed=4321)
    if case["family"] == "inpaint":
        mask = host.draw_masks_from_boxes(inp["boxes"], hw).numpy()
        inp["extra"] = ic.make_extra(ic.z0_of(case["name"], h, w), mask)
    return inp
