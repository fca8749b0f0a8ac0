"""Golden-vector case table of the keypoint grounding family (``checkpoint_generation_keypoint.pth``, ``keypoint_grounding_net.PositionNet``:
17 grounding tokens per person from 2-D points, a learned person table and a learned keypoint table).  Shared by tools/make_kp_goldens.py
(reference side, build container only) and tests/test_kp_host.py / tests/test_gpu_kp.py.

Like tests/norel_cases.py every case is data; inputs and weights are recipe tensors, the fixtures hold the reference's OUTPUTS only.  The UNet
is the upstream one (``relation=False``: attn1 -> fuser -> attn2 -> ff), the only block the family runs on.
"""
from __future__ import annotations

import dataclasses

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import TINY, UNetConfig

KP_TARGET = "ldm.modules.diffusionmodules.keypoint_grounding_net.PositionNet"
KEYS = ("points", "masks")


def kp_cfg(base: UNetConfig, P: int) -> UNetConfig:
    """``base`` as a keypoint config of P persons: 17 P tokens, person features as wide as the tokens"""
    return dataclasses.replace(base, relation=False, grounding="keypoint", max_objs=17 * P, pos_in_dim=base.pos_out_dim)


KP_TINY = {P: kp_cfg(TINY, P) for P in (1, 3, 8)}
FULL = {P: kp_cfg(UNetConfig(), P) for P in (3, 8)}        # the PositionNet alone at the shipped width (D = 768, K = 800)

CASES = [
    dict(name="kp_posnet_p3", kind="position_net", P=3, B=2),
    dict(name="kp_posnet_p8", kind="position_net", P=8, B=2),
    dict(name="kp_unet_tiny_p3_s1", kind="unet", P=3, B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    dict(name="kp_unet_tiny_p3_s03", kind="unet", P=3, B=2, h=16, w=16, t=[601, 601], grounding="real", scale=0.3, sdconv=False),
    dict(name="kp_unet_tiny_p3_s0_sd", kind="unet", P=3, B=2, h=16, w=16, t=[21, 21], grounding="real", scale=0.0, sdconv=True),
    dict(name="kp_unet_tiny_p8_s1", kind="unet", P=8, B=2, h=16, w=16, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    dict(name="kp_unet_tiny_p8_s03", kind="unet", P=8, B=2, h=16, w=16, t=[601, 601], grounding="real", scale=0.3, sdconv=False),
    dict(name="kp_unet_tiny_p8_s0_sd", kind="unet", P=8, B=2, h=16, w=16, t=[21, 21], grounding="real", scale=0.0, sdconv=True),
    dict(name="kp_unet_tiny_rect", kind="unet", P=8, B=2, h=16, w=24, t=[601, 601], grounding="real", scale=1.0, sdconv=False),
    # null grounding alone (zero points, zero masks: every token is MLP(null features)), on the conditional context and timestep of p8_s1
    dict(name="kp_unet_tiny_null", kind="unet", P=8, B=2, h=16, w=16, t=[981, 981], grounding="null", scale=1.0, sdconv=False),
    # the names and shapes of the reference model's state dict, in registration order (P = 3, tiny)
    dict(name="kp_params", kind="params", P=3),
    # the reference's own two-person meta through its own prepare_batch_kp (gligen_inference.py:199-218, :585-633)
    dict(name="kp_prepare_batch", kind="prepare_batch", P=8, B=2),
]
UNET_CASES = [c for c in CASES if c["kind"] == "unet"]
POSNET_CASES = [c for c in CASES if c["kind"] == "position_net"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cfg_of(case):
    return FULL[case["P"]] if case["kind"] == "position_net" else KP_TINY[case["P"]]


def case_inputs(case):
    """Numpy inputs of a case (weights excluded): x, context, uc, points [B, 17 P, 2], masks [B, 17 P] with missing keypoints, an absent last
    person and one fractional mask (recipe.synth_inputs_kp)."""
    h, w = case.get("h", 16), case.get("w", 16)
    return recipe.synth_inputs_kp(cfg_of(case), case["B"], (h, w), seed=4321)
