"""Case table of the RECTANGULAR goldens (h != w), shared by tools/make_rect_goldens.py (reference side, build container only)
and tests/test_rect_host.py / tests/test_gpu_rect.py.  Same convention as tests/golden_cases.py: every case is data, inputs
and weights are recipe tensors (pure functions of name, shape and seed), the fixtures under tests/golden/ hold the
reference's OUTPUTS (plus, for the inpainting case, the mask / x0 / replayed noise the reference sampler was given).

Shapes are (h, w) = (rows, columns).  Every kind comes in an orientation where h < w ("wide") and, for the kinds where a
transposed-shape bug could hide behind one orientation, one where h > w ("tall").
"""
from __future__ import annotations

import numpy as np

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import TINY

import golden_cases as gc

CTX, MO = gc.CTX, gc.MO


def rect_boxes(B: int):
    """Boxes whose x and y extents differ (swapping h and w changes every rectangle), one whose x1 * w clamps to w, one that is
    degenerate at both 8 x 12 and 12 x 8 (x0 and x1 truncate to the same column: the reference `break`s there and drops the
    valid-looking box after it) in sample 0 only; sample 1 keeps all four."""
    boxes = np.zeros((B, MO, 4), np.float32)
    masks = np.zeros((B, MO), np.float32)
    for b in range(B):
        boxes[b, 0] = (0.10, 0.20, 0.70, 0.50)
        boxes[b, 1] = (0.50, 0.10, 1.30, 0.90)                                           # x1 * w > w -> clamped
        boxes[b, 2] = (0.50, 0.20, 0.55, 0.90) if b == 0 else (0.30, 0.25, 0.80, 0.75)   # b = 0: zero width -> break
        boxes[b, 3] = (0.20, 0.50, 0.90, 0.90)
        masks[b, :4] = 1
    return boxes, masks


CASES = [
    dict(name="rela_rect_wide", kind="rela", C=64, heads=4, h=8, w=12, B=2, R=10, n_rel=3),
    dict(name="rela_rect_tall", kind="rela", C=64, heads=4, h=12, w=8, B=2, R=10, n_rel=3),
    dict(name="st_rect", kind="spatial_transformer", C=64, heads=4, h=8, w=12, B=2, scale=1.0, R=10, n_rel=3),
    dict(name="down_rect", kind="down", C=64, h=8, w=12, B=2),
    dict(name="up_rect", kind="up", C=64, h=4, w=6, B=2),
    dict(name="unet_tiny_rect_wide", kind="unet", B=2, h=16, w=24, t=[981, 981], grounding="real", scale=1.0, sdconv=False),
    dict(name="unet_tiny_rect_tall", kind="unet", B=2, h=24, w=16, t=[21, 21], grounding="real", scale=0.0, sdconv=True),
    dict(name="vae_tiny_rect", kind="vae", B=2, h=8, w=12),
    dict(name="vae_enc_tiny_rect", kind="vae_enc", B=2, h=32, w=48),
    dict(name="plms_rect_tiny", kind="plms", B=2, h=16, w=24, S=10, guidance=7.5, alpha_type=[0.3, 0.0, 0.7]),
    dict(name="plms_inpaint_rect_tiny", kind="plms_inpaint", B=2, h=16, w=24, S=10, guidance=7.5, alpha_type=[0.3, 0.0, 0.7]),
]
NAMES = [c["name"] for c in CASES]


def case(name):
    return next(c for c in CASES if c["name"] == name)


def rnd(tag, shape, seed=7):
    return recipe.normal(f"golden.{tag}", tuple(shape), seed)


def case_inputs(c):
    """Numpy inputs of a case (weights excluded)."""
    k, nm = c["kind"], c["name"]
    h, w, B = c["h"], c["w"], c["B"]
    if k in ("rela", "spatial_transformer"):
        C = c["C"]
        boxes, masks = rect_boxes(B)
        rel = np.zeros((B, c["R"], CTX), np.float32)
        rel[:, :c["n_rel"]] = rnd(f"{nm}.rel", (B, c["n_rel"], CTX))
        out = dict(relations=rel, boxes=boxes, masks=masks)
        if k == "rela":
            out["x"] = rnd(f"{nm}.x", (B, h * w, C))
        else:
            out["x"] = rnd(f"{nm}.x", (B, C, h, w))
            out["context"] = rnd(f"{nm}.context", (B, 77, CTX))
            out["objs"] = rnd(f"{nm}.objs", (B, MO, CTX))
        return out
    if k in ("down", "up"):
        return dict(x=rnd(f"{nm}.x", (B, c["C"], h, w)))
    if k in ("unet", "plms", "plms_inpaint"):
        d = recipe.synth_inputs(TINY, B, (h, w), n_boxes=4, n_rel=3, seed=4321)
        if k == "plms_inpaint":
            d["x0"] = (recipe.normal("inpaint.rect.x0", (1, 4, h, w), 5) * np.float32(0.8)).astype(np.float32)
        return d
    if k == "vae":
        return dict(z=rnd(f"{nm}.z", (B, 4, h, w)) * np.float32(0.18215 * 2.0))
    if k == "vae_enc":
        return dict(x=np.clip(recipe.normal("inpaint.rect.enc.x", (B, 3, h, w), 5) * np.float32(0.5), -1, 1).astype(np.float32))
    raise ValueError(k)


def rect_mask_rule(boxes, H: int, W: int):
    """The per-axis rectangle mask, stated independently of host.draw_masks_from_boxes: ones [B, 1, H, W]; per box x0, x1 =
    int(fp32 product with W), y0, y1 = int(fp32 product with H); the python slice [y0:y1, x0:x1] set to 0."""
    boxes = np.asarray(boxes, np.float32)
    out = np.ones((boxes.shape[0], 1, H, W), np.float32)
    for k in range(boxes.shape[0]):
        for i in range(boxes.shape[1]):
            x0 = int(np.float32(boxes[k, i, 0]) * np.float32(W))
            y0 = int(np.float32(boxes[k, i, 1]) * np.float32(H))
            x1 = int(np.float32(boxes[k, i, 2]) * np.float32(W))
            y1 = int(np.float32(boxes[k, i, 3]) * np.float32(H))
            rows = range(H)[y0:y1]
            cols = range(W)[x0:x1]
            for y in rows:
                for x in cols:
                    out[k, 0, y, x] = 0.0
    return out
