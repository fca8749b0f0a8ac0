"""The grounding families, stated once: one ``Family`` record per family and ``family_of(cfg)``, the only place that turns
``(cfg.grounding, cfg.ds_kind)`` into one.  GLIGEN distributes five -- text, text_image, keypoint, the canny / hed / depth / normal maps
("spatial") and the semantic map ("sem", also ``grounding == "spatial"`` in the config) -- so this is a closed table of data and small
functions.  ``interface._run``, the model's conditioning, ``gligen_inference.run`` and ``txt2img.generate`` read it where they used to
compare ``cfg.grounding``; the checkpoint layout (arch.py, weights.py) and the map stages (spatial.py, semantic.py) keep their own arms."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple


@dataclass(frozen=True)
class Family:
    name: str
    label: str                                   # how a refusal names a checkpoint of the family
    keys: Tuple[str, ...]                        # what the grounding input's prepare() returns and the conditioning reads
    batch: Tuple[str, str]                       # interface's batch builder: (one layout repeated, one layout per prompt)
    build: Callable                              # (builder, meta, cfg, clip_model, clip_processor, batch, device): the builder's own call
    condition: Callable                          # (engine, context, relations, grounding, hw): the engine entry of the family
    extra_key: Optional[str] = None              # the key whose tensor also feeds grounding_extra_input ("map" / "sem"); None: no downsampler
    boxes: bool = False                          # grounded on boxes: meta["input_image"] inpainting and the txt2img entry
    images: bool = False                         # takes reference images under meta["images"]
    refuses: Tuple[Tuple[str, str], ...] = ()    # (meta key, why) it refuses by name

    @property
    def clip(self) -> bool:
        """needs the CLIP phrase model: phrases come with boxes"""
        return self.boxes

    @property
    def relation(self) -> bool:
        """relation phrases can apply: the relation chain pools image features over boxes"""
        return self.boxes


def _boxes(eng, ctx, rel, g, hw):
    eng.set_conditioning(ctx, rel, g["boxes"], g["masks"], g["positive_embeddings"], hw)


def _boxes_images(eng, ctx, rel, g, hw):
    eng.set_conditioning(ctx, rel, g["boxes"], g["masks"], g["text_embeddings"], hw, text_masks=g["text_masks"], image_masks=g["image_masks"],
                         image_embeddings=g["image_embeddings"])


def _points(eng, ctx, rel, g, hw):
    eng.set_conditioning_kp(ctx, g["points"], g["masks"], hw)


def _tokens(eng, ctx, rel, g, hw):
    eng.set_conditioning_tokens(ctx, g["tokens"], hw)          # the model's tokenizer has turned the map into tokens (UNetModel.tokens_of)


_BOX_BATCH = dict(batch=("prepare_batch", "prepare_batch_multiple"), boxes=True,
                  build=lambda fn, meta, cfg, clip_model, clip_processor, bs, device: fn(meta, clip_model, clip_processor, bs, device=device))
_MAP_REFUSES = (("images", "it is grounded on a map, not on reference images"), ("input_image", "there is no inpainting form of it"),
                ("locations", "it takes no boxes"))

FAMILIES = {f.name: f for f in (
    Family(name="text", label="text", keys=("boxes", "masks", "positive_embeddings"), condition=_boxes, **_BOX_BATCH),
    Family(name="text_image", label="text_image", keys=("boxes", "masks", "text_masks", "image_masks", "text_embeddings", "image_embeddings"),
           condition=_boxes_images, images=True, **_BOX_BATCH),
    Family(name="keypoint", label="keypoint", keys=("points", "masks"), condition=_points,
           batch=("prepare_batch_kp", "prepare_batch_kp_multiple"),
           build=lambda fn, meta, cfg, clip_model, clip_processor, bs, device: fn(meta, bs, cfg.max_persons, device),
           refuses=(("images", "it is grounded on poses (meta['locations'] = persons of 17 [x, y])"),
                    ("input_image", "the inpainting mask is drawn from boxes, and poses have none"))),
    Family(name="spatial", label="canny / hed / depth / normal", keys=("map", "mask"), extra_key="map", condition=_tokens,
           batch=("prepare_batch_spatial",) * 2, build=lambda fn, meta, cfg, clip_model, clip_processor, bs, device: fn(meta, bs, device),
           refuses=_MAP_REFUSES),
    Family(name="sem", label="semantic-map", keys=("sem", "mask"), extra_key="sem", condition=_tokens,
           batch=("prepare_batch_sem",) * 2,
           build=lambda fn, meta, cfg, clip_model, clip_processor, bs, device: fn(meta, bs, device, cfg.sem_classes), refuses=_MAP_REFUSES),
)}


def family_of(cfg) -> Family:
    """The family of a UNetConfig.  Anything that is no UNetConfig (``None``, a stub without the fields) reads as the defaults, the text
    family: the one place that tolerates it."""
    grounding = getattr(cfg, "grounding", "text")
    return FAMILIES["sem" if grounding == "spatial" and getattr(cfg, "ds_kind", "") == "sem" else grounding]
