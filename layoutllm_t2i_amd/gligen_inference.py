"""Counterpart of ``GLIGEN/gligen_inference.py`` for the text_layout modality.

The reference file is an upstream GLIGEN script that is *stale* relative to the modified UNet (it passes
no ``relations`` and calls ``prepare(batch)`` with one argument, gligen_inference.py:411-424; SURVEY
App-B#9), so only its entry-point name and argument meaning are kept; semantics follow
``GLIGEN/interface.py``:

    run(meta, config, starting_noise=None) -> list[PIL.Image]

``config`` may carry ``height`` / ``width`` (pixels, multiples of 64; default: the 64 x 64 latent, 512 pixels): they size the starting noise when none is passed;
a passed ``starting_noise`` [bs, 4, h, w] decides the shape itself (image = 8h x 8w).

``meta``: ``ckpt`` (path), ``prompt``, ``phrases``, ``locations`` (ltrb, normalised), optional
``alpha_type``, ``save_folder_name``, ``images`` (one reference image or None per box, for a ``*_box_text_image`` checkpoint; with
``text_mask`` / ``image_mask`` / ``projection_matrix`` as in interface.prepare_batch); ``config``: object/dict with ``batch_size``, ``guidance_scale``,
``no_plms`` (must be False), optional ``sampler`` ("plms", the default, "ddim" with ``ddim_eta`` / ``ddim_discretize``, or "dpmpp_2m" with
``dpm_order`` / ``dpm_discretize``: sampler.SAMPLER_KEYS, checked by sampler.resolve_sampler),
optional ``negative_prompt`` (a string encoded for the unconditional pass, gligen_inference.py:379-380; default
None = the empty prompt), optional ``folder``.  Images are saved like the reference does
(gligen_inference.py:437-446) when ``config.folder`` is given.

``meta["input_image"]`` (a path or a PIL.Image) inpaints that image inside the layout boxes (gligen_inference.py:393-407): it is
encoded by the checkpoint's VAE encoder, the mask is 0 inside the boxes, and the PLMS sampler replaces the known region of the
latent at every step.  The reference asserts a 9-channel ``inpaint_mode`` checkpoint at this point (:398).  Such a checkpoint
(``checkpoint_inpainting_text.pth`` / ``checkpoint_inpainting_text_image.pth``: ``inpaint_mode: True``, first conv ``[320, 9, 3, 3]``) loads
here and additionally feeds ``cat([z0 * mask, mask])`` to the first conv on every forward (:406-407, openaimodel.py:436-439); it needs
``meta["input_image"]`` (ValueError otherwise).  A 4-channel text_layout / text_image checkpoint with ``input_image`` keeps running the
latent-blend inpainting alone, which the reference refuses.

``config["init_image"]`` (a path or a PIL.Image; ``meta["init_image"]`` is read as well) with ``config["strength"]`` in (0, 1] (0.75 when absent):
image-to-image (SDEdit, arXiv 2108.01073; not in the reference's script).  The image is encoded like ``input_image``, noised to the timestep where
the last int(strength * n) of the schedule's n nodes begin, and re-rendered from there under the prompt and the boxes; every checkpoint family
and sampler, with or without ``input_image``.  ``strength`` without an image raises ValueError.

A keypoint checkpoint (``checkpoint_generation_keypoint.pth``, ``keypoint_grounding_net.PositionNet``) takes ``meta["locations"]`` as a
list of persons, each a list of 17 ``[x, y]`` in [0, 1] with ``[0, 0]`` for a missing keypoint (gligen_inference.py:199-218, :585-633); it
needs neither ``phrases`` nor a CLIP model, and ``images`` / ``input_image`` raise ValueError.

A spatial checkpoint (``checkpoint_generation_canny.pth`` / ``_hed`` / ``_depth`` / ``_normal``) takes its map under the reference's own meta
key (``canny_image`` / ``hed_image`` / ``depth`` / ``normal``: a path or a ``PIL.Image``); it needs neither ``locations`` nor ``phrases`` nor a
CLIP model, and ``images`` / ``input_image`` / boxes raise ValueError.  The semantic-map checkpoint (``checkpoint_generation_sem.pth``) takes
an image of class ids under ``meta["sem"]`` in the same way.

A checkpoint without ``rela_fuse`` tensors (every public GLIGEN checkpoint) runs on the upstream transformer block it was trained with
(attention_original.py:312-316): no relation phrases are parsed or encoded for it.
"""
from __future__ import annotations

import os

import torch

from . import interface
from .family import family_of
from .sampler import SAMPLER_KEYS

_MODELS = {}


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


@torch.no_grad()
def run(meta, config, starting_noise=None, clip_model=None, clip_processor=None):
    """``clip_model`` / ``clip_processor``: the HF CLIP objects the reference creates inline (gligen_inference.py:96-98,
    ``openai/clip-vit-large-patch14``); pass them in to run offline -- they are only downloaded when omitted."""
    device = _get(config, "device", "cuda")
    ckpt = meta["ckpt"]
    if ckpt not in _MODELS:
        _MODELS[ckpt] = interface.load_all_models(ckpt, device)
    all_models = _MODELS[ckpt]
    # The reference reloads the checkpoint on every run() (gligen_inference.py:346), so each run starts from the GLIGEN
    # first conv; the cached model here must be put back (restore_first_conv_from_SD is permanent, openaimodel.py:393-411).
    all_models[0].first_conv_type = "GLIGEN"
    bs = _get(config, "batch_size", 1)
    args = dict(batch_size=bs, no_plms=bool(_get(config, "no_plms", False)), guidance_scale=_get(config, "guidance_scale", 7.5))
    if _get(config, "negative_prompt") is not None:      # gligen_inference.py:379-380; absent / None = the empty prompt
        args["negative_prompt"] = _get(config, "negative_prompt")
    # the reference routes on the checkpoint's file name (gligen_inference.py:363-372); here the loaded model's family decides.  A map family
    # (canny / hed / depth / normal, sem) is grounded on one map under the reference's own meta key: no locations, no phrases
    fam = family_of(getattr(all_models[0], "cfg", None))
    m = dict(prompt=meta["prompt"], phrases=meta.get("phrases"), locations=meta.get("locations") if fam.extra_key else meta["locations"],
             alpha_type=meta.get("alpha_type", [0.3, 0.0, 0.7]), input_image=meta.get("input_image"))
    for k in interface.SPATIAL_META_KEYS + (interface.SEM_META_KEY,):
        if meta.get(k) is not None:
            m[k] = meta[k]
    # image grounding (a *_box_text_image checkpoint, gligen_inference.py:350-352): one reference image or None per box
    for k in ("images", "text_mask", "image_mask", "projection_matrix"):
        if meta.get(k) is not None:
            m[k] = meta[k]
    init_image = _get(config, interface.INIT_IMAGE_KEY)
    init_image = meta.get(interface.INIT_IMAGE_KEY) if init_image is None else init_image
    if init_image is not None:
        m[interface.INIT_IMAGE_KEY] = init_image
    if starting_noise is None:
        h, w = interface.latent_hw(_get(config, "height"), _get(config, "width"), all_models[1])
        starting_noise = torch.randn(bs, 4, h, w).to(device)
    # (a keypoint checkpoint is grounded on meta["locations"] = persons of 17 [x, y] alone: no phrases, and no CLIP model to create)
    if fam.clip and (clip_model is None or clip_processor is None):
        from transformers import CLIPModel, CLIPProcessor
        version = "openai/clip-vit-large-patch14"
        clip_model = CLIPModel.from_pretrained(version).to(device)
        clip_processor = CLIPProcessor.from_pretrained(version)
    # per-call keys, handed on only when the config carries them: the step count, the sampler switch (sampler.resolve_sampler), the
    # layout's guidance scale (interface.check_layout_guidance) and image-to-image's strength (interface.check_strength)
    for k in ("steps",) + SAMPLER_KEYS + (interface.LAYOUT_GUIDANCE_KEY, interface.STRENGTH_KEY):
        if k in (config if isinstance(config, dict) else vars(config)):
            args[k] = _get(config, k)
    images = interface.run_one_image(all_models, args, m, starting_noise, clip_model, clip_processor, device=device)
    folder = _get(config, "folder")
    if folder:
        out = os.path.join(folder, meta.get("save_folder_name", "out"))
        os.makedirs(out, exist_ok=True)
        start = len(os.listdir(out))
        for i, im in enumerate(images):
            im.save(os.path.join(out, f"{start + i}.png"))
    return images
