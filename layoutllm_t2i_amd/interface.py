"""Drop-in counterpart of ``GLIGEN/interface.py``: same function names, signatures, argument meaning
and quirks, with the denoiser (UNet + PLMS) running on the MI355X HIP engine.

    load_all_models(ckpt, device)                     interface.py:366-373
    load_ckpt(ckpt_path, device)                      interface.py:78-101
    generate_batch_images(all_models, captions, labels, bboxes, clip_model, clip_processor, device)  :551-570
    generate_one_image(all_models, caption, label, bbox, clip_model, clip_processor, device)          :376-395
    run_batch_images / run_one_image(all_models, args, meta, starting_noise, clip_model, clip_processor, device)
    set_alpha_scale, alpha_generator, prepare_batch, prepare_batch_multiple, prepare_relation_phrases,
    convert_xywh_to_ltrb, convert_xcycwh_to_ltrb

``all_models`` stays the reference's 5-tuple ``(model, autoencoder, text_encoder, diffusion, config)``.
``model`` is this package's UNetModel; ``autoencoder`` / ``text_encoder`` are whatever the caller
provides with the reference's ``decode(z)`` / ``encode(list[str], return_pooler_output=...)`` methods
(the reference's own CPU modules work unchanged -- VAE and CLIP are SURVEY 8f "next" rows, and the
LLM / policy orchestration stays on the reference path by design).

Preserved behaviour: alpha_type [0.3, 0, 0.7]; 50 PLMS steps; CFG 7.5; noise from the
global CPU RNG ``torch.randn(bs, 4, 64, 64)``; ``generate_batch_images`` passes boxes through
UNconverted while ``generate_one_image`` converts xywh -> ltrb; ``config.update(args)`` mutates the
caller's dict; relation phrases are "PAD" + every relation twice, truncated to max_relations;
clamp -> *0.5+0.5 -> *255 -> astype(uint8) truncation.
"""
from __future__ import annotations

import math
import os
import warnings
from functools import partial
from typing import Union

import numpy as np
import torch

from . import host
from .arch import UNetConfig
from .arch import VAEConfig
from .family import family_of
from .model import LatentDiffusion, UNetModel, grounding_input_for, load_sd_first_conv
from .vae import VAEDecoder
from .sampler import SAMPLERS, DDIMSampler, DPMSolverSampler, PLMSSampler, resolve_sampler  # noqa: F401  (the classes: part of the surface)

MAX_OBJS = 30
PLMS_STEPS = 50
# SAMPLERS (above): ("plms", "ddim", "dpmpp_2m"), the values of args["sampler"] out of sampler.SAMPLER_TABLE; "plms" is the default


def set_alpha_scale(model, alpha_scale):
    """interface.py:34-38: only the gated self-attention fuser is scaled; rela_fuse.scale stays 1."""
    model.fuser_scale = alpha_scale


alpha_generator = host.alpha_generator


class _AttrDict(dict):
    """Enough of OmegaConf.create(dict) for run_*_images: attribute access on a dict."""
    __getattr__ = dict.__getitem__


def _instantiate_reference(config_node):
    """instantiate_from_config (ldm/util.py:71-85) for the non-hot-path modules (VAE, CLIP text encoder):
    resolved from whatever ``ldm`` package is importable (the reference's, on its CPU path)."""
    import importlib
    module, cls = config_node["target"].rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)(**config_node.get("params", dict()))


def _load_text_encoder(node, state_dict, device):
    """The conditioning encoder (interface.py:85-88).  A checkpoint whose ``text_encoder`` entry holds a CLIP text tower
    (``FrozenCLIPEmbedder.state_dict()``: ``transformer.text_model.*``) runs on the HIP kernels (text_encoder.HipCLIPTextEncoder,
    SURVEY 8f-2); its tokenizer is the config's ``params.tokenizer`` node when present, else HuggingFace's CLIPTokenizer of
    ``params.version`` exactly as FrozenCLIPEmbedder loads it (encoders/modules.py:148).  Anything else -- or
    GLIGEN_REFERENCE_TEXT_ENCODER=1 -- is instantiated from whatever ``ldm`` package is importable, like the reference does."""
    from .text_encoder import HipCLIPTextEncoder
    params = node.get("params", {}) or {}
    if not os.environ.get("GLIGEN_REFERENCE_TEXT_ENCODER") and HipCLIPTextEncoder.accepts(state_dict):
        if params.get("tokenizer") is not None:
            tokenizer = _instantiate_reference(params["tokenizer"])
        else:
            from transformers import CLIPTokenizer
            tokenizer = CLIPTokenizer.from_pretrained(params.get("version", "openai/clip-vit-large-patch14"))
        return HipCLIPTextEncoder(state_dict, tokenizer, device, heads=params.get("num_attention_heads"), max_length=params.get("max_length", 77))
    text_encoder = _instantiate_reference(node).to(device).eval()
    text_encoder.load_state_dict(state_dict)
    return text_encoder


def hip_phrase_encoder(clip_model, device, heads=None):
    """The ``clip_model`` argument of generate_batch_images / generate_one_image (a HuggingFace ``CLIPModel``, used only for the
    grounding phrases' ``text_model_output.pooler_output``, interface.py:114-141) moved onto the HIP text tower: pass the result
    as ``clip_model`` instead; ``clip_processor`` keeps tokenising.  ``heads`` defaults to hidden / 64."""
    from .text_encoder import HipCLIPTextEncoder
    sd = clip_model if isinstance(clip_model, dict) else clip_model.state_dict()
    if heads is None and hasattr(clip_model, "config"):
        heads = getattr(getattr(clip_model.config, "text_config", None), "num_attention_heads", None)
    return HipCLIPTextEncoder(sd, None, device, heads=heads)


def find_sd_first_conv(ckpt_path=None):
    """Locates ``SD_input_conv_weight_bias.pth``.  The reference reads it from the GLIGEN code directory on every
    scale-0 step (openaimodel.py:396-398) and fails hard when it is missing.  Search order: $GLIGEN_SD_FIRST_CONV,
    next to the checkpoint, $GLIGEN_HOME, and the directory the reference itself computes -- four levels above
    ``ldm/modules/diffusionmodules/openaimodel.py`` of whatever ``ldm`` package is importable.  Returns None if absent."""
    name = "SD_input_conv_weight_bias.pth"
    cands = []
    if os.environ.get("GLIGEN_SD_FIRST_CONV"):
        cands.append(os.environ["GLIGEN_SD_FIRST_CONV"])
    if ckpt_path is not None:
        cands.append(os.path.join(os.path.dirname(os.path.abspath(ckpt_path)), name))
    if os.environ.get("GLIGEN_HOME"):
        cands.append(os.path.join(os.environ["GLIGEN_HOME"], name))
    try:
        import importlib.util
        spec = importlib.util.find_spec("ldm")
        if spec is not None and spec.submodule_search_locations:
            cands.append(os.path.join(os.path.dirname(list(spec.submodule_search_locations)[0]), name))
    except (ImportError, ValueError):
        pass
    for c in cands:
        if os.path.exists(c):
            return c
    return None


def checkpoint_has_relation(state_dict, cfg) -> bool:
    """Which transformer block a checkpoint's UNet was trained on, read off its keys: no ``*.rela_fuse.*`` tensor at all = upstream GLIGEN's
    block (attention_original.py:312-316; every public GLIGEN checkpoint) -> False; all of them = LayoutLLM-T2I's (attention.py:394-402) ->
    True.  Some but not all is a damaged checkpoint: KeyError naming a missing tensor, what packing it raises."""
    import dataclasses
    from .arch import param_shapes
    if not any(".rela_fuse." in k for k in state_dict):
        return False
    missing = [k for k in param_shapes(dataclasses.replace(cfg, relation=True)) if ".rela_fuse." in k and k not in state_dict]
    if missing:
        raise KeyError(f"state_dict is missing {len(missing)} tensors, e.g. {missing[:3]}")
    return True


def load_ckpt(ckpt_path, device="cuda", strict=None):
    """interface.py:78-101.  The UNet ('model') is built by this package from saved_ckpt['model'];
    autoencoder / text_encoder / grounding tokenizer are instantiated from the checkpoint's config.

    ``strict`` (default: the environment variable ``GLIGEN_STRICT=1``): pack the UNet's weights in the split layout ([Whi | Wlo] for
    every matrix, twice the bytes) and run the engine in STRICT mode (gl_set_handle_option 50: split-fp16 operands for every matrix
    product): the UNet output is then within rtol 1e-3 / atol 1e-4 of the fp32 reference (measured rel-L2 < 1e-5) at ~0.47 x the default
    mode's images/s.  ``model.set_strict(False)`` switches the same handle back to the default (fast) arithmetic.

    Like the reference (openaimodel.py:393-405) the SD first-conv file is needed as soon as a fuser-scale-0 step runs:
    a missing file warns here and raises in ``restore_first_conv_from_SD`` (where the reference fails), never silently
    keeps the GLIGEN conv.  ``GLIGEN_ALLOW_NO_SD_CONV=1`` opts out explicitly (first_conv_restorable = False)."""
    saved_ckpt = torch.load(ckpt_path, map_location="cpu")
    config = saved_ckpt["config_dict"]["_content"]
    # every family loads (family.py): _run builds the batch and the extras each needs; the family is read off the config, not off the file name,
    # and a map family's ConvNeXt tokenizer and grounding downsampler are built from the checkpoint's own tensors -- nothing is fetched
    cfg = UNetConfig.from_dict(config["model"]["params"], allow_inpaint=True, allow_keypoint=True, allow_spatial=True, allow_semantic=True)
    import dataclasses
    fam = family_of(cfg)
    if not fam.relation and any(".rela_fuse." in k for k in saved_ckpt["model"]):
        raise NotImplementedError(f"a {cfg.grounding} checkpoint with *.rela_fuse.* tensors: the relation chain pools image features over grounding "
                                  f"boxes, and a {cfg.grounding} model has none (it runs on the upstream block only)")
    if fam.extra_key is not None:
        # the ConvNeXt's depths and widths are the checkpoint's own (its config does not state them; the shipped ones are convnext_tiny's)
        from .spatial import backbone_of
        depths, dims = backbone_of(saved_ckpt["model"])
        cfg = dataclasses.replace(cfg, convnext_depths=depths, convnext_dims=dims)
    # a checkpoint without rela_fuse tensors (GLIGEN's own) runs on the upstream block, not on a default-initialised relation chain
    cfg = dataclasses.replace(cfg, relation=checkpoint_has_relation(saved_ckpt["model"], cfg))
    if strict is None:
        strict = os.environ.get("GLIGEN_STRICT") == "1"
    if strict and fam.extra_key is not None:
        raise NotImplementedError("strict mode (strict=True / GLIGEN_STRICT=1) of a spatial checkpoint: the ConvNeXt tokenizer has no split-fp16 "
                                  "form; load it in the default mode")
    if strict:
        cfg = dataclasses.replace(cfg, split_weights=True)
    # (an inpaint_mode checkpoint's 9-channel first conv is not restorable, openaimodel.py:296: the SD conv file is neither looked for nor missed)
    sd_path = None if cfg.inpaint_mode else find_sd_first_conv(ckpt_path)
    allow_missing = os.environ.get("GLIGEN_ALLOW_NO_SD_CONV") == "1"
    if sd_path is None and not allow_missing and not cfg.inpaint_mode:
        warnings.warn(
            "SD_input_conv_weight_bias.pth not found (looked at $GLIGEN_SD_FIRST_CONV, next to the checkpoint, $GLIGEN_HOME and "
            "the importable ldm package's GLIGEN directory): the first fuser-scale-0 step will raise, exactly where the reference "
            "fails (openaimodel.py:393-405); schedules without a scale-0 stage run.  GLIGEN_ALLOW_NO_SD_CONV=1 keeps the GLIGEN conv "
            "instead (results then differ from the reference).")
    model = UNetModel(cfg, saved_ckpt["model"], device=device, sd_first_conv=load_sd_first_conv(sd_path),
                      allow_missing_sd_conv=sd_path is None and allow_missing and not cfg.inpaint_mode)
    if strict:
        model.set_strict(True)
    dparams = config["diffusion"].get("params", {})
    diffusion = LatentDiffusion(linear_start=dparams.get("linear_start", 0.00085), linear_end=dparams.get("linear_end", 0.012),
                                timesteps=dparams.get("timesteps", 1000), device=device)
    if os.environ.get("GLIGEN_REFERENCE_VAE"):
        autoencoder = _instantiate_reference(config["autoencoder"]).to(device).eval()
        autoencoder.load_state_dict(saved_ckpt["autoencoder"])
    else:
        # decode stage on the HIP kernels, plus `.encode(x)` for inpainting when the checkpoint holds the encoder
        ap = config["autoencoder"].get("params", {})
        dd = ap.get("ddconfig", {})
        vcfg = VAEConfig(ch=dd.get("ch", 128), ch_mult=tuple(dd.get("ch_mult", (1, 2, 4, 4))),
                         num_res_blocks=dd.get("num_res_blocks", 2), z_channels=dd.get("z_channels", 4),
                         out_ch=dd.get("out_ch", 3), embed_dim=ap.get("embed_dim", 4), scale_factor=ap.get("scale_factor", 0.18215))
        autoencoder = VAEDecoder(saved_ckpt["autoencoder"], vcfg, device)
    text_encoder = _load_text_encoder(config["text_encoder"], saved_ckpt["text_encoder"], device)
    for m in (autoencoder, text_encoder):
        # (reference modules keep the device string they .to()'d; the HIP stages own a resolved torch.device and keep it)
        if not isinstance(m, VAEDecoder) and not _is_hip_encoder(m) and "device" in vars(m):
            m.device = device
    return model, autoencoder, text_encoder, diffusion, config


def load_all_models(ckpt, device, strict=None):
    """interface.py:366-373 (``strict``: see load_ckpt)."""
    model, autoencoder, text_encoder, diffusion, config = load_ckpt(ckpt, device, strict=strict)
    model.grounding_tokenizer_input = grounding_input_for(model.cfg)      # text, text_image (*_box_text_image) or keypoint
    return model, autoencoder, text_encoder, diffusion, config


def convert_xcycwh_to_ltrb(bbox):
    xc, yc, w, h = bbox
    return [xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2]


def convert_xywh_to_ltrb(bbox):
    x1, y1, w, h = bbox
    return [x1, y1, x1 + w, y1 + h]


def complete_mask(has_mask, max_objs):
    mask = torch.ones(1, max_objs)
    if has_mask is None:
        return mask
    if type(has_mask) == int or type(has_mask) == float:
        return mask * has_mask
    for idx, value in enumerate(has_mask):
        mask[0, idx] = value
    return mask


def _hf_text_pooler_output(model, input_ids, attention_mask, device):
    """``outputs.text_model_output.pooler_output`` of interface.py:136-139 under the reference's pinned transformers 4.19.2: the
    text tower's pooled hidden state BEFORE ``text_projection`` (``which_layer_text = 'before'``, :115).  transformers 5.x
    overwrites that field with the PROJECTED feature inside ``CLIPModel.forward``; calling the text tower itself gives the
    4.19.2 value under every version (and skips the placeholder vision pass)."""
    if hasattr(model, "text_model"):
        return model.text_model(input_ids=input_ids, attention_mask=attention_mask).pooler_output
    return model(input_ids=input_ids, attention_mask=attention_mask, pixel_values=torch.ones(1, 3, 224, 224).to(device)).text_model_output.pooler_output


IMAGE_FEATURE_NORM = 28.7          # interface.py:129
_PROJECTION_CACHE = {}


def load_projection_matrix(meta=None, device=None) -> torch.Tensor:
    """The CLIP projection matrix of interface.py:128 (``torch.load('projection_matrix')``), fp32 on ``device``.  Looked up in
    ``meta["projection_matrix"]`` (a tensor or a path), then ``$GLIGEN_PROJECTION_MATRIX``, then a file ``projection_matrix`` in the working
    directory (where the reference reads it); a file is loaded once per (path, device) and cached.  FileNotFoundError names all three."""
    src = (meta or {}).get("projection_matrix") if hasattr(meta, "get") else None
    if torch.is_tensor(src):
        return src.detach().to(device, torch.float32).contiguous()
    cands = [src, os.environ.get("GLIGEN_PROJECTION_MATRIX"), os.path.join(os.getcwd(), "projection_matrix")]
    for c in cands:
        if c and os.path.exists(c):
            key = (os.path.abspath(c), str(device))
            if key not in _PROJECTION_CACHE:
                _PROJECTION_CACHE[key] = torch.load(c, map_location="cpu").detach().to(device, torch.float32).contiguous()
            return _PROJECTION_CACHE[key]
    raise FileNotFoundError("image grounding needs CLIP's projection matrix (interface.py:128); looked at meta['projection_matrix'] "
                            f"({src!r}), $GLIGEN_PROJECTION_MATRIX ({os.environ.get('GLIGEN_PROJECTION_MATRIX')!r}) and "
                            f"{os.path.join(os.getcwd(), 'projection_matrix')!r}")


def _clip_image_embeds(model, pixel_values, device):
    """the CLIP image embedding (``outputs.image_embeds`` of interface.py:125-126) from a HuggingFace ``CLIPModel`` or anything with
    ``get_image_features`` (clip.ClipTowers)"""
    if not hasattr(model, "get_image_features"):
        raise TypeError("image grounding needs a CLIP model with get_image_features (a HuggingFace CLIPModel or clip.ClipTowers)")
    px = torch.as_tensor(np.asarray(pixel_values) if not torch.is_tensor(pixel_values) else pixel_values)
    out = model.get_image_features(pixel_values=px.to(device))
    if not torch.is_tensor(out):           # newer transformers return an output object
        out = out.pooler_output if getattr(out, "pooler_output", None) is not None else out[0]
    return out


def get_clip_feature(model, processor, input, device, is_image=False, projection_matrix=None):
    """interface.py:114-141.  Text: the 'before' projection feature (pooler_output).  Image ('after_reproject', :118-130): ``input`` is a
    path or a ``PIL.Image``; ``.convert("RGB")``, the caller's ``processor(images=[image])``, the CLIP image embedding of the caller's
    model, then ``28.7 * (f @ P) / ||f @ P||`` on the device (gl_image_ground_feature).  ``projection_matrix``: a tensor, a ``meta``
    dict, or None (see load_projection_matrix)."""
    if input is None:
        return None
    if is_image:
        from PIL import Image
        from . import ops
        image = (input if isinstance(input, Image.Image) else Image.open(input)).convert("RGB")
        P = projection_matrix if torch.is_tensor(projection_matrix) else load_projection_matrix(projection_matrix, device)
        inputs = processor(images=[image], return_tensors="pt", padding=True)
        feat = _clip_image_embeds(model, inputs["pixel_values"], device).detach().to(device, torch.float32).reshape(1, -1).contiguous()
        return ops.image_ground_feature(feat, P.to(device, torch.float32).contiguous(), IMAGE_FEATURE_NORM)
    inputs = processor(text=input, return_tensors="pt", padding=True)
    return _hf_text_pooler_output(model, inputs["input_ids"].to(device), inputs["attention_mask"].to(device), device)


def get_clip_features_batched(model, processor, phrases, device):
    """Conditioning-prep batching.  The reference calls ``get_clip_feature`` once per phrase,
    sequentially (interface.py:446-448: B x n_boxes CLIP forwards, each also running the vision tower on a
    placeholder image).  Here every DISTINCT phrase of the whole batch goes through ONE padded forward; CLIP's
    text tower is causal and the pooled feature is read at the EOS position, so padding after EOS cannot change
    it (checked against the per-phrase path in tests/test_host_cpu.py).  Returns {phrase: [1, 768] feature}."""
    uniq = [p for p in dict.fromkeys(phrases) if p is not None]
    if not uniq:
        return {}
    inputs = processor(text=uniq, return_tensors="pt", padding=True)
    if hasattr(model, "pooler_output") and callable(model.pooler_output):
        # the HIP text tower (hip_phrase_encoder / text_encoder.HipCLIPTextEncoder): token rows in, pooled rows out; no vision pass
        pooled = model.pooler_output(inputs["input_ids"])
        return {p: pooled[i:i + 1] for i, p in enumerate(uniq)}
    pooled = _hf_text_pooler_output(model, inputs["input_ids"].to(device), inputs["attention_mask"].to(device), device)
    return {p: pooled[i:i + 1] for i, p in enumerate(uniq)}


def _image_key(im):
    return im if isinstance(im, (str, os.PathLike)) else id(im)


def get_image_features_cached(model, processor, images, device, meta=None, cache=None):
    """{id of the image object or its path: [1, 768] grounding feature} for the DISTINCT non-None entries of ``images`` (the reference
    encodes every box's image separately, interface.py:172-174).  The projection matrix is resolved only when there is an image."""
    cache = {} if cache is None else cache
    P = None
    for im in images:
        if im is None:
            continue
        k = _image_key(im)
        if k not in cache:
            if P is None:
                P = load_projection_matrix(meta, device)
            cache[k] = get_clip_feature(model, processor, im, device, is_image=True, projection_matrix=P)
    return cache


def _one_sample_grounding(phrases, locations, model, processor, max_objs, device, feature_cache=None, images=None, image_cache=None):
    boxes = torch.zeros(max_objs, 4)
    masks = torch.zeros(max_objs)
    text_masks = torch.zeros(max_objs)
    image_masks = torch.zeros(max_objs)
    text_embeddings = torch.zeros(max_objs, 768)
    image_embeddings = torch.zeros(max_objs, 768)
    if phrases is None:
        phrases = [None] * len(locations)           # interface.py:166: zero embeddings, boxes still grounded
    if feature_cache is None:
        feature_cache = get_clip_features_batched(model, processor, phrases, device)
    feats = [None if ph is None else feature_cache[ph] for ph in phrases]
    if images is None:
        images = [None] * len(locations)
    elif len(images) != len(locations):        # (without images the text path keeps zip's silent truncation, like the reference)
        raise ValueError(f"{len(locations)} boxes with {len(images)} images: one entry (or None) per box")
    ifeats = [None if im is None else image_cache[_image_key(im)] for im in images]
    for idx, (box, feat, ifeat) in enumerate(zip(locations, feats, ifeats)):
        boxes[idx] = torch.tensor(box)
        masks[idx] = 1
        if feat is not None:
            text_embeddings[idx] = feat
            text_masks[idx] = 1
        if ifeat is not None:
            image_embeddings[idx] = ifeat.detach().float().cpu()
            image_masks[idx] = 1
    return boxes, masks, text_masks, image_masks, text_embeddings, image_embeddings


@torch.no_grad()
def prepare_batch(meta, model, processor, batch=1, max_objs=MAX_OBJS, device=None):
    """interface.py:156-193: one layout repeated `batch` times.  ``meta["images"]``: one reference image (path / PIL.Image) or None per
    box; ``phrases=None`` with images grounds on the images alone."""
    images = meta.get("images")
    icache = get_image_features_cached(model, processor, images, device, meta) if images is not None else None
    boxes, masks, tm, im, te, ie = _one_sample_grounding(meta.get("phrases"), meta["locations"], model, processor, max_objs, device,
                                                         images=images, image_cache=icache)
    out = {
        "boxes": boxes.unsqueeze(0).repeat(batch, 1, 1),
        "masks": masks.unsqueeze(0).repeat(batch, 1),
        "text_masks": tm.unsqueeze(0).repeat(batch, 1) * complete_mask(meta.get("text_mask"), max_objs),
        "image_masks": im.unsqueeze(0).repeat(batch, 1) * complete_mask(meta.get("image_mask"), max_objs),
        "text_embeddings": te.unsqueeze(0).repeat(batch, 1, 1),
        "image_embeddings": ie.unsqueeze(0).repeat(batch, 1, 1),
    }
    return {k: v.to(device) for k, v in out.items()}


@torch.no_grad()
def prepare_batch_kp(meta, batch=1, max_persons=8, device=None):
    """gligen_inference.py:199-218: ``meta["locations"]`` is a list of persons, each a list of 17 ``[x, y]`` in [0, 1] (a missing keypoint is
    ``[0, 0]``); one pose layout repeated ``batch`` times.  Returns ``points`` [batch, 17 * max_persons, 2] and ``masks`` [batch, 17 * max_persons]
    = ``points.mean(dim=1) != 0``, as the reference derives them.  More than ``max_persons`` persons (the reference runs off the end of its
    tensor) and a person without exactly 17 points (the reference would misalign every later person) raise ValueError."""
    points, masks = _one_sample_pose(meta["locations"], max_persons)
    out = {"points": points.unsqueeze(0).repeat(batch, 1, 1), "masks": masks.unsqueeze(0).repeat(batch, 1)}
    return {k: v.to(device) for k, v in out.items()} if device is not None else out


def _one_sample_pose(persons, max_persons):
    if len(persons) > max_persons:
        raise ValueError(f"{len(persons)} persons, the checkpoint was built for at most {max_persons} (max_persons_per_image)")
    points = torch.zeros(max_persons * 17, 2)
    for p, kps in enumerate(persons):
        if len(kps) != 17 or any(len(kp) != 2 for kp in kps):
            raise ValueError(f"person {p} has {len(kps)} keypoints: each person is a list of 17 [x, y] pairs ([0, 0] = missing)")
        points[17 * p:17 * (p + 1)] = torch.tensor(kps, dtype=torch.float32)
    masks = ((points.mean(dim=1) != 0) * 1).float()
    return points, masks


@torch.no_grad()
def prepare_batch_kp_multiple(meta, batch, max_persons=8, device=None):
    """``prepare_batch_kp`` with one pose layout per prompt: ``meta["locations"][i]`` is prompt i's list of persons."""
    if len(meta["locations"]) != batch:
        raise ValueError(f"locations: {len(meta['locations'])} pose layouts for a batch of {batch}")
    parts = [_one_sample_pose(persons, max_persons) for persons in meta["locations"]]
    out = {"points": torch.stack([p for p, _ in parts], 0), "masks": torch.stack([m for _, m in parts], 0)}
    return {k: v.to(device) for k, v in out.items()} if device is not None else out


SPATIAL_META_KEYS = ("canny_image", "hed_image", "depth", "normal")       # the reference's own meta keys (gligen_inference.py:226-289)


def _spatial_map_of(meta):
    """the one map a meta dict carries under the reference's keys, or None"""
    given = [k for k in SPATIAL_META_KEYS if meta.get(k) is not None]
    if len(given) > 1:
        raise ValueError(f"meta carries more than one grounding map: {given}")
    return meta[given[0]] if given else None


def _need_spatial_map(meta):
    src = _spatial_map_of(meta)
    if src is None:
        raise ValueError(f"a spatial checkpoint needs its map under one of the meta keys {SPATIAL_META_KEYS}")
    return src


def _need_sem_map(meta):
    if meta.get(SEM_META_KEY) is None:
        raise ValueError(f"a semantic-map checkpoint needs its class map under the meta key {SEM_META_KEY!r}")
    return meta[SEM_META_KEY]


def load_spatial_map(image) -> torch.Tensor:
    """gligen_inference.py:190-194 + :226-228: ``Image.open(path).convert("RGB")`` (or a ``PIL.Image``), torchvision's centre crop to the
    shorter side (top / left = round((side - crop) / 2)), PIL ``resize((512, 512))`` (its default filter), pil_to_tensor, ``/ 255``,
    ``(v - 0.5) / 0.5`` -> fp32 [3, 512, 512]"""
    from PIL import Image
    im = image if isinstance(image, Image.Image) else Image.open(image)
    im = im.convert("RGB")
    w, h = im.size
    crop = min(w, h)
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    im = im.crop((left, top, left + crop, top + crop)).resize((512, 512))
    x = torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1).contiguous()       # torchvision PILToTensor
    return (x.float() / 255 - 0.5) / 0.5


@torch.no_grad()
def prepare_batch_spatial(meta, batch=1, device=None):
    """gligen_inference.py:221-297 (prepare_batch_hed / _canny / _depth / _normal, one function here: they differ in the meta key alone).  The
    map under ``meta["canny_image"]`` / ``["hed_image"]`` / ``["depth"]`` / ``["normal"]`` (a path or a ``PIL.Image``) repeated ``batch`` times:
    ``map`` [batch, 3, 512, 512] in [-1, 1] and ``mask`` [batch, 1] of ones.  A list of ``batch`` maps gives one map per sample."""
    src = _need_spatial_map(meta)
    if isinstance(src, (list, tuple)):
        if len(src) != batch:
            raise ValueError(f"{len(src)} grounding maps for a batch of {batch}")
        maps = torch.stack([load_spatial_map(s) for s in src], 0)
    else:
        maps = load_spatial_map(src).unsqueeze(0).repeat(batch, 1, 1, 1)
    out = {"map": maps, "mask": torch.ones(batch, 1)}
    return {k: v.to(device) for k, v in out.items()} if device is not None else out


SEM_META_KEY = "sem"                      # the reference's meta key of a semantic map (gligen_inference.py:322)
SEM_IMAGE_SIZE = 512


def load_sem_map(image) -> torch.Tensor:
    """gligen_inference.py:322-324 + :330: ``Image.open(path).convert("L")`` (or a ``PIL.Image``), torchvision's centre crop to the shorter
    side (the rounding of ``load_spatial_map``), ``resize((512, 512), Image.NEAREST)``, pil_to_tensor -> the class ids, uint8 [512, 512]"""
    from PIL import Image
    im = image if isinstance(image, Image.Image) else Image.open(image)
    im = im.convert("L")
    w, h = im.size
    crop = min(w, h)
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    im = im.crop((left, top, left + crop, top + crop)).resize((SEM_IMAGE_SIZE, SEM_IMAGE_SIZE), Image.NEAREST)
    return torch.from_numpy(np.array(im, dtype=np.uint8)).contiguous()


@torch.no_grad()
def prepare_batch_sem(meta, batch=1, device=None, classes=152):
    """gligen_inference.py:318-337 without its one-hot: the semantic map under ``meta["sem"]`` (a path or a ``PIL.Image`` of class ids)
    repeated ``batch`` times as ``sem`` uint8 [batch, 512, 512], the CLASS MAP the reference's ``scatter_`` one-hot [batch, classes, 512, 512]
    argmaxes to (the kernels of a semantic-map model read it directly), and ``mask`` [batch, 1] of ones.  A list of ``batch`` maps gives one
    map per sample.  A pixel value >= ``classes`` raises ValueError (the reference's ``scatter_`` raises there too); the colour visualisation
    side file of the reference is not written."""
    src = _need_sem_map(meta)
    if isinstance(src, (list, tuple)):
        if len(src) != batch:
            raise ValueError(f"{len(src)} semantic maps for a batch of {batch}")
        maps = torch.stack([load_sem_map(s) for s in src], 0)
    else:
        maps = load_sem_map(src).unsqueeze(0).repeat(batch, 1, 1)
    hi = int(maps.max())
    if hi >= classes:
        raise ValueError(f"the semantic map holds the class id {hi}: the model has the classes 0 .. {classes - 1}")
    out = {"sem": maps, "mask": torch.ones(batch, 1)}
    return {k: v.to(device) for k, v in out.items()} if device is not None else out


@torch.no_grad()
def prepare_batch_multiple(meta, model, processor, batch=1, max_objs=MAX_OBJS, device=None):
    """interface.py:424-475: one layout per prompt."""
    phrases_batch = meta.get("phrases")
    if phrases_batch is None:
        phrases_batch = [None] * len(meta["locations"])
    phrases_batch = [[None] * len(loc) if ph is None else ph for ph, loc in zip(phrases_batch, meta["locations"])]
    assert batch == len(phrases_batch)
    cols = [[] for _ in range(6)]
    cache = get_clip_features_batched(model, processor, [ph for phrases in phrases_batch for ph in phrases], device)
    # meta["images"]: per prompt a list with one reference image (path / PIL.Image) or None per box, or None for a prompt without images;
    # distinct images are encoded once for the whole batch
    images_batch = meta.get("images")
    icache = None
    if images_batch is not None:
        if len(images_batch) != len(phrases_batch):
            raise ValueError(f"images: {len(images_batch)} lists for a batch of {len(phrases_batch)}")
        icache = get_image_features_cached(model, processor, [im for ims in images_batch if ims is not None for im in ims], device, meta)
    for i, phrases in enumerate(phrases_batch):
        parts = _one_sample_grounding(phrases, meta["locations"][i], model, processor, max_objs, device, cache,
                                      images=None if images_batch is None else images_batch[i], image_cache=icache)
        parts = list(parts)
        parts[2] = parts[2].unsqueeze(0) * complete_mask(meta.get("text_mask"), max_objs)
        parts[3] = parts[3].unsqueeze(0) * complete_mask(meta.get("image_mask"), max_objs)
        for j in (0, 1, 4, 5):
            parts[j] = parts[j].unsqueeze(0)
        for j in range(6):
            cols[j].append(parts[j])
    names = ("boxes", "masks", "text_masks", "image_masks", "text_embeddings", "image_embeddings")
    return {n: torch.cat(c, dim=0).to(device) for n, c in zip(names, cols)}


def _relation_phrases(prompt, max_relas):
    """interface.py:221-240: scene-graph triplets "subject relation object"; 'PAD' first, each relation listed
    twice, truncated to max_relas.  [] when the prompt has no relation."""
    import sng_parser   # same optional dependency as the reference (interface.py:8)
    graph = sng_parser.parse(prompt)
    entities = graph["entities"]
    triplets = []
    for r in graph.get("relations", []):
        triplets.append(" ".join([entities[r["subject"]]["lemma_head"], r["relation"], entities[r["object"]]["lemma_head"]]))
    return (["PAD"] + triplets + triplets)[:max_relas] if triplets else []


@torch.no_grad()
def prepare_relation_phrases_batch(prompts, max_relas=5, text_encoder=None, device=None, parse=_relation_phrases):
    """One ``text_encoder.encode`` call for the relation phrases of ALL prompts (the reference encodes them prompt
    by prompt, interface.py:490-496).  FrozenCLIPEmbedder pads every row to 77 tokens (modules.py:159-161), so
    batching cannot change a row's pooled embedding.  Returns [len(prompts), max_relas, 768], zero-padded."""
    lists = [parse(p, max_relas) for p in prompts]
    flat = [ph for l in lists for ph in l]
    emb = torch.zeros(len(prompts), max_relas, 768)
    if flat:
        _, pooled = text_encoder.encode(flat, return_pooler_output=True)
        pooled = pooled.to(emb.dtype).cpu()
        k = 0
        for i, l in enumerate(lists):
            emb[i, :len(l), :] = pooled[k:k + len(l)]
            k += len(l)
    return emb.to(device)


@torch.no_grad()
def prepare_relation_phrases(prompt, batch_size=1, max_relas=5, text_encoder=None, device=None):
    """interface.py:221-252: one prompt's relation embeddings repeated batch_size times."""
    emb = prepare_relation_phrases_batch([prompt], max_relas, text_encoder, device)
    return emb.repeat(batch_size, 1, 1)


def _postprocess(samples):
    """interface.py:543-547: clamp -> [0,1] -> *255 -> uint8 truncation -> PIL."""
    from PIL import Image
    out = []
    for sample in samples:
        sample = torch.clamp(sample, min=-1, max=1) * 0.5 + 0.5
        sample = sample.cpu().numpy().transpose(1, 2, 0) * 255
        out.append(Image.fromarray(sample.astype(np.uint8)))
    return out


def _vae_factor(autoencoder) -> int:
    cfg = getattr(autoencoder, "cfg", None)
    return 2 ** (len(cfg.ch_mult) - 1) if cfg is not None else 8


def load_input_image(image, side, device=None) -> torch.Tensor:
    """gligen_inference.py:400-401 at any size: ``Image.open(path).convert("RGB").resize((side, side))`` (or that of a
    ``PIL.Image``), pil_to_tensor, then ``(x / 255 - 0.5) / 0.5`` in fp32 on ``device`` -> [1, 3, side, side].  ``side`` may be
    ``(H, W)``: the image is resized to PIL's (W, H) -> [1, 3, H, W]."""
    from PIL import Image
    H, W = (side, side) if isinstance(side, int) else (int(v) for v in side)
    im = image if isinstance(image, Image.Image) else Image.open(image)
    im = im.convert("RGB").resize((W, H))
    x = torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1).contiguous()       # torchvision pil_to_tensor
    return (x.float().unsqueeze(0).to(device) / 255 - 0.5) / 0.5


def build_inpainting_extra(z0, mask):
    """gligen_inference.py:406-407: ``masked_z = z0 * mask``, ``cat([masked_z, mask], dim=1)`` -- what an inpaint_mode UNet's first conv reads
    next to the latent.  z0 [1|B, 4, h, w] (broadcast over the mask's batch), mask [B, 1, h, w] -> [B, 5, h, w]."""
    return torch.cat([z0 * mask, mask], dim=1)


def check_sampler_args(sampler="plms", ddim_eta=0.0, ddim_discretize="uniform"):
    """The sampler switch (``args["sampler"]`` / ``args["ddim_eta"]`` / ``args["ddim_discretize"]``), checked before any encoder or kernel
    runs: an unknown sampler, a negative or non-finite eta, an unknown discretisation, or eta / "quad" together with PLMS (which has neither)
    raise ValueError.  Returns (sampler, eta, discretize).  sampler.resolve_sampler up to the "ddim" stage: the keys of the samplers behind
    it, and what those refuse, are check_dpm_args' part."""
    _, v = resolve_sampler(dict(sampler=sampler, ddim_eta=ddim_eta, ddim_discretize=ddim_discretize), upto="ddim")
    return v["sampler"], v["ddim_eta"], v["ddim_discretize"]


def check_dpm_args(sampler="plms", dpm_order=2, dpm_discretize="logsnr", ddim_eta=0.0, ddim_discretize="uniform"):
    """The keys of ``args["sampler"] = "dpmpp_2m"`` (``args["dpm_order"]`` 2 | 1, ``args["dpm_discretize"]`` "logsnr" | "quad" | "uniform"),
    checked next to check_sampler_args (which has judged ``sampler`` and the ddim keys on their own), before any encoder or kernel runs.
    ValueError naming the key: a bad order or discretisation; either at a non-default value with "plms" / "ddim" (which have neither);
    ``ddim_eta`` != 0 or ``ddim_discretize`` != "uniform" with "dpmpp_2m" (a deterministic solver with its own grids).
    Returns (order, discretize).  sampler.resolve_sampler on all five keys: what check_sampler_args would refuse is refused here as well."""
    _, v = resolve_sampler(dict(sampler=sampler, dpm_order=dpm_order, dpm_discretize=dpm_discretize, ddim_eta=ddim_eta, ddim_discretize=ddim_discretize))
    return v["dpm_order"], v["dpm_discretize"]


LAYOUT_GUIDANCE_KEY = "layout_guidance_scale"


def check_layout_guidance(value, family=None):
    """``args["layout_guidance_scale"]``, the layout's own guidance scale s_l next to ``guidance_scale`` = s_t (three-branch guidance,
    sampler._Sampler), checked before any encoder or kernel runs.  None (the key absent: one scale for both) or a finite real >= 0 that is
    no bool; anything else raises ValueError naming the key.  ``family`` (family.Family): a map family (canny / hed / depth / normal, sem)
    refuses a number -- its map also enters through the first conv, which every branch shares, so a text-only branch is not defined there.
    Returns None or the float."""
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value) or value < 0:
        raise ValueError(f"{LAYOUT_GUIDANCE_KEY} = {value!r}: None or a finite number >= 0")
    if family is not None and family.extra_key is not None:
        raise ValueError(f"{LAYOUT_GUIDANCE_KEY} given to a {family.label} checkpoint: its map also feeds the first conv, which the text-only "
                         "branch would share; separate text and layout scales need a text, text_image or keypoint checkpoint")
    return float(value)


STRENGTH_KEY = "strength"
INIT_IMAGE_KEY = "init_image"


def check_strength(value, has_image):
    """``args["strength"]`` against ``meta["init_image"]`` (image-to-image, sampler._Sampler.sample_from), checked before any encoder or
    kernel runs.  Without an image the key must be absent (or None): a number there raises ValueError naming it; returns None.  With one:
    None = host.IMG2IMG_DEFAULT_STRENGTH (0.75, the Stable Diffusion img2img script's default), else host.check_strength -- a finite real in
    (0, 1] that is no bool.  Returns None or the float."""
    if value is not None:
        value = host.check_strength(value)
    if not has_image:
        if value is not None:
            raise ValueError(f"{STRENGTH_KEY} = {value!r} without meta[{INIT_IMAGE_KEY!r}]: it is the share of the schedule that runs on that image")
        return None
    return host.IMG2IMG_DEFAULT_STRENGTH if value is None else value


def _load_images(ims, key, bs, side, device) -> torch.Tensor:
    """``meta[key]``: one image (a path or a PIL.Image) for every sample, or a list with one per sample (another length: ValueError naming
    the key) -> fp32 [1|bs, 3, H, W] (load_input_image)"""
    if isinstance(ims, (list, tuple)):
        if len(ims) != bs:
            raise ValueError(f"{key}: {len(ims)} images for a batch of {bs}")
        return torch.cat([load_input_image(im, side, device) for im in ims], 0)
    return load_input_image(ims, side, device)


@torch.no_grad()
def denoise(all_models, context, uc, relations, grounding_batch, starting_noise, alpha_type=None, guidance_scale=7.5,
            steps=PLMS_STEPS, mask=None, x0=None, inpainting_extra_input=None, grounding_extra_input=None, sampler="plms", ddim_eta=0.0,
            ddim_discretize="uniform", dpm_order=2, dpm_discretize="logsnr", layout_guidance_scale=None, init_latent=None, strength=None):
    """The denoising hot path proper, from conditioning tensors to the final latent
    (run_batch_images lines interface.py:505-539 without text/VAE stages).  ``mask`` [1|B, 1, h, w] (1 = keep) and ``x0``
    [1|B, 4, h, w] (the encoded input image): inpainting, plms.py:95-99.  The latent's shape [B, 4, h, w] is ``starting_noise``'s
    (plms.py:68-71); h != w needs both to be multiples of 2^(number of UNet downsamples) = 8.  ``inpainting_extra_input`` [1|B, 5, h, w]: the
    extra first-conv input of an inpaint_mode model (required there, ignored by every other model).  ``relations``: None for a model without
    the relation chain (ignored there); a model with it raises ValueError on None before any kernel runs.  ``grounding_extra_input``
    [B, 3, H, W]: the map a spatial model's grounding downsampler reads (required there, ignored by every other model).  ``sampler``: "plms"
    or "ddim" (sampler.DDIMSampler, with ``ddim_eta`` >= 0 and ``ddim_discretize`` "uniform" | "quad"), or "dpmpp_2m"
    (sampler.DPMSolverSampler, with ``dpm_order`` 2 | 1 and ``dpm_discretize`` "logsnr" | "quad" | "uniform"; there ``steps`` bounds the
    number of UNet evaluations, 20 is the usual choice); all five go through sampler.resolve_sampler first.  ``layout_guidance_scale``:
    None, or the layout's own scale s_l >= 0 -- e = (e_u + s_t (e_t - e_u)) + s_l (e_c - e_t) with s_t = ``guidance_scale`` and e_t the
    branch that reads the prompt and the null grounding (check_layout_guidance; any sampler; refused on a map family).  ``init_latent``
    fp32 [1|B, 4, h, w] with ``strength`` in (0, 1] (both or neither): image-to-image -- the last int(strength * n) of the schedule's n nodes
    run, from ``init_latent`` noised with ``starting_noise`` to where they begin (any sampler; sampler._Sampler.sample_from)."""
    model, autoencoder, text_encoder, diffusion, config = all_models
    if (init_latent is None) != (strength is None):
        raise ValueError(f"{STRENGTH_KEY} and init_latent go together: got {STRENGTH_KEY} = {strength!r} and init_latent "
                         f"{'absent' if init_latent is None else 'given'}")
    if strength is not None:
        strength = host.check_strength(strength)
    spec, values = resolve_sampler(dict(sampler=sampler, ddim_eta=ddim_eta, ddim_discretize=ddim_discretize, dpm_order=dpm_order,
                                        dpm_discretize=dpm_discretize))
    layout = check_layout_guidance(layout_guidance_scale, family_of(getattr(model, "cfg", None)))
    _check_noise(model, starting_noise)
    callbacks = dict(alpha_generator_func=partial(alpha_generator, type=alpha_type), set_alpha_scale=set_alpha_scale)
    sampler = spec.cls(diffusion, model, **spec.kwargs(values), **callbacks)
    grounding_input = model.grounding_tokenizer_input.prepare(grounding_batch, text_encoder)
    input = dict(x=starting_noise, timesteps=None, context=context, relations=relations, grounding_input=grounding_input,
                 inpainting_extra_input=inpainting_extra_input, grounding_extra_input=grounding_extra_input)
    shape = tuple(starting_noise.shape)
    if init_latent is not None:
        return sampler.sample_from(S=steps, shape=shape, input=input, uc=uc, guidance_scale=guidance_scale, init_latent=init_latent,
                                   strength=strength, mask=mask, x0=x0, layout_guidance_scale=layout)
    if layout is not None:
        return sampler.sample_layout(S=steps, shape=shape, input=input, uc=uc, guidance_scale=guidance_scale, layout_guidance_scale=layout,
                                     mask=mask, x0=x0)
    return sampler.sample(S=steps, shape=shape, input=input, uc=uc, guidance_scale=guidance_scale, mask=mask, x0=x0)


def _check_noise(model, starting_noise) -> None:
    """A rectangular starting noise that breaks the engine's shape rule is refused here, before any encoder or kernel runs."""
    if torch.is_tensor(starting_noise) and starting_noise.dim() == 4 and starting_noise.shape[-2] != starting_noise.shape[-1]:
        from .engine import check_latent_hw
        check_latent_hw(model.cfg, int(starting_noise.shape[-2]), int(starting_noise.shape[-1]))


def _has_images(images, multiple) -> bool:
    """any reference image in meta["images"] (a flat list, or per-prompt lists / None with ``multiple``)"""
    if images is None:
        return False
    flat = [im for ims in images if ims is not None for im in ims] if multiple else images
    return any(im is not None for im in flat)


_OWN_MAP = {"map": _need_spatial_map, "sem": _need_sem_map}       # Family.extra_key -> the map under the family's own meta key(s), or ValueError


def _refuse_foreign_meta(model, fam, meta, multiple, hw) -> None:
    """Every refusal of ``_run``, before any encoder or kernel runs: what the meta dict carries against what the family (family.Family) takes.
    Reads ``model.cfg`` alone, plus ``model.grounding_extra_of`` (the latent-size rule) on a map family."""
    if _has_images(meta.get("images"), multiple) and not fam.images:
        # (the reference would prepare image tokens and drop them silently: text_layout_tokinzer_input.py reads three keys)
        raise ValueError("meta['images'] given to a text-only checkpoint: image grounding needs a *_box_text_image checkpoint "
                         "(grounding_tokenizer target text_image_grounding_net.PositionNet)")
    if fam.extra_key != "sem" and meta.get(SEM_META_KEY) is not None:
        raise ValueError(f"a semantic map (meta['sem']) given to a {fam.label} checkpoint: class maps need a semantic-map checkpoint "
                         "(grounding_tokenizer target sem_grounding_net.PositionNet)")
    if fam.extra_key != "map" and _spatial_map_of(meta) is not None:
        raise ValueError(f"a grounding map ({[k for k in SPATIAL_META_KEYS if meta.get(k) is not None][0]}) given to a {fam.label} checkpoint: " +
                         ("it is grounded on a class map under meta['sem']" if fam.extra_key else "maps need a canny / hed / depth / normal checkpoint"))
    for k, why in fam.refuses:
        if meta.get(k) is not None and (k != "locations" or len(meta[k]) > 0):
            raise ValueError(f"meta[{k!r}] given to a {model.cfg.grounding} checkpoint: {why}")
    if fam.extra_key is not None:
        _OWN_MAP[fam.extra_key](meta)
        model.grounding_extra_of({"grounding_extra_input": True}, hw)      # the latent-size rule
    if model.cfg.inpaint_mode and meta.get("input_image") is None:
        # (the reference would fail inside the first forward, on th.cat([h, None]), openaimodel.py:439)
        raise ValueError("an inpaint_mode checkpoint needs meta['input_image']: its first conv reads the masked image latent and the mask "
                         "(layout-to-image without an input image runs on the 4-channel checkpoints)")


def _run(all_models, args, meta, starting_noise, clip_model, clip_processor, device, multiple):
    model, autoencoder, text_encoder, diffusion, config = all_models
    _check_noise(model, starting_noise)
    fam = family_of(model.cfg)           # the batch builder follows the model, not the checkpoint's file name
    # the layout's guidance scale is read from ``args`` per call, like ``steps``; absent (or None), denoise is called as it always was
    layout = check_layout_guidance(args.get(LAYOUT_GUIDANCE_KEY), fam)
    # image-to-image: ``strength`` is read from ``args`` per call as well, and never from the cached config
    strength = check_strength(args.get(STRENGTH_KEY), meta.get(INIT_IMAGE_KEY) is not None)
    _refuse_foreign_meta(model, fam, meta, multiple, tuple(int(v) for v in starting_noise.shape[-2:]) if fam.extra_key else None)
    # the sampler switch is read from ``args`` per call, like ``steps``: not sticky through the cached config
    _, sampler_values = resolve_sampler(args)
    if layout is not None:
        sampler_values = dict(sampler_values, layout_guidance_scale=layout)
    config.update(args)                      # mutates the caller's dict, like interface.py:297/484
    cfg = _AttrDict(config)
    if cfg.get("no_plms", False):
        raise NotImplementedError("no_plms = True is the reference's DDIM switch, which is broken there with this UNet (SURVEY App-B#8) and "
                                  "stays refused; DDIM runs under args[\"sampler\"] = \"ddim\" (with args[\"ddim_eta\"], args[\"ddim_discretize\"])")
    bs = cfg.batch_size
    if isinstance(meta.get(INIT_IMAGE_KEY), (list, tuple)) and len(meta[INIT_IMAGE_KEY]) != bs:      # refused before any encoder runs
        raise ValueError(f"{INIT_IMAGE_KEY}: {len(meta[INIT_IMAGE_KEY])} images for a batch of {bs}")
    max_rel = cfg.get("max_relations", 10)
    # (a keypoint model: no phrases, no CLIP model, and -- always on the upstream block -- no relation phrases)
    batch = fam.build(globals()[fam.batch[multiple]], meta, model.cfg, clip_model, clip_processor, bs, device)
    prompts = meta["prompts"] if multiple else [meta["prompt"]] * bs
    context = text_encoder.encode(prompts)
    relations = None
    if model.cfg.relation:                   # a checkpoint without rela_fuse: no scene-graph parse, no relation phrases
        relations = prepare_relation_phrases_batch(meta["prompts"], max_rel, text_encoder, device=device) if multiple else \
            prepare_relation_phrases(meta["prompt"], bs, max_rel, text_encoder, device=device)
    # the reference encodes bs copies of "" (interface.py:496); args["negative_prompt"] (gligen_inference.py:379-380) replaces it, per call
    neg = args.get("negative_prompt")
    if neg is not None and not isinstance(neg, str):
        raise TypeError(f"negative_prompt must be a string or None, got {type(neg).__name__}")
    uc = text_encoder.encode(["" if neg is None else neg]).repeat(bs, 1, 1)
    mask = z0 = extra = None
    if meta.get("input_image") is not None:
        # inpainting (gligen_inference.py:393-407): encode the input image, regenerate inside the boxes (mask 0), keep the rest
        L = tuple(int(v) for v in starting_noise.shape[-2:])              # latent (h, w); the image is vae_factor times that per axis
        side = tuple(_vae_factor(autoencoder) * v for v in L)
        z0 = autoencoder.encode(_load_images(meta["input_image"], "input_image", bs, side, device))
        mask = host.draw_masks_from_boxes(batch["boxes"], L).to(starting_noise.device)
        if model.cfg.inpaint_mode:
            # an inpaint_mode checkpoint (gligen_inference.py:406-407): the first conv also reads [z0 * mask | mask]; the sampler keeps
            # replacing the known region as well (:430 passes mask and x0 too).  A 4-channel model runs the latent blend alone.
            extra = build_inpainting_extra(z0, mask)
    if strength is not None:
        # image-to-image (SDEdit): the encoded image (the posterior sample * scale factor, as above; its one torch.randn draw comes before
        # anything the sampler draws) is noised to where the truncated schedule starts; independent of the inpainting keys
        side = tuple(_vae_factor(autoencoder) * int(v) for v in starting_noise.shape[-2:])
        sampler_values = dict(sampler_values, strength=strength,
                              init_latent=autoencoder.encode(_load_images(meta[INIT_IMAGE_KEY], INIT_IMAGE_KEY, bs, side, device)))
    # S is a harness parameter: the reference hard-codes 50 (interface.py:507); ``args["steps"]`` overrides it
    samples = denoise(all_models, context, uc, relations, batch, starting_noise, meta.get("alpha_type"), cfg.guidance_scale,
                      steps=int(args.get("steps", PLMS_STEPS)), mask=mask, x0=z0,   # steps per call: not sticky through the cached config
                      inpainting_extra_input=extra,
                      grounding_extra_input=batch[fam.extra_key] if fam.extra_key else None,      # *_grounding_downsampler_input.prepare: the map itself
                      **sampler_values)
    return _postprocess(autoencoder.decode(samples))


@torch.no_grad()
def run_one_image(all_models, args, meta, starting_noise=None, clip_model=None, clip_processor=None, device=None):
    """interface.py:292-357.  ``meta["input_image"]`` (a path or a PIL.Image): inpaint that image inside the boxes.  ``meta["init_image"]``
    (a path or a PIL.Image) with ``args["strength"]`` in (0, 1] (0.75 when absent): image-to-image, re-render that image under the prompt
    and the boxes, the more freely the higher the strength (independent of ``input_image``; every checkpoint family).  On a keypoint checkpoint
    ``meta["locations"]`` is a list of persons, each 17 ``[x, y]`` (prepare_batch_kp); no phrases, no CLIP model, no input image."""
    return _run(all_models, args, meta, starting_noise, clip_model, clip_processor, device, multiple=False)


@torch.no_grad()
def run_batch_images(all_models, args, meta, starting_noise=None, clip_model=None, clip_processor=None, device=None):
    """interface.py:478-549.  ``meta["input_image"]`` / ``meta["init_image"]`` (inpainting / image-to-image with ``args["strength"]``, see
    run_one_image): a list with one image (path or PIL.Image) per sample, or one for all.  On a keypoint
    checkpoint ``meta["locations"]`` holds one pose layout (a list of persons of 17 ``[x, y]``) per prompt; no phrases, no CLIP model."""
    return _run(all_models, args, meta, starting_noise, clip_model, clip_processor, device, multiple=True)


def latent_hw(height=None, width=None, autoencoder=None):
    """Latent (h, w) of a ``height`` x ``width`` pixel image: each a positive multiple of 8 * vae_factor (the UNet halves the latent three
    times, the VAE scales it by vae_factor = 8: multiples of 64 pixels), else ValueError.  None = the reference's 64 latent rows / columns
    (interface.py:388, :566), 512 pixels with the shipped VAE."""
    f = _vae_factor(autoencoder)
    height, width = (64 * f if v is None else v for v in (height, width))
    for name, v in (("height", height), ("width", width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0 or v % (8 * f):
            raise ValueError(f"{name} = {v!r}: must be a positive multiple of {8 * f} pixels")
    return int(height) // f, int(width) // f


def generate_one_image(all_models, caption, label, bbox, clip_model=None, clip_processor=None, device=None):
    """interface.py:376-395 (converts xywh -> ltrb, :383): the reference's signature and its 512 x 512 image."""
    return generate_one_image_sized(all_models, caption, label, bbox, clip_model, clip_processor, device)


def generate_one_image_sized(all_models, caption, label, bbox, clip_model=None, clip_processor=None, device=None, height=None, width=None):
    """``generate_one_image`` with ``height`` / ``width`` (pixels, multiples of 64).  They only size the starting noise
    ``torch.randn(1, 4, height / 8, width / 8)``; None (the default) is the reference's 64 latent rows / columns = 512 pixels, drawn the
    same way."""
    h, w = latent_hw(height, width, all_models[1])
    args = dict(batch_size=1, no_plms=False, guidance_scale=7.5)
    bbox = [convert_xywh_to_ltrb(b) for b in bbox]
    meta = dict(prompt=caption, phrases=label, locations=bbox, alpha_type=[0.3, 0.0, 0.7])
    starting_noise = torch.randn(args["batch_size"], 4, h, w).to(device)
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    return run_one_image(all_models, args, meta, starting_noise, clip_model, clip_processor, device=device)


def generate_batch_images(all_models, captions, labels, bboxes, clip_model=None, clip_processor=None, device=None):
    """interface.py:551-570 (boxes are NOT converted here, App-B#10): the reference's signature and its 512 x 512 images."""
    return generate_batch_images_sized(all_models, captions, labels, bboxes, clip_model, clip_processor, device)


def generate_batch_images_sized(all_models, captions, labels, bboxes, clip_model=None, clip_processor=None, device=None, height=None,
                                width=None):
    """``generate_batch_images`` with ``height`` / ``width`` (pixels, multiples of 64): as in generate_one_image_sized."""
    h, w = latent_hw(height, width, all_models[1])
    bs = len(captions)
    args = dict(batch_size=bs, no_plms=False, guidance_scale=7.5)
    meta = dict(prompts=captions, phrases=labels, locations=bboxes, alpha_type=[0.3, 0.0, 0.7])
    starting_noise = torch.randn(bs, 4, h, w).to(device)
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    return run_batch_images(all_models, args, meta, starting_noise, clip_model, clip_processor, device=device)


# ------------------------------------------------------------------------------------------------------------------
# Multi-GPU product entry.  The reference's inference path is single-GPU (txt2img.py:535-536,
# train_rl.py:321); prompts are independent units, so the 8-GPU mode is: rank 0 reads the checkpoint, ONE broadcast
# carries the packed UNet + VAE weights, every call shards the prompts round-robin (rank r takes prompts r, r + world, ...),
# per-PROMPT seeds make a sample's result independent of the rank that ran it, and the uint8 images are gathered on rank 0.
# One process per GPU under torch.distributed ("nccl" = RCCL over xGMI on ROCm; "gloo" in the tests).
# ------------------------------------------------------------------------------------------------------------------
def load_all_models_sharded(ckpt, device, src=0, strict=None):
    """``load_all_models`` for a torch.distributed job: only rank ``src`` touches the checkpoint file; the others receive the
    packed UNet (the C engine's flat weight buffer), the packed VAE decoder and -- when the checkpoint's text encoder runs on the HIP
    tower -- its weights in dist.broadcast_bundle's single collective, plus the config dict.  With a reference torch text encoder
    the receiving ranks get ``text_encoder = None``: conditioning is then prepared on ``src`` and scattered per call
    (generate_batch_images_sharded).  Returns the usual 5-tuple on every rank."""
    import torch.distributed as dist
    from .dist import broadcast_bundle
    if not (dist.is_available() and dist.is_initialized()):
        return load_all_models(ckpt, device, strict=strict)
    rank = dist.get_rank()
    if rank == src:
        am = load_all_models(ckpt, device, strict=strict)
        model, autoencoder, text_encoder, diffusion, config = am
        if family_of(model.cfg).name != "text":
            raise NotImplementedError(f"the sharded entry is text-only: a {model.cfg.grounding} checkpoint runs through load_all_models / "
                                      "run_batch_images")
        if model.cfg.inpaint_mode:
            raise NotImplementedError("the sharded entry has no input image: an inpaint_mode checkpoint runs through load_all_models / "
                                      "run_one_image / run_batch_images with meta['input_image']")
        if not model.cfg.relation:
            raise NotImplementedError("the sharded entry prepares and scatters relation phrases: a checkpoint without rela_fuse runs through "
                                      "load_all_models / run_one_image / run_batch_images")
        if not isinstance(autoencoder, VAEDecoder):
            raise NotImplementedError("the sharded entry broadcasts the HIP VAE decoder's packed weights (unset GLIGEN_REFERENCE_VAE)")
        dcfg = dict(linear_start=diffusion.linear_start, linear_end=diffusion.linear_end, timesteps=diffusion.num_timesteps)
        # the HIP text tower travels too (fp32 state dict, ~0.5 GB for ViT-L/14's text model, same single broadcast) together with its
        # (picklable, host-side) tokenizer, so that every rank encodes its own prompts; a reference torch encoder stays on src
        hip_te = _is_hip_encoder(text_encoder)
        te_extra = dict(tokenizer=text_encoder.tokenizer, heads=text_encoder.heads, max_length=text_encoder.max_length) if hip_te else None
        broadcast_bundle(model.engine.P, autoencoder.W, model.cfg, device, src,
                         extra=dict(config=config, vcfg=autoencoder.cfg, diffusion=dcfg, text_encoder=te_extra,
                                    allow_missing_sd_conv=bool(model.allow_missing_sd_conv),
                                    strict=bool(model.strict)),
                         aux=dict(text_encoder=text_encoder.towers_state_dict()) if hip_te else None)
        return am
    P, vw, extra, aux = broadcast_bundle(None, None, None, device, src, want_aux=True)
    model = UNetModel.from_packed(P, P.cfg, device, extra.get("allow_missing_sd_conv", False))     # src's GLIGEN_ALLOW_NO_SD_CONV applies to every rank
    if extra.get("strict"):                 # ... and so does its strict mode (the split weight layout travelled in the broadcast)
        model.set_strict(True)
    autoencoder = VAEDecoder.from_packed(vw, extra["vcfg"], device)
    d = extra["diffusion"]
    diffusion = LatentDiffusion(linear_start=d["linear_start"], linear_end=d["linear_end"], timesteps=d["timesteps"], device=device)
    text_encoder = None
    if extra.get("text_encoder") is not None:
        from .text_encoder import HipCLIPTextEncoder
        te = extra["text_encoder"]
        text_encoder = HipCLIPTextEncoder(aux["text_encoder"], te["tokenizer"], device, heads=te["heads"], max_length=te["max_length"])
    return model, autoencoder, text_encoder, diffusion, extra["config"]


def _collective_device(device):
    """Object collectives of the RCCL backend stage their bytes on the CURRENT device: make that this rank's GPU even when the
    caller never called torch.cuda.set_device (all ranks staging on GPU 0 is an RCCL 'duplicate GPU' error)."""
    import contextlib
    d = torch.device(device)
    return torch.cuda.device(d) if d.type == "cuda" else contextlib.nullcontext()


@torch.no_grad()
def prepare_conditioning(all_models, captions, labels, bboxes, clip_model, clip_processor, device):
    """Everything ``run_batch_images`` feeds the sampler (interface.py:486-535), per prompt row, on the CPU: context / uc
    [n, 77, 768], relations [n, R, 768], boxes / masks / text_embeddings [n, 30, ...].  Rows are independent, so any subset of
    rows is a valid batch."""
    model, autoencoder, text_encoder, diffusion, config = all_models
    n = len(captions)
    meta = dict(prompts=captions, phrases=labels, locations=bboxes)
    batch = prepare_batch_multiple(meta, clip_model, clip_processor, n, device=device)
    cond = dict(context=text_encoder.encode(captions), uc=text_encoder.encode([""]).repeat(n, 1, 1),
                relations=prepare_relation_phrases_batch(captions, config.get("max_relations", 10), text_encoder, device=device),
                boxes=batch["boxes"], masks=batch["masks"], text_embeddings=batch["text_embeddings"])
    return {k: v.detach().float().cpu().contiguous() for k, v in cond.items()}


def _is_hip_encoder(m) -> bool:
    from .text_encoder import HipCLIPTextEncoder
    return isinstance(m, HipCLIPTextEncoder)


def tokenize_conditioning(all_models, captions, labels, bboxes, clip_processor, max_objs=MAX_OBJS):
    """Host-side half of the conditioning prep for the HIP encoders: every string of ``run_batch_images``'s prep
    (interface.py:424-475, :486-496) becomes token rows -- no GPU work, a few KB per prompt, so rank ``src`` does it for the
    whole call and the ranks encode their own rows (encode_conditioning).  Returns a dict of CPU tensors:
    cap_ids [n, 77], uc_ids [1, 77], rel_ids [m, 77] + rel_owner / rel_slot [m] (prompt, slot) of each relation phrase,
    phrase_ids [k, L] (the distinct grounding phrases, ``clip_processor`` padding) + phrase_index [n, max_objs] (-1 = none),
    boxes [n, max_objs, 4], masks [n, max_objs]."""
    model, autoencoder, text_encoder, diffusion, config = all_models
    n = len(captions)
    R = config.get("max_relations", 10)
    rel_lists = [_relation_phrases(p_, R) for p_ in captions]
    flat = [ph for l in rel_lists for ph in l]
    T = text_encoder.max_length
    phrases_batch = labels if labels is not None else [None] * n
    phrases_batch = [[None] * len(loc) if ph is None else ph for ph, loc in zip(phrases_batch, bboxes)]
    uniq = [p_ for p_ in dict.fromkeys(ph for phrases in phrases_batch for ph in phrases) if p_ is not None]
    where = {p_: i for i, p_ in enumerate(uniq)}
    boxes = torch.zeros(n, max_objs, 4)
    masks = torch.zeros(n, max_objs)
    pidx = torch.full((n, max_objs), -1, dtype=torch.long)
    for i, (phrases, locs) in enumerate(zip(phrases_batch, bboxes)):
        for j, (box, ph) in enumerate(zip(locs, phrases)):
            boxes[i, j] = torch.tensor(box)
            masks[i, j] = 1
            if ph is not None:
                pidx[i, j] = where[ph]
    return dict(cap_ids=text_encoder.tokenize(captions), uc_ids=text_encoder.tokenize([""]),
                rel_ids=text_encoder.tokenize(flat) if flat else torch.zeros(0, T, dtype=torch.long),
                rel_owner=torch.tensor([i for i, l in enumerate(rel_lists) for _ in l], dtype=torch.long),
                rel_slot=torch.tensor([j for l in rel_lists for j in range(len(l))], dtype=torch.long), max_relations=R,
                phrase_ids=clip_processor(text=uniq, return_tensors="pt", padding=True)["input_ids"] if uniq else torch.zeros(0, 1, dtype=torch.long),
                phrase_index=pidx, boxes=boxes, masks=masks)


@torch.no_grad()
def encode_conditioning(all_models, tok, rows, phrase_encoder, device):
    """GPU half: the conditioning tensors of prompt rows ``rows`` from their token rows, on THIS rank's HIP text tower
    (all_models' HipCLIPTextEncoder for prompts / empty prompt / relation phrases; ``phrase_encoder`` for the grounding phrases'
    pooled features, interface.py:114-141).  Same dict as prepare_conditioning, on ``device``."""
    te = all_models[2]
    rows = [int(r_) for r_ in rows]
    nr, R, D = len(rows), int(tok["max_relations"]), te.hidden
    context = te.encode_ids(tok["cap_ids"][rows]) if nr else torch.zeros(0, te.max_length, D, device=device)
    uc = te.encode_ids(tok["uc_ids"]).repeat(nr, 1, 1)
    relations = torch.zeros(nr, R, D, device=device)
    pos = {r_: i for i, r_ in enumerate(rows)}
    sel = [k for k, o in enumerate(tok["rel_owner"].tolist()) if o in pos]
    if sel:
        pooled = te.encode_ids(tok["rel_ids"][sel], return_pooler_output=True)[1]
        relations[[pos[int(tok["rel_owner"][k])] for k in sel], [int(tok["rel_slot"][k]) for k in sel]] = pooled
    pidx = tok["phrase_index"][rows]
    emb = torch.zeros(nr, pidx.shape[1], D, device=device)
    used = sorted(set(int(v) for v in pidx.flatten().tolist() if v >= 0))
    if used:
        pooled = phrase_encoder.pooler_output(tok["phrase_ids"][used])
        lut = {u: i for i, u in enumerate(used)}
        ii, jj = (pidx >= 0).nonzero(as_tuple=True)
        emb[ii.to(device), jj.to(device)] = pooled[[lut[int(pidx[a, b])] for a, b in zip(ii.tolist(), jj.tolist())]]
    return dict(context=context, uc=uc, relations=relations, boxes=tok["boxes"][rows].to(device), masks=tok["masks"][rows].to(device),
                text_embeddings=emb)


def prompt_noise(seeds, latent=64):
    """Starting noise [n, 4, latent, latent] (``latent`` = (h, w): [n, 4, h, w]), row i drawn from its OWN CPU generator seeded with
    ``seeds[i]``: a prompt's noise does not depend on the batch it is in or the rank it runs on."""
    lh, lw = (latent, latent) if isinstance(latent, int) else (int(v) for v in latent)
    rows = []
    for sd_ in seeds:
        g = torch.Generator(device="cpu")
        g.manual_seed(int(sd_))
        rows.append(torch.randn(1, 4, lh, lw, generator=g))
    return torch.cat(rows, 0) if rows else torch.zeros(0, 4, lh, lw)


@torch.no_grad()
def run_shard(all_models, cond, noise, device, alpha_type=(0.3, 0.0, 0.7), guidance_scale=7.5, steps=PLMS_STEPS):
    """Denoise + decode the rows of ``cond`` (a prepare_conditioning dict, or a row subset of one) as ONE batch;
    returns uint8 [n, H, W, 3] (the arithmetic of _postprocess, interface.py:543-547)."""
    model, autoencoder = all_models[0], all_models[1]
    n = noise.shape[0]
    if n == 0:
        return np.zeros((0, 0, 0, 3), dtype=np.uint8)
    model.first_conv_type = "GLIGEN"      # every sharded call starts from the checkpoint's state, whatever ran before on this rank
    dv = lambda t: t.to(device)
    batch = dict(boxes=dv(cond["boxes"]), masks=dv(cond["masks"]), text_embeddings=dv(cond["text_embeddings"]))
    lat = denoise(all_models, dv(cond["context"]), dv(cond["uc"]), dv(cond["relations"]), batch, dv(noise), list(alpha_type),
                  guidance_scale, steps=steps)
    img = autoencoder.decode(lat)
    img = torch.clamp(img, min=-1, max=1) * 0.5 + 0.5
    return (img.cpu().numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)


@torch.no_grad()
def generate_batch_images_sharded(all_models, captions=None, labels=None, bboxes=None, clip_model=None, clip_processor=None,
                                  device=None, seeds=None, src=0, steps=PLMS_STEPS, latent=64, height=None, width=None):
    """``generate_batch_images`` (interface.py:551-570) across the ranks of a torch.distributed job.  Rank ``src`` passes the
    prompts (the others pass None) and gets the list of PIL images in prompt order; the other ranks get None.
    Per call: one object broadcast of the conditioning rows (~0.4 MB per prompt), no collective during the 51 sampling
    steps, one gather of uint8 images.  ``seeds[i]`` seeds prompt i's starting noise (default: i).  ``height`` / ``width`` (pixels,
    multiples of 64, the same on every rank) size the starting noise as in generate_batch_images_sized; an axis left None stays at ``latent``
    (512 pixels by default)."""
    import torch.distributed as dist
    from .dist import shard_indices
    from PIL import Image
    if height is not None or width is not None:          # validated on every rank alike, before the first collective
        f = _vae_factor(all_models[1])
        lh, lw = (latent, latent) if isinstance(latent, int) else latent
        latent = latent_hw(f * lh if height is None else height, f * lw if width is None else width, all_models[1])
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    box = [None]
    # With the HIP text tower in all_models on every rank (load_all_models_sharded ships its weights in the bundle) only the
    # host-side STRING work happens on src: the token rows travel (a few KB per prompt) and every rank encodes its own shard --
    # no rank-0 serial encoder stage.  Reference torch encoders (only present on src) keep the older flow: src encodes all rows.
    # Nothing between two collectives may raise on one rank only (the others would block forever in the next collective): every
    # failure travels as the payload of the collective that follows it and is raised on every rank after it.
    hip_flow = _is_hip_encoder(all_models[2])
    if rank == src or not multi:
        try:
            n = len(captions)
            seeds = list(range(n)) if seeds is None else [int(s_) for s_ in seeds]
            assert len(seeds) == n
            if hip_flow:
                if clip_model is not None and not _is_hip_encoder(clip_model):
                    # a reference torch CLIPModel for the grounding phrases (interface.py:114-141): never substituted silently by the
                    # checkpoint's text tower.  One process: moved onto the HIP tower once (cached on the object); several ranks: the
                    # other ranks do not hold its weights, so the caller has to pass an encoder every rank can build
                    if multi:
                        raise ValueError("clip_model is a torch CLIPModel that only rank %d holds: pass hip_phrase_encoder(clip_model, device) "
                                         "built from the same weights on EVERY rank, or None on every rank to encode the grounding phrases "
                                         "with the checkpoint's text tower" % src)
                    # cached on the object together with a fingerprint of what it was built from (target device, storage address and in-place
                    # version counter of the first parameter): a CLIPModel that is fine-tuned, reloaded or moved afterwards gets a fresh
                    # fp16 copy instead of silently encoding with the stale one
                    p0 = next(iter(clip_model.parameters()), None) if hasattr(clip_model, "parameters") else None
                    fp = (str(device), None if p0 is None else (p0.data_ptr(), int(getattr(p0, "_version", 0)), str(p0.device)))
                    entry = getattr(clip_model, "_gligen_hip_phrase_encoder", None)
                    if entry is None or entry[0] != fp:
                        entry = (fp, hip_phrase_encoder(clip_model, device))
                        try:
                            clip_model._gligen_hip_phrase_encoder = entry
                        except AttributeError:      # objects without attribute storage (__slots__): rebuilt per call
                            pass
                    clip_model = entry[1]
                box = [dict(tok=tokenize_conditioning(all_models, captions, labels, bboxes, clip_processor), seeds=seeds,
                            own_phrase_encoder=_is_hip_encoder(clip_model))]
            else:
                # prepare_conditioning returns HOST tensors: object collectives pickle tensors with their device, and rank r must not
                # receive rank 0's "cuda:0" tensors
                box = [dict(cond=prepare_conditioning(all_models, captions, labels, bboxes, clip_model, clip_processor, device), seeds=seeds)]
        except Exception as ex:          # noqa: BLE001
            if not multi:
                raise
            box = [dict(error=f"rank {rank}: {type(ex).__name__}: {ex}")]
    if multi:
        with _collective_device(device):
            dist.broadcast_object_list(box, src=src)
        if "error" in box[0]:
            raise RuntimeError("generate_batch_images_sharded failed on " + box[0]["error"])      # on every rank alike
        if "tok" in box[0] and box[0]["own_phrase_encoder"]:
            # src encodes the grounding phrases with its own HIP phrase encoder (clip_model): every rank must hold one -- agreed on
            # by ALL ranks before any of them diverges
            flags = [None] * world
            with _collective_device(device):
                dist.all_gather_object(flags, bool(_is_hip_encoder(clip_model)))
            missing = [r_ for r_, f_ in enumerate(flags) if not f_]
            if missing:
                raise ValueError("ranks %s passed no HIP phrase encoder: src encodes the grounding phrases with its own (clip_model); every "
                                 "rank must pass one built from the same CLIP weights, or all ranks pass None to use the checkpoint's text "
                                 "tower" % missing)
    seeds = box[0]["seeds"]
    n = len(seeds)
    mine = shard_indices(n, rank, world)
    # a rank whose shard fails (encoding included: sequence too long, out of memory, graph capture) still takes part in the gather,
    # with the error as its payload: the others must not block forever in gather_object, and src re-raises
    err, imgs = None, None
    try:
        if "tok" in box[0]:
            # grounding phrases: this rank's own phrase encoder when src has one (a HipCLIPTextEncoder, e.g.
            # hip_phrase_encoder(CLIPModel)), else the conditioning tower itself -- the GLIGEN checkpoint's text encoder and the
            # reference's default CLIPModel are both openai/clip-vit-large-patch14 (encoders/modules.py:146, train_rl.py:282)
            pe = clip_model if box[0]["own_phrase_encoder"] else all_models[2]
            sub = encode_conditioning(all_models, box[0]["tok"], mine, pe, device)
        else:
            sub = {k: v[mine] for k, v in box[0]["cond"].items()}
        imgs = run_shard(all_models, sub, prompt_noise([seeds[i] for i in mine], latent), device, steps=steps)
    except Exception as ex:          # noqa: BLE001
        if not multi:
            raise
        imgs, err = None, f"rank {rank}: {type(ex).__name__}: {ex}"
    if not multi:
        return [Image.fromarray(a) for a in imgs]
    parts = [None] * world if rank == src else None
    with _collective_device(device):
        dist.gather_object((mine, imgs, err), parts, dst=src)
    if rank != src:
        if err is not None:
            raise RuntimeError(err)
        return None
    errors = [e_ for _, _, e_ in parts if e_ is not None]
    if errors:
        raise RuntimeError("generate_batch_images_sharded failed on " + "; ".join(errors))
    out = [None] * n
    for idx, arr, _ in parts:
        for j, i in enumerate(idx):
            out[i] = Image.fromarray(arr[j])
    return out
