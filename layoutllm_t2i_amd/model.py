"""Host-side mirrors of the reference objects that sit on the denoising path's boundary.

  UNetModel          <- ldm.modules.diffusionmodules.openaimodel.UNetModel     (openaimodel.py:234-459)
  LatentDiffusion    <- ldm.models.diffusion.ldm.LatentDiffusion / ddpm.DDPM   (schedule buffers only)
  GroundingNetInput  <- grounding_input.text_layout_tokinzer_input.GroundingNetInput

Same attribute names, call contracts and error behaviour; the arithmetic lives in the HIP engine.
"""
from __future__ import annotations

import os
from typing import Mapping, Optional

import numpy as np
import torch

from . import host
from .arch import UNetConfig
from .engine import UNetEngine
from .weights import pack_state_dict


class LatentDiffusion:
    """Schedule holder (ddpm.py:19-54; ldm.py:12-22).  Only the buffers the sampler reads."""

    def __init__(self, linear_start: float = 0.00085, linear_end: float = 0.012, timesteps: int = 1000,
                 beta_schedule: str = "linear", device="cpu"):
        if beta_schedule != "linear":
            raise NotImplementedError("only the 'linear' beta schedule is on the reference's path (coco2014.yaml:1-6)")
        acp = host.alphas_cumprod(timesteps, linear_start, linear_end)
        betas64 = np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2
        self.num_timesteps = int(timesteps)
        self.linear_start, self.linear_end = linear_start, linear_end
        self.betas = torch.tensor(betas64, dtype=torch.float32, device=device)
        self.alphas_cumprod = torch.tensor(acp, dtype=torch.float32, device=device)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, acp.astype(np.float64)[:-1]), dtype=torch.float32, device=device)
        # q(x_t | x_0) coefficients (ddpm.py:39-40): fp64 sqrt of the fp64 cumprod (util.py:21-23 builds the betas with
        # torch.linspace), stored as fp32 -- what q_sample and the masked PLMS step read
        acp64 = np.cumprod(1.0 - (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=torch.float64) ** 2).numpy(), axis=0)
        self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(acp64), dtype=torch.float32, device=device)
        self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - acp64), dtype=torch.float32, device=device)
        self.clip_denoised = False

    def to(self, device):
        for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def q_sample(self, x_start, t, noise=None):
        """ldm.py:19-22: extract_into_tensor of the two fp32 buffers, a * x_start + s * noise."""
        noise = torch.randn_like(x_start) if noise is None else noise
        b = t.shape[0]
        a = self.sqrt_alphas_cumprod.to(x_start.device).gather(-1, t.to(x_start.device)).reshape(b, *((1,) * (x_start.dim() - 1)))
        s = self.sqrt_one_minus_alphas_cumprod.to(x_start.device).gather(-1, t.to(x_start.device)).reshape(b, *((1,) * (x_start.dim() - 1)))
        return a * x_start + s * noise


class GroundingNetInput:
    """text_layout_tokinzer_input.py:6-62: pass-through of boxes/masks/text embeddings, zeros as null."""

    def __init__(self):
        self.set = False

    def prepare(self, batch, text_encoder=None):
        self.set = True
        boxes, masks = batch["boxes"], batch["masks"]
        self.batch, self.max_box, _ = boxes.shape
        self.device = boxes.device
        self.in_dim = 768
        if "text_embeddings" in batch:
            positive_embeddings = batch["text_embeddings"]
        else:
            labels = [s.split("|") for s in batch["labels"]]
            box_list = torch.sum(masks, dim=-1).tolist()
            positive_embeddings = torch.zeros((self.batch, self.max_box, self.in_dim)).to(self.device)
            for b in range(self.batch):
                for i in range(int(box_list[b])):
                    positive_embeddings[b, i] = text_encoder.encode_one_token(labels[b][i])
        self.dtype = positive_embeddings.dtype
        return {"boxes": boxes, "masks": masks, "positive_embeddings": positive_embeddings}

    def get_null_input(self, batch=None, device=None, dtype=None):
        assert self.set, "not set yet, cannot call this funcion"
        batch = self.batch if batch is None else batch
        device = self.device if device is None else device
        dtype = self.dtype if dtype is None else dtype
        boxes = torch.zeros(batch, self.max_box, 4).type(dtype).to(device)
        masks = torch.zeros(batch, self.max_box).type(dtype).to(device)
        positive_embeddings = torch.zeros(batch, self.max_box, self.in_dim).type(dtype).to(device)
        return {"boxes": boxes, "masks": masks, "positive_embeddings": positive_embeddings}


class TextImageGroundingNetInput:
    """text_image_grounding_tokinzer_input.py:5-61: pass-through of the six grounding tensors of a ``*_box_text_image`` checkpoint, zeros
    as null.  ``prepare`` also accepts the two-argument call of interface.py:516."""
    KEYS = ("boxes", "masks", "text_masks", "image_masks", "text_embeddings", "image_embeddings")

    def __init__(self):
        self.set = False

    def prepare(self, batch, text_encoder=None):
        self.set = True
        text_embeddings = batch["text_embeddings"]
        self.batch, self.max_box, self.in_dim = text_embeddings.shape
        self.device = text_embeddings.device
        self.dtype = text_embeddings.dtype
        return {k: batch[k] for k in self.KEYS}

    def get_null_input(self, batch=None, device=None, dtype=None):
        assert self.set, "not set yet, cannot call this funcion"
        batch = self.batch if batch is None else batch
        device = self.device if device is None else device
        dtype = self.dtype if dtype is None else dtype
        z = lambda *shape: torch.zeros(*shape).type(dtype).to(device)
        return {"boxes": z(batch, self.max_box, 4), "masks": z(batch, self.max_box), "text_masks": z(batch, self.max_box),
                "image_masks": z(batch, self.max_box), "text_embeddings": z(batch, self.max_box, self.in_dim),
                "image_embeddings": z(batch, self.max_box, self.in_dim)}


class KeypointGroundingNetInput:
    """keypoint_grounding_tokinzer_input.py:6-44: pass-through of ``points`` [B, 17 P, 2] and ``masks`` [B, 17 P] of a keypoint checkpoint,
    zeros as null.  ``prepare`` also accepts the two-argument call of interface.py:516."""
    KEYS = ("points", "masks")

    def __init__(self):
        self.set = False

    def prepare(self, batch, text_encoder=None):
        self.set = True
        points, masks = batch["points"], batch["masks"]
        self.batch, tokens, _ = points.shape
        self.max_persons_per_image = int(tokens / 17)
        self.device = points.device
        self.dtype = points.dtype
        return {"points": points, "masks": masks}

    def get_null_input(self, batch=None, device=None, dtype=None):
        assert self.set, "not set yet, cannot call this funcion"
        batch = self.batch if batch is None else batch
        device = self.device if device is None else device
        dtype = self.dtype if dtype is None else dtype
        return {"points": torch.zeros(batch, self.max_persons_per_image * 17, 2).type(dtype).to(device),
                "masks": torch.zeros(batch, self.max_persons_per_image * 17).type(dtype).to(device)}


class SpatialGroundingNetInput:
    """{canny,hed,depth,normal}_grounding_tokinzer_input.py:6-43 under generic keys: pass-through of ``map`` [B, 3, H, W] in [-1, 1] (the
    reference's canny_edge / hed_edge / depth / normal) and ``mask`` [B]; the null input is a zero map with a zero mask."""
    KEYS = ("map", "mask")

    def __init__(self):
        self.set = False

    def prepare(self, batch, text_encoder=None):
        self.set = True
        map_, mask = batch["map"], batch["mask"]
        self.batch, self.C, self.H, self.W = map_.shape
        self.device = map_.device
        self.dtype = map_.dtype
        return {"map": map_, "mask": mask}

    def get_null_input(self, batch=None, device=None, dtype=None):
        assert self.set, "not set yet, cannot call this funcion"
        batch = self.batch if batch is None else batch
        device = self.device if device is None else device
        dtype = self.dtype if dtype is None else dtype
        return {"map": torch.zeros(batch, self.C, self.H, self.W).type(dtype).to(device), "mask": torch.zeros(batch).type(dtype).to(device)}


class SemGroundingNetInput:
    """sem_grounding_tokinzer_input.py:6-43: pass-through of ``sem`` and ``mask`` [B].  ``sem`` is the integer class map [B, H, W] (the native
    form here) or the reference's float one-hot [B, C, H, W] (semantic.ClassMapInput); the null input is a zero tensor of the same form with
    a zero mask."""
    KEYS = ("sem", "mask")

    def __init__(self):
        self.set = False

    def prepare(self, batch, text_encoder=None):
        self.set = True
        sem, mask = batch["sem"], batch["mask"]
        self.batch, self.shape = sem.shape[0], tuple(sem.shape[1:])
        self.device = sem.device
        self.dtype = sem.dtype
        return {"sem": sem, "mask": mask}

    def get_null_input(self, batch=None, device=None, dtype=None):
        assert self.set, "not set yet, cannot call this funcion"
        batch = self.batch if batch is None else batch
        device = self.device if device is None else device
        dtype = self.dtype if dtype is None else dtype
        return {"sem": torch.zeros(batch, *self.shape).type(dtype).to(device), "mask": torch.zeros(batch).type(torch.float32).to(device)}


_GROUNDING_INPUTS = {"text": GroundingNetInput, "text_image": TextImageGroundingNetInput, "keypoint": KeypointGroundingNetInput,
                     "spatial": SpatialGroundingNetInput}


def grounding_input_class(cfg: UNetConfig):
    """the grounding-tokenizer input class that goes with the config's PositionNet (the semantic-map family is a spatial config with its own
    keys)"""
    return SemGroundingNetInput if getattr(cfg, "ds_kind", "") == "sem" else _GROUNDING_INPUTS[cfg.grounding]


def grounding_input_for(cfg: UNetConfig):
    return grounding_input_class(cfg)()


class UNetModel:
    """Callable with the reference's ``input`` dict (keys interface.py:527-535), returns eps [B,4,h,w].

    ``state_dict``: reference-named fp32 tensors (numpy or torch).  ``sd_first_conv``: the tensors of
    GLIGEN/SD_input_conv_weight_bias.pth (``{'weight','bias'}``) that restore_first_conv_from_SD()
    switches to, permanently, exactly like the reference (openaimodel.py:393-411).
    """

    def __init__(self, cfg: UNetConfig, state_dict: Mapping[str, object], device="cuda:0",
                 sd_first_conv: Optional[Mapping[str, object]] = None, allow_missing_sd_conv: bool = False):
        self.cfg = cfg
        self.device = torch.device(device)
        self.image_size = cfg.image_size
        self.in_channels = cfg.in_channels
        self.out_channels = cfg.out_channels
        self.model_channels = cfg.model_channels
        if cfg.inpaint_mode and sd_first_conv is not None:
            raise ValueError("an inpaint_mode model has no SD first conv: its 9-channel first conv is not restorable (openaimodel.py:296)")
        self.inpaint_mode = cfg.inpaint_mode
        self.first_conv_restorable = sd_first_conv is not None
        self.allow_missing_sd_conv = allow_missing_sd_conv
        self.first_conv_type = "GLIGEN"
        self.grounding_tokenizer_input: Optional[GroundingNetInput] = None   # set externally (interface.py:370)
        self.fuser_scale = 1.0          # what set_alpha_scale writes (interface.py:34-38)
        self.training = False
        if cfg.grounding == "spatial" and getattr(cfg, "split_weights", False):
            raise NotImplementedError("strict mode (split_weights) of a spatial model: the ConvNeXt tokenizer has no split-fp16 form")
        packed = pack_state_dict(state_dict, cfg, self.device, sd_first_conv)
        self.engine = UNetEngine(packed)
        self.tokenizer = self.downsampler = None
        if cfg.grounding == "spatial":
            # the two stages in front of the UNet, from the checkpoint's own position_net.* / downsample_net.* tensors
            if cfg.ds_kind == "sem":
                # the semantic-map family: both stages read one class map (a float one-hot is converted once for the two)
                from .semantic import ClassMapInput, SemDownsampler, SemTokenizer
                cm = ClassMapInput(cfg.sem_classes, self.device)
                self.tokenizer = SemTokenizer(state_dict, cfg, self.device, cm)
                self.downsampler = SemDownsampler(state_dict, cfg, self.device, cm)
            else:
                from .spatial import SpatialDownsampler, SpatialTokenizer
                self.tokenizer = SpatialTokenizer(state_dict, cfg, self.device)
                self.downsampler = SpatialDownsampler(state_dict, cfg, self.device)
        self._cond_key = None
        self.strict = False

    def set_strict(self, on: bool = True):
        """STRICT mode of the engine (gl_set_handle_option 50; include/gligen_hip.h): every matrix product on split-fp16 operands, output
        within north_star's rtol 1e-3 / atol 1e-4 of the fp32 reference.  Needs weights packed in the split layout
        (``UNetConfig.split_weights``; ``interface.load_ckpt(..., strict=True)`` does both)."""
        if on and not getattr(self.cfg, "split_weights", False):
            raise RuntimeError("strict mode needs the split weight layout: build the model with dataclasses.replace(cfg, split_weights=True) "
                               "(interface.load_ckpt(..., strict=True) / GLIGEN_STRICT=1 do)")
        self.engine.set_option(50, 1 if on else 0)
        self.strict = bool(on)
        self._cond_key = None           # the conditioning hoists are option-dependent: recompute on the next call
        return self

    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device:
            raise NotImplementedError("weights are packed for one device at construction")
        return self

    def restore_first_conv_from_SD(self):
        """openaimodel.py:393-408.  The reference's non-restorable branch exists for inpainting models only; for this
        (non-inpainting) UNet a missing SD conv would silently change 35 of 50 steps, so it is an error unless the
        model was built with ``allow_missing_sd_conv=True`` (then the reference's message is printed)."""
        if getattr(self, "inpaint_mode", False):
            # the reference's non-restorable branch (openaimodel.py:406-408): nothing is switched, nothing raises, every step keeps the
            # checkpoint's 9-channel conv (the reference prints its message on every scale-0 step; here once per model)
            if not getattr(self, "_told_not_restorable", False):
                print("First conv layer is not restorable and skipped this process, probably because this is an inpainting model?")
                self._told_not_restorable = True
        elif self.first_conv_restorable:
            self.first_conv_type = "SD"
        elif getattr(self, "allow_missing_sd_conv", False):
            print("First conv layer is not restorable and skipped this process, probably because this is an inpainting model?")
        else:
            raise RuntimeError("restore_first_conv_from_SD: the SD first-conv weights (GLIGEN/SD_input_conv_weight_bias.pth) were "
                               "not given to UNetModel(sd_first_conv=...); the reference switches to them on every fuser-scale-0 "
                               "step (openaimodel.py:393-405)")

    @property
    def use_sd_conv(self) -> bool:
        return self.first_conv_type == "SD" and self.first_conv_restorable

    # -- conditioning plumbing shared with the sampler
    def grounding_of(self, input: dict) -> dict:
        if "grounding_input" in input:
            return input["grounding_input"]
        if self.grounding_tokenizer_input is None:
            raise RuntimeError("model.grounding_tokenizer_input is not set (interface.py:370)")
        return self.grounding_tokenizer_input.get_null_input()      # (the family's own keys: grounding_input_for)

    def set_conditioning(self, context, relations, grounding: dict, hw, key=None) -> None:
        """``hw``: the latent side, or (h, w) for a rectangular latent (UNetEngine.set_conditioning).  ``relations``: None on a model without
        the relation chain (a given tensor is ignored there); None on any other model raises ValueError before the engine is touched."""
        if getattr(self.cfg, "relation", True) and relations is None:
            self.relations_of({})
        if key is not None and key == self._cond_key:
            return
        if self.cfg.grounding != "text":
            keys = grounding_input_class(self.cfg).KEYS
            missing = [k for k in keys if k not in grounding]
            if missing:
                raise ValueError(f"a {self.cfg.grounding} model needs the grounding keys {keys}; missing {missing}")
        if self.cfg.grounding == "spatial":
            self.engine.set_conditioning_tokens(context, self.tokenizer.tokens(grounding[keys[0]], grounding["mask"]), hw)      # "map" | "sem"
        elif self.cfg.grounding == "keypoint":
            self.engine.set_conditioning_kp(context, grounding["points"], grounding["masks"], hw)
        elif self.cfg.grounding == "text_image":
            self.engine.set_conditioning(context, relations, grounding["boxes"], grounding["masks"], grounding["text_embeddings"], hw,
                                         text_masks=grounding["text_masks"], image_masks=grounding["image_masks"],
                                         image_embeddings=grounding["image_embeddings"])
        else:
            self.engine.set_conditioning(context, relations, grounding["boxes"], grounding["masks"],
                                         grounding["positive_embeddings"], hw)
        self._cond_key = key

    def relations_of(self, input: dict):
        """``input["relations"]``: required on a model with the rela_fuse chain (ValueError before any kernel runs); a model loaded from a
        checkpoint without it (``cfg.relation`` False, the upstream GLIGEN block) takes no relations -- the upstream ``input`` dict has no such
        key -- and ignores a given tensor."""
        if not getattr(self.cfg, "relation", True):
            return None
        rel = input.get("relations")
        if rel is None:
            raise ValueError("this model carries the rela_fuse relation chain: input['relations'] [B, R, ctx] is required (only a checkpoint "
                             "without rela_fuse tensors, UNetConfig.relation = False, runs without relations)")
        return rel

    def inpaint_extra_of(self, input: dict) -> Optional[torch.Tensor]:
        """``input["inpainting_extra_input"]`` (openaimodel.py:436-439): required on an inpaint_mode model, ignored on every other (as the
        reference ignores it)."""
        if not getattr(self, "inpaint_mode", False):
            return None
        extra = input.get("inpainting_extra_input")
        if extra is None:
            raise ValueError("an inpaint_mode model needs input['inpainting_extra_input'] = cat([z0 * mask, mask], dim=1) "
                             "(gligen_inference.py:406-407)")
        return extra

    def grounding_extra_of(self, input: dict, hw=None) -> Optional[torch.Tensor]:
        """``input["grounding_extra_input"]`` (openaimodel_original.py:430-432): the map [B, 3, H, W] the grounding downsampler of a spatial
        model reads; required there (ValueError before any kernel runs), ignored on every other model, as the reference ignores it.  ``hw``:
        the latent's (h, w), which has to be the downsampler's output size (the reference fails inside th.cat otherwise)."""
        if getattr(self, "downsampler", None) is None:
            return None
        extra = input.get("grounding_extra_input")
        if extra is None:
            raise ValueError("a spatial model needs input['grounding_extra_input'], the map its grounding downsampler reads "
                             "(gligen_inference.py:412-422)")
        side = self.cfg.ds_latent
        if hw is not None and tuple(hw) != (side, side):
            raise ValueError(f"latent {hw[0]} x {hw[1]}: this model's grounding downsampler yields {side} x {side} (resize_input / 4; 64 for hed), "
                             "and the latent has to match it")
        return extra

    @torch.no_grad()
    def __call__(self, input: dict) -> torch.Tensor:
        """UNetModel.forward (openaimodel.py:413-459): one B-sized evaluation."""
        x = input["x"]
        if getattr(self, "downsampler", None) is not None:
            gextra = None if self.use_sd_conv else self.grounding_extra_of(input, tuple(int(v) for v in x.shape[-2:]))
            H, W = (int(v) for v in x.shape[-2:])
            self.set_conditioning(input["context"], None, self.grounding_of(input), H if H == W else (H, W), key=None)
            if gextra is not None:
                self.engine.set_grounding_extra(self.downsampler(gextra))
            return self.engine.forward(x.to(self.device, torch.float32).contiguous(), input["timesteps"], self.fuser_scale, self.use_sd_conv,
                                       1).clone()
        extra = self.inpaint_extra_of(input)
        rel = self.relations_of(input)
        g = self.grounding_of(input)
        H, W = (int(v) for v in x.shape[-2:])
        self.set_conditioning(input["context"], rel, g, H if H == W else (H, W), key=None)
        if extra is not None:
            self.engine.set_inpaint_extra(extra)
        t = input["timesteps"]
        return self.engine.forward(x.to(self.device, torch.float32).contiguous(), t, self.fuser_scale, self.use_sd_conv, 1).clone()

    forward = __call__


def load_sd_first_conv(path: Optional[str] = None) -> Optional[dict]:
    """Reads GLIGEN/SD_input_conv_weight_bias.pth once (the reference re-reads it from disk on every
    scale-0 step, openaimodel.py:397-398)."""
    if path is None or not os.path.exists(path):
        return None
    sd = torch.load(path, map_location="cpu")
    return {"weight": sd["weight"].float(), "bias": sd["bias"].float()}
