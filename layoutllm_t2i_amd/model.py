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
from .family import FAMILIES, family_of
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


class _GroundingInput:
    """The one implementation behind the reference's five ``*_tokinzer_input`` classes: ``prepare`` passes the family's tensors through and
    notes the payload's batch / device / dtype and the null shapes; ``get_null_input`` is zeros of those.  ``prepare`` also accepts the
    two-argument call of interface.py:516.  KEYS are the family record's."""
    KEYS = ()
    PAYLOAD = ""                # the key whose tensor gives batch, device and dtype
    NULL_DTYPES = {}            # keys whose null tensor has a dtype of its own

    def __init__(self):
        self.set = False

    def _tensors(self, batch, text_encoder):
        return {k: batch[k] for k in self.KEYS}

    def prepare(self, batch, text_encoder=None):
        self.set = True
        out = self._tensors(batch, text_encoder)
        payload = out[self.PAYLOAD]
        self.batch, self.device, self.dtype = payload.shape[0], payload.device, payload.dtype
        self._null_shapes = self._shapes(out)       # per key, behind the batch axis
        return out

    def get_null_input(self, batch=None, device=None, dtype=None):
        assert self.set, "not set yet, cannot call this funcion"
        batch = self.batch if batch is None else batch
        device = self.device if device is None else device
        dtype = self.dtype if dtype is None else dtype
        return {k: torch.zeros(batch, *shape).type(self.NULL_DTYPES.get(k, dtype)).to(device) for k, shape in self._null_shapes.items()}


class GroundingNetInput(_GroundingInput):
    """text_layout_tokinzer_input.py:6-62: boxes / masks / text embeddings (or ``labels``, encoded token by token) -> ``positive_embeddings``."""
    KEYS, PAYLOAD = FAMILIES["text"].keys, "positive_embeddings"

    def _tensors(self, batch, text_encoder):
        boxes, masks = batch["boxes"], batch["masks"]
        if "text_embeddings" in batch:
            positive_embeddings = batch["text_embeddings"]
        else:
            labels = [s.split("|") for s in batch["labels"]]
            box_list = torch.sum(masks, dim=-1).tolist()
            positive_embeddings = torch.zeros((boxes.shape[0], boxes.shape[1], 768)).to(boxes.device)
            for b in range(boxes.shape[0]):
                for i in range(int(box_list[b])):
                    positive_embeddings[b, i] = text_encoder.encode_one_token(labels[b][i])
        return {"boxes": boxes, "masks": masks, "positive_embeddings": positive_embeddings}

    def _shapes(self, out):
        (_, self.max_box, _), self.in_dim = out["boxes"].shape, 768
        return {"boxes": (self.max_box, 4), "masks": (self.max_box,), "positive_embeddings": (self.max_box, self.in_dim)}


class TextImageGroundingNetInput(_GroundingInput):
    """text_image_grounding_tokinzer_input.py:5-61: the six grounding tensors of a ``*_box_text_image`` checkpoint."""
    KEYS, PAYLOAD = FAMILIES["text_image"].keys, "text_embeddings"

    def _shapes(self, out):
        _, self.max_box, self.in_dim = out["text_embeddings"].shape
        return {k: (self.max_box,) + {"boxes": (4,), "text_embeddings": (self.in_dim,), "image_embeddings": (self.in_dim,)}.get(k, ())
                for k in self.KEYS}


class KeypointGroundingNetInput(_GroundingInput):
    """keypoint_grounding_tokinzer_input.py:6-44: ``points`` [B, 17 P, 2] and ``masks`` [B, 17 P] of a keypoint checkpoint."""
    KEYS, PAYLOAD = FAMILIES["keypoint"].keys, "points"

    def _shapes(self, out):
        self.max_persons_per_image = int(out["points"].shape[1] / 17)
        return {"points": (self.max_persons_per_image * 17, 2), "masks": (self.max_persons_per_image * 17,)}


class SpatialGroundingNetInput(_GroundingInput):
    """{canny,hed,depth,normal}_grounding_tokinzer_input.py:6-43 under generic keys: ``map`` [B, 3, H, W] in [-1, 1] (the reference's
    canny_edge / hed_edge / depth / normal) and ``mask``; the null input is a zero map with a zero mask [B]."""
    KEYS, PAYLOAD = FAMILIES["spatial"].keys, "map"

    def _shapes(self, out):
        _, self.C, self.H, self.W = out["map"].shape
        return {"map": (self.C, self.H, self.W), "mask": ()}


class SemGroundingNetInput(_GroundingInput):
    """sem_grounding_tokinzer_input.py:6-43: ``sem``, the integer class map [B, H, W] (the native form here) or the reference's float
    one-hot [B, C, H, W] (semantic.ClassMapInput), and ``mask``; the null input is a zero tensor of the same form with a float32 zero mask [B]."""
    KEYS, PAYLOAD, NULL_DTYPES = FAMILIES["sem"].keys, "sem", {"mask": torch.float32}

    def _shapes(self, out):
        self.shape = tuple(out["sem"].shape[1:])
        return {"sem": self.shape, "mask": ()}


_GROUNDING_INPUTS = {"text": GroundingNetInput, "text_image": TextImageGroundingNetInput, "keypoint": KeypointGroundingNetInput,
                     "spatial": SpatialGroundingNetInput, "sem": SemGroundingNetInput}


def grounding_input_class(cfg: UNetConfig):
    """the grounding-tokenizer input class that goes with the config's PositionNet"""
    return _GROUNDING_INPUTS[family_of(cfg).name]


def grounding_input_for(cfg: UNetConfig):
    return grounding_input_class(cfg)()


class UNetModel:
    """Callable with the reference's ``input`` dict (keys interface.py:527-535), returns eps [B,4,h,w].

    ``state_dict``: reference-named fp32 tensors (numpy or torch).  ``sd_first_conv``: the tensors of
    GLIGEN/SD_input_conv_weight_bias.pth (``{'weight','bias'}``) that restore_first_conv_from_SD()
    switches to, permanently, exactly like the reference (openaimodel.py:393-411).
    """

    # what an instance assembled by hand around an engine (bench.py's facade) leaves unset
    tokenizer = downsampler = None
    inpaint_mode = allow_missing_sd_conv = strict = _told_not_restorable = False

    def __init__(self, cfg: UNetConfig, state_dict: Mapping[str, object], device="cuda:0",
                 sd_first_conv: Optional[Mapping[str, object]] = None, allow_missing_sd_conv: bool = False):
        if cfg.inpaint_mode and sd_first_conv is not None:
            raise ValueError("an inpaint_mode model has no SD first conv: its 9-channel first conv is not restorable (openaimodel.py:296)")
        maps = family_of(cfg).extra_key is not None
        if maps and cfg.split_weights:
            raise NotImplementedError("strict mode (split_weights) of a spatial model: the ConvNeXt tokenizer has no split-fp16 form")
        self._assemble(pack_state_dict(state_dict, cfg, torch.device(device), sd_first_conv), cfg, device, allow_missing_sd_conv,
                       sd_first_conv is not None)
        if maps:
            # the two stages in front of the UNet, from the checkpoint's own position_net.* / downsample_net.* tensors
            from .spatial import map_stages
            self.tokenizer, self.downsampler = map_stages(state_dict, cfg, self.device)

    @classmethod
    def from_packed(cls, packed, cfg: UNetConfig, device, allow_missing_sd_conv: bool = False) -> "UNetModel":
        """A model around already-packed weights (a broadcast pack, another model's): every attribute ``__init__`` sets, the family's
        grounding input included.  ``packed=None``: no engine, for host-side use of the model's checks."""
        self = cls.__new__(cls)
        self._assemble(packed, cfg, device, allow_missing_sd_conv, packed is not None and bool(packed.has_sd_conv))
        self.grounding_tokenizer_input = grounding_input_for(cfg)
        return self

    def _assemble(self, packed, cfg, device, allow_missing_sd_conv, restorable):
        self.cfg = cfg
        self.device = torch.device(device)
        self.image_size, self.in_channels, self.out_channels, self.model_channels = cfg.image_size, cfg.in_channels, cfg.out_channels, cfg.model_channels
        self.inpaint_mode = cfg.inpaint_mode
        self.first_conv_restorable = restorable
        self.allow_missing_sd_conv = bool(allow_missing_sd_conv)
        self.first_conv_type = "GLIGEN"
        self.grounding_tokenizer_input: Optional[GroundingNetInput] = None   # set externally (interface.py:370)
        self.fuser_scale = 1.0          # what set_alpha_scale writes (interface.py:34-38)
        self.training = False
        self.engine = UNetEngine(packed) if packed is not None else None
        self.tokenizer = self.downsampler = None
        self._cond_key = None
        self.strict = False

    def set_strict(self, on: bool = True):
        """STRICT mode of the engine (gl_set_handle_option 50; include/gligen_hip.h): every matrix product on split-fp16 operands, output
        within north_star's rtol 1e-3 / atol 1e-4 of the fp32 reference.  Needs weights packed in the split layout
        (``UNetConfig.split_weights``; ``interface.load_ckpt(..., strict=True)`` does both)."""
        if on and not self.cfg.split_weights:
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
        if self.inpaint_mode:
            # the reference's non-restorable branch (openaimodel.py:406-408): nothing is switched, nothing raises, every step keeps the
            # checkpoint's 9-channel conv (the reference prints its message on every scale-0 step; here once per model)
            if not self._told_not_restorable:
                print("First conv layer is not restorable and skipped this process, probably because this is an inpainting model?")
                self._told_not_restorable = True
        elif self.first_conv_restorable:
            self.first_conv_type = "SD"
        elif self.allow_missing_sd_conv:
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

    def tokens_of(self, grounding: dict) -> dict:
        """What the family's engine entry reads of a grounding dict: the dict itself, or -- a map family -- the tokens of its tokenizer.
        The one check that the family's keys are all there."""
        fam = family_of(self.cfg)
        missing = [k for k in fam.keys if k not in grounding]
        if missing:
            raise ValueError(f"a {self.cfg.grounding} model needs the grounding keys {fam.keys}; missing {missing}")
        if fam.extra_key is None:
            return grounding
        return {"tokens": self.tokenizer.tokens(grounding[fam.extra_key], grounding["mask"])}

    def set_conditioning(self, context, relations, grounding: dict, hw, key=None) -> None:
        """``hw``: the latent side, or (h, w) for a rectangular latent (UNetEngine.set_conditioning).  ``relations``: None on a model without
        the relation chain (a given tensor is ignored there); None on any other model raises ValueError before the engine is touched."""
        if self.cfg.relation and relations is None:
            self.relations_of({})
        if key is not None and key == self._cond_key:
            return
        family_of(self.cfg).condition(self.engine, context, relations, self.tokens_of(grounding), hw)
        self._cond_key = key

    def condition(self, input: dict, uc=None, always_extra: bool = False, text_branch: bool = False) -> int:
        """Everything the engine holds per image, from the reference's ``input`` dict: the family's conditioning entry, then the downsampled
        ``grounding_extra_input`` of a map family and the ``inpainting_extra_input`` of an inpaint_mode model.  Every missing input raises
        before the engine is touched.  ``uc``: the unconditional context of classifier-free guidance -- the conditioning batch becomes
        [cond ; uncond] over whatever keys the family has, the unconditional half on the null grounding (a map family: the tokenizer's cached
        null tokens) and, where there are relations, on the same ones (plms.py:115-124).  ``always_extra``: hand the grounding extra over
        even while the SD first conv, which does not read it, is switched in (a sampler switches convs between steps).  ``text_branch``
        (needs ``uc``): the batch of three-branch guidance, [cond ; text-only ; uncond] -- the added third carries the conditional context
        with the unconditional third's grounding and relations; the inpainting extra is shared by all thirds.  Returns the batch multiple,
        3 with ``text_branch``, else 2 with ``uc`` and 1 without."""
        if text_branch and uc is None:
            raise ValueError("text_branch=True needs uc: the text-only third sits between the conditional and the unconditional one")
        H, W = (int(v) for v in input["x"].shape[-2:])
        extra = self.inpaint_extra_of(input)
        gextra = self.grounding_extra_of(input, (H, W)) if always_extra or not self.use_sd_conv else None
        rel = self.relations_of(input)
        g = self.tokens_of(self.grounding_of(input))
        ctx = input["context"]
        if uc is not None:
            if "tokens" in g:
                null = {"tokens": self.tokenizer.null_tokens().expand(g["tokens"].shape[0], -1, -1)}
            elif self.grounding_tokenizer_input is None:
                raise RuntimeError("model.grounding_tokenizer_input is not set (interface.py:370)")
            else:
                null = self.grounding_tokenizer_input.get_null_input()
            f32 = lambda t: t.to(self.device, torch.float32)
            if text_branch:
                # [cond ; text-only ; uncond]: the middle third reads the prompt, the null grounding and the same relations
                ctx = torch.cat([f32(ctx), f32(ctx), f32(uc)], 0)
                rel = torch.cat([f32(rel)] * 3, 0) if rel is not None else None
                g = {k: torch.cat([f32(g[k]), f32(null[k]), f32(null[k])], 0) for k in null}
            else:
                ctx = torch.cat([f32(ctx), f32(uc)], 0)
                rel = torch.cat([f32(rel)] * 2, 0) if rel is not None else None
                g = {k: torch.cat([f32(g[k]), f32(null[k])], 0) for k in null}
        family_of(self.cfg).condition(self.engine, ctx, rel, g, H if H == W else (H, W))      # (H, W): the rectangular entry and its shape check
        self._cond_key = None
        if gextra is not None:
            self.engine.set_grounding_extra(self.downsampler(gextra))
        if extra is not None:
            self.engine.set_inpaint_extra(extra)
        return 1 if uc is None else 3 if text_branch else 2

    def relations_of(self, input: dict):
        """``input["relations"]``: required on a model with the rela_fuse chain (ValueError before any kernel runs); a model loaded from a
        checkpoint without it (``cfg.relation`` False, the upstream GLIGEN block) takes no relations -- the upstream ``input`` dict has no such
        key -- and ignores a given tensor."""
        if not self.cfg.relation:
            return None
        rel = input.get("relations")
        if rel is None:
            raise ValueError("this model carries the rela_fuse relation chain: input['relations'] [B, R, ctx] is required (only a checkpoint "
                             "without rela_fuse tensors, UNetConfig.relation = False, runs without relations)")
        return rel

    def inpaint_extra_of(self, input: dict) -> Optional[torch.Tensor]:
        """``input["inpainting_extra_input"]`` (openaimodel.py:436-439): required on an inpaint_mode model, ignored on every other (as the
        reference ignores it)."""
        if not self.inpaint_mode:
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
        if self.downsampler is None:
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
        self.condition(input)
        return self.engine.forward(input["x"].to(self.device, torch.float32).contiguous(), input["timesteps"], self.fuser_scale, self.use_sd_conv,
                                   1).clone()

    forward = __call__


def load_sd_first_conv(path: Optional[str] = None) -> Optional[dict]:
    """Reads GLIGEN/SD_input_conv_weight_bias.pth once (the reference re-reads it from disk on every
    scale-0 step, openaimodel.py:397-398)."""
    if path is None or not os.path.exists(path):
        return None
    sd = torch.load(path, map_location="cpu")
    return {"weight": sd["weight"].float(), "bias": sd["bias"].float()}
