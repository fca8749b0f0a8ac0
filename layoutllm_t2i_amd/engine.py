"""Python face of the MI355X UNet engine.  The engine itself is C++ behind the forward-level C ABI of
``include/gligen_hip.h`` (``csrc/engine.hip``): block plan, packed-weight layout, activation pool, hoisted
conditioning, launch sequence and hipGraph capture / replay all live behind ``gl_create`` / ``gl_load_weights`` /
``gl_set_conditioning`` / ``gl_unet_forward`` / ``gl_plms_step``.  This class only turns torch tensors (device memory
and streams) into raw pointers for those calls -- it replaces ``UNetModel.forward`` (openaimodel.py:413-459) for the
Python callers (``model.UNetModel``, ``sampler.PLMSSampler``).

No torch op touches activations on the hot path, and there is no fallback: a missing library, a CPU tensor or a
missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import Cfg3EvalArgs, DdimStepArgs, DpmppStepArgs, PlmsStepArgs, check, init_device
from .arch import UNetConfig
from .weights import PackedWeights

F16, F32 = torch.float16, torch.float32


def check_latent_hw(cfg: UNetConfig, h: int, w: int) -> None:
    """The shape rule of a rectangular latent (gl_set_conditioning_hw): rows and columns each a positive multiple of
    2^(number of downsamples) -- with fewer, an upsampled map no longer matches the skip tensor it is concatenated with."""
    f = 2 ** (len(cfg.channel_mult) - 1)
    if h <= 0 or w <= 0 or h % f or w % f:
        raise ValueError(f"latent shape {h} x {w}: rows and columns must each be a positive multiple of {f}")


class UNetEngine:
    def __init__(self, packed: PackedWeights):
        if not torch.cuda.is_available():
            raise RuntimeError("UNetEngine needs a GPU: the denoising path has no CPU fallback")
        if packed.flat is None or not packed.flat.is_cuda:
            raise _lib.HipLibraryError("packed weights must be a flat buffer on the GPU (PackedWeights.to_flat on a cuda device)")
        self.P = packed
        self.cfg: UNetConfig = packed.cfg
        self.plan = packed.plan
        self.dev = torch.device(packed.device)
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.W, self.S = packed.w, packed.s
        init_device(self.dev.index)
        self._lib = _lib.lib()
        self.handle = _lib.create_engine(self.cfg, getattr(packed, "fold_up", None))      # the table the buffer was laid out by
        with torch.cuda.device(self.dev):
            check(self._lib.gl_load_weights(self.handle, packed.flat.data_ptr(), packed.flat.numel(), int(packed.has_sd_conv), self._stream()),
                  "gl_load_weights")
        self._pool: Dict[Tuple, torch.Tensor] = {}
        self.cond: Optional[dict] = None
        self._cond_refs: Tuple = ()
        self._extra_ref: Optional[torch.Tensor] = None
        self.use_graphs = True

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                self._lib.gl_destroy(h)
            except Exception:
                pass

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.dev).cuda_stream

    def set_option(self, key: int, value: int) -> None:
        """Override one gl_set_option knob for THIS engine only (gl_set_handle_option): in effect while its entry points run,
        invisible to other engines and to op-level calls; its captured graphs are rebuilt on the next forward."""
        check(self._lib.gl_set_handle_option(self.handle, int(key), int(value)), "gl_set_handle_option")

    def clear_options(self) -> None:
        check(self._lib.gl_clear_handle_options(self.handle), "gl_clear_handle_options")

    # ------------------------------------------------------------------ torch-side scratch (sampler state, outputs)
    def buf(self, tag: str, shape, dtype=F16, zero: bool = False) -> torch.Tensor:
        key = (tag, tuple(shape), dtype)
        t = self._pool.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=self.dev)
            self._pool[key] = t
        return t

    def pool_bytes(self) -> int:
        """bytes of the engine's activation pool (C side) + the torch-side sampler buffers"""
        return int(self._lib.gl_pool_bytes(self.handle)) + sum(t.numel() * t.element_size() for t in self._pool.values())

    def num_launches(self) -> int:
        """kernel launches of one forward (as counted by the last eager / capture pass)"""
        return int(self._lib.gl_num_launches(self.handle))

    # ------------------------------------------------------------------ conditioning (once per image)
    @torch.no_grad()
    def set_conditioning(self, context, relations, boxes, masks, positive_embeddings, hw, text_masks=None, image_masks=None,
                         image_embeddings=None) -> None:
        """context [Bn,77,ctx], relations [Bn,R,ctx], boxes [Bn,30,4], masks [Bn,30],
        positive_embeddings [Bn,30,in_dim]: fp32 tensors (any device).  Null grounding = zeros
        (text_layout_tokinzer_input.py:47-62).  ``hw`` = latent side (64 for 512x512; gl_set_conditioning), or ``(h, w)`` = latent rows
        and columns (gl_set_conditioning_hw): each a multiple of 2^(number of downsamples), else ValueError before anything is launched.

        A text_image engine (``cfg.grounding == "text_image"``, gl_set_conditioning_ti) takes the phrase embeddings as
        ``positive_embeddings`` plus ``text_masks`` / ``image_masks`` [Bn,30] and ``image_embeddings`` [Bn,30,in_dim]
        (text_image_grounding_net.py:41); giving them to a text engine, or leaving them out of a text_image one, raises.

        An engine without the relation chain (``cfg.relation`` False, gl_unet_config.no_relation) takes ``relations=None`` and ignores a
        given tensor; on every other engine ``None`` raises ValueError before anything is launched."""
        if self.cfg.grounding == "keypoint":
            raise ValueError("a keypoint model is conditioned on points and masks (set_conditioning_kp), not on boxes and embeddings")
        if self.cfg.grounding == "spatial":
            raise ValueError("boxes given to a spatial model: it is conditioned on the tokens of its map (set_conditioning_tokens)")
        rel_on = self.cfg.relation
        if not rel_on:
            relations = None
        elif relations is None:
            raise ValueError("this model carries the rela_fuse relation chain: it needs relations [Bn, R, ctx] (only a model loaded from a "
                             "checkpoint without rela_fuse, UNetConfig.relation = False, runs without)")
        ti = self.cfg.grounding == "text_image"
        extra = (text_masks, image_masks, image_embeddings)
        if ti and any(v is None for v in extra):
            raise ValueError("a text_image model needs text_masks, image_masks and image_embeddings")
        if not ti and any(v is not None for v in extra):
            raise ValueError("text_masks / image_masks / image_embeddings given to a text-only model")
        rect = not isinstance(hw, int)
        if rect:
            h, w = (int(v) for v in hw)
            check_latent_hw(self.cfg, h, w)
        else:
            h = w = hw
        dev = self.dev
        f32 = lambda t: torch.as_tensor(t, dtype=F32).to(dev).contiguous()
        context = f32(context)
        relations = f32(relations) if rel_on else None
        boxes, masks, pe = f32(boxes), f32(masks), f32(positive_embeddings)
        Bn, mo = boxes.shape[0], boxes.shape[1]
        if mo != self.cfg.max_objs:
            raise ValueError(f"{mo} grounding slots, the model was built for {self.cfg.max_objs}")
        if context.shape[-1] != self.cfg.context_dim or (rel_on and relations.shape[-1] != self.cfg.context_dim) or pe.shape[-1] != self.cfg.pos_in_dim:
            raise ValueError("conditioning feature dims do not match the model config")
        if not (context.shape[0] == masks.shape[0] == pe.shape[0] == Bn) or (rel_on and relations.shape[0] != Bn):
            raise ValueError("conditioning batch sizes differ")
        R, Lc = (relations.shape[1] if rel_on else 0), context.shape[1]
        rel_ptr = relations.data_ptr() if rel_on else None      # NULL on an engine without the relation chain
        if ti:
            check_latent_hw(self.cfg, h, w)          # gl_set_conditioning_ti applies the _hw entry's shape rule to squares too
            tm, im, ie = f32(text_masks), f32(image_masks), f32(image_embeddings)
            if tuple(tm.shape) != tuple(masks.shape) or tuple(im.shape) != tuple(masks.shape) or tuple(ie.shape) != tuple(pe.shape):
                raise ValueError("text_masks / image_masks must match masks, image_embeddings must match the text embeddings")
            with torch.cuda.device(dev):
                check(self._lib.gl_set_conditioning_ti(self.handle, context.data_ptr(), rel_ptr, boxes.data_ptr(), masks.data_ptr(),
                                                       tm.data_ptr(), im.data_ptr(), pe.data_ptr(), ie.data_ptr(), Bn, Lc, R, h, w, self._stream()),
                      "gl_set_conditioning_ti")
            self._cond_refs = (context, relations, boxes, masks, pe, tm, im, ie)      # read asynchronously by the launched kernels
            self.cond = dict(Bn=Bn, mo=mo, R=R, Lc=Lc, hw=hw, H=h, W=w)
            return
        with torch.cuda.device(dev):
            if rect:
                check(self._lib.gl_set_conditioning_hw(self.handle, context.data_ptr(), rel_ptr, boxes.data_ptr(), masks.data_ptr(),
                                                       pe.data_ptr(), Bn, Lc, R, h, w, self._stream()), "gl_set_conditioning_hw")
            else:
                check(self._lib.gl_set_conditioning(self.handle, context.data_ptr(), rel_ptr, boxes.data_ptr(), masks.data_ptr(),
                                                    pe.data_ptr(), Bn, Lc, R, hw, self._stream()), "gl_set_conditioning")
        self._cond_refs = (context, relations, boxes, masks, pe)      # read asynchronously by the launched kernels
        self.cond = dict(Bn=Bn, mo=mo, R=R, Lc=Lc, hw=hw, H=h, W=w)

    @torch.no_grad()
    def set_conditioning_kp(self, context, points, masks, hw) -> None:
        """The conditioning of a keypoint engine (``cfg.grounding == "keypoint"``, gl_set_conditioning_kp): context [Bn,77,ctx], points
        [Bn,17P,2] (token t = keypoint t % 17 of person t // 17), masks [Bn,17P], fp32 tensors (any device); null grounding = zeros.
        ``hw``: the latent side or ``(h, w)``, under the shape rule of the rectangular entry.  On an engine of another family: ValueError."""
        if self.cfg.grounding != "keypoint":
            raise ValueError(f"points / masks given to a {self.cfg.grounding} model: keypoint grounding needs a keypoint checkpoint")
        h, w = (hw, hw) if isinstance(hw, int) else (int(v) for v in hw)
        check_latent_hw(self.cfg, h, w)
        dev = self.dev
        f32 = lambda t: torch.as_tensor(t, dtype=F32).to(dev).contiguous()
        context, points, masks = f32(context), f32(points), f32(masks)
        Bn, mo = points.shape[0], self.cfg.max_objs
        if tuple(points.shape) != (Bn, mo, 2) or tuple(masks.shape) != (Bn, mo):
            raise ValueError(f"points {tuple(points.shape)} / masks {tuple(masks.shape)}: the model was built for {self.cfg.max_persons} persons, "
                             f"[Bn, {mo}, 2] and [Bn, {mo}]")
        if context.dim() != 3 or context.shape[0] != Bn or context.shape[-1] != self.cfg.context_dim:
            raise ValueError("context does not match the batch or the model config")
        Lc = context.shape[1]
        with torch.cuda.device(dev):
            self._check(self._lib.gl_set_conditioning_kp(self.handle, context.data_ptr(), points.data_ptr(), masks.data_ptr(), Bn, Lc, h, w,
                                                         self._stream()), "gl_set_conditioning_kp")
        self._cond_refs = (context, points, masks)      # read asynchronously by the launched kernels
        self.cond = dict(Bn=Bn, mo=mo, R=0, Lc=Lc, hw=hw, H=h, W=w)

    @torch.no_grad()
    def set_conditioning_tokens(self, context, objs, hw) -> None:
        """The conditioning of a spatial engine (``cfg.grounding == "spatial"``, gl_set_conditioning_tokens): context [Bn,77,ctx] and the
        finished grounding tokens objs [Bn, n_ground, out_dim] (``spatial.SpatialTokenizer.tokens`` / ``null_tokens``), fp32 tensors (any
        device).  ``hw``: the latent side or ``(h, w)``.  On an engine of another family: ValueError."""
        if self.cfg.grounding != "spatial":
            raise ValueError(f"grounding tokens of a map given to a {self.cfg.grounding} model: spatial grounding needs a canny / hed / depth / "
                             "normal checkpoint")
        h, w = (hw, hw) if isinstance(hw, int) else (int(v) for v in hw)
        check_latent_hw(self.cfg, h, w)
        dev = self.dev
        f32 = lambda t: torch.as_tensor(t, dtype=F32).to(dev).contiguous()
        context, objs = f32(context), f32(objs)
        Bn, ng = objs.shape[0], self.cfg.n_ground
        if tuple(objs.shape) != (Bn, ng, self.cfg.pos_out_dim):
            raise ValueError(f"objs {tuple(objs.shape)}: the model takes [Bn, {ng}, {self.cfg.pos_out_dim}] grounding tokens")
        if context.dim() != 3 or context.shape[0] != Bn or context.shape[-1] != self.cfg.context_dim:
            raise ValueError("context does not match the batch or the model config")
        Lc = context.shape[1]
        with torch.cuda.device(dev):
            self._check(self._lib.gl_set_conditioning_tokens(self.handle, context.data_ptr(), objs.data_ptr(), Bn, Lc, h, w, self._stream()),
                        "gl_set_conditioning_tokens")
        self._cond_refs = (context, objs)      # read asynchronously by the launched kernels
        self.cond = dict(Bn=Bn, mo=ng, R=0, Lc=Lc, hw=hw, H=h, W=w)

    @torch.no_grad()
    def set_grounding_extra(self, extra: torch.Tensor) -> None:
        """The downsampled ``grounding_extra_input`` of a spatial model (``spatial.SpatialDownsampler``): fp32 [1 | samples, ds_out, h, w] at the
        conditioning's latent shape (gl_set_grounding_extra); the GLIGEN first conv reads cat([x, extra]), the SD conv the latent alone.  Call
        it after ``set_conditioning_tokens``, once per image."""
        if not self.cfg.ds_out:
            raise ValueError("set_grounding_extra on a model without a grounding downsampler (its first conv reads the latent alone)")
        c = self.cond
        if c is None:
            raise RuntimeError("call set_conditioning_tokens() first")
        extra = torch.as_tensor(extra, dtype=F32).to(self.dev).contiguous()
        want = (self.cfg.ds_out, c["H"], c["W"])
        if extra.dim() != 4 or tuple(extra.shape[1:]) != want or not 1 <= extra.shape[0] <= c["Bn"]:
            raise ValueError(f"downsampled grounding_extra_input {tuple(extra.shape)}: need [1 | samples, {want[0]}, {want[1]}, {want[2]}] (the "
                             "latent has to be as large as the downsampler's output)")
        with torch.cuda.device(self.dev):
            self._check(self._lib.gl_set_grounding_extra(self.handle, extra.data_ptr(), int(extra.shape[0]), self._stream()), "gl_set_grounding_extra")
        self._extra_ref = extra             # read asynchronously by the stream-ordered copy

    @torch.no_grad()
    def set_inpaint_extra(self, extra: torch.Tensor) -> None:
        """The ``inpainting_extra_input`` of an inpaint_mode model (gligen_inference.py:406-407: cat([z0 * mask, mask], dim=1)): fp32
        [1 | samples, in_channels + 1, h, w] at the conditioning's latent shape (gl_set_inpaint_extra).  The engine copies it into a pool
        buffer that its captured graphs read at replay time; call it after ``set_conditioning``, once per image (not per step)."""
        if not self.cfg.inpaint_mode:
            raise ValueError("set_inpaint_extra on a model without inpaint_mode (its first conv reads the latent alone)")
        c = self.cond
        if c is None:
            raise RuntimeError("call set_conditioning() first")
        extra = torch.as_tensor(extra, dtype=F32).to(self.dev).contiguous()
        want = (self.cfg.in_channels + 1, c["H"], c["W"])
        if extra.dim() != 4 or tuple(extra.shape[1:]) != want or not 1 <= extra.shape[0] <= c["Bn"]:
            raise ValueError(f"inpainting_extra_input {tuple(extra.shape)}: need [1 | samples, {want[0]}, {want[1]}, {want[2]}]")
        with torch.cuda.device(self.dev):
            self._check(self._lib.gl_set_inpaint_extra(self.handle, extra.data_ptr(), int(extra.shape[0]), self._stream()), "gl_set_inpaint_extra")
        self._extra_ref = extra             # read asynchronously by the stream-ordered copy

    def _check(self, code: int, what: str) -> None:
        """``check`` with the handle's gl_last_error message: the entries of an inpaint_mode handle leave one for every refusal"""
        if code != 0 and (self.cfg.inpaint_mode or self.cfg.grounding in ("keypoint", "spatial")):
            msg = _lib.last_error(self.handle)
            if msg:
                raise _lib.HipLibraryError(f"{what} failed with code {code}: {msg}")
        check(code, what)

    # ------------------------------------------------------------------ forward
    def _check_x(self, x_lat: torch.Tensor, reps: int):
        c = self.cond
        if c is None:
            raise RuntimeError("call set_conditioning() first")
        Bn, H, W = c["Bn"], c["H"], c["W"]
        if x_lat.dim() != 4 or x_lat.shape[0] * reps != Bn or tuple(x_lat.shape[-2:]) != (H, W) or x_lat.shape[1] != self.cfg.in_channels:
            raise ValueError(f"latent batch {tuple(x_lat.shape)} x reps {reps} does not match conditioning batch {Bn} @ {H} x {W}")
        if not x_lat.is_cuda or x_lat.dtype != F32 or not x_lat.is_contiguous():
            raise _lib.HipLibraryError("latent must be a contiguous fp32 GPU tensor (the HIP path has no CPU fallback)")
        return Bn, H, W

    @torch.no_grad()
    def forward(self, x_lat: torch.Tensor, t, fuser_scale: float = 1.0, sd_conv: bool = False, reps: int = 1,
                eps_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x_lat fp32 [Bn/reps, 4, h, w] (NCHW, like the reference); returns eps fp32 [Bn, 4, h, w].
        With reps=2 the latent is shared by both CFG halves of a [cond ; uncond] conditioning batch."""
        Bn, H, W = self._check_x(x_lat, reps)
        if sd_conv and not self.P.has_sd_conv:
            raise RuntimeError("SD first-conv weights were not packed")
        if eps_out is None:
            eps_out = self.buf("out.eps", (Bn, self.cfg.out_channels, H, W), F32)
        t_dev, t_host, keep = None, 0.0, None
        if torch.is_tensor(t):
            if t.numel() == 1:
                t_host = float(t.reshape(-1)[0])
            else:
                keep = t.to(self.dev, F32).reshape(-1).contiguous()
                if keep.numel() != Bn:
                    raise ValueError("timesteps must have one entry per sample")
                t_dev = keep.data_ptr()
        else:
            t_host = float(t)
        with torch.cuda.device(self.dev):
            self._check(self._lib.gl_unet_forward(self.handle, x_lat.data_ptr(), t_dev, t_host, reps, float(fuser_scale), int(bool(sd_conv)),
                                                  eps_out.data_ptr(), int(self.use_graphs), self._stream()), "gl_unet_forward")
        return eps_out

    def _check_step(self, x: torch.Tensor, reps: int, operands, required=()) -> None:
        """What the three steps check first: the evaluated latent against the conditioning, then every (name, tensor) of ``operands`` -- a
        contiguous fp32 GPU tensor of the latent's shape; None passes unless the name is in ``required``."""
        self._check_x(x, reps)
        for name, tns in operands:
            if tns is None and name in required:
                raise _lib.HipLibraryError(f"{name}: required")
            if tns is not None and (not tns.is_cuda or tns.dtype != F32 or not tns.is_contiguous() or tns.shape != x.shape):
                raise _lib.HipLibraryError(f"{name}: need a contiguous fp32 GPU tensor of the latent's shape")

    def _run_step(self, entry: str, a, t, reps, guidance, fuser_scale, sd_conv) -> None:
        """What the three steps end with, behind their own checks: the SD first-conv refusal, the fields every step struct carries
        (_lib._STEP_EVAL, use_graph), the entry under the device guard."""
        if sd_conv and not self.P.has_sd_conv:
            raise RuntimeError("SD first-conv weights were not packed")
        a.t, a.reps, a.guidance, a.fuser_scale, a.sd_conv = float(t), int(reps), float(guidance), float(fuser_scale), int(bool(sd_conv))
        a.use_graph = int(self.use_graphs)
        with torch.cuda.device(self.dev):
            self._check(getattr(self._lib, entry)(self.handle, C.byref(a), self._stream()), entry)

    @torch.no_grad()
    def plms_step(self, x_eval: torch.Tensor, x_base: torch.Tensor, x_out: torch.Tensor, e_out: torch.Tensor, e_terms: List[torch.Tensor],
                  coefs, div: float, t: float, reps: int, guidance: float, fuser_scale: float, sd_conv: bool, sqrt_at: float, s1m: float,
                  sqrt_aprev: float, dir_coef: float) -> torch.Tensor:
        """One gl_plms_step: UNet(x_eval, t) -> CFG combine into ``e_out`` -> e' = sum coefs[j] * e_terms[j] / div ->
        x_out = PLMS / DDIM(sigma 0) update of x_base (plms.py:110-163)."""
        self._check_step(x_eval, reps, [("x_eval", x_eval), ("x_base", x_base), ("x_out", x_out), ("e_out", e_out), *[("e_term", e) for e in e_terms]])
        if not 1 <= len(e_terms) <= 4 or len(coefs) != len(e_terms):
            raise ValueError("1..4 eps terms with one coefficient each")
        a = PlmsStepArgs()
        a.x_eval, a.x_base, a.x_out, a.e_out = x_eval.data_ptr(), x_base.data_ptr(), x_out.data_ptr(), e_out.data_ptr()
        for j, (e, c) in enumerate(zip(e_terms, coefs)):
            a.e_terms[j] = e.data_ptr()
            a.coef[j] = float(c)
        a.n_terms, a.div = len(e_terms), float(div)
        a.sqrt_at, a.s1m, a.sqrt_aprev, a.dir_coef = float(sqrt_at), float(s1m), float(sqrt_aprev), float(dir_coef)
        self._run_step("gl_plms_step", a, t, reps, guidance, fuser_scale, sd_conv)
        return x_out

    @torch.no_grad()
    def ddim_step(self, x: torch.Tensor, x_out: torch.Tensor, *, t: float, reps: int, guidance: float, fuser_scale: float, sd_conv: bool,
                  sqrt_at: float, s1m: float, sqrt_aprev: float, dir_coef: float, sigma: float = 0.0, noise: Optional[torch.Tensor] = None,
                  pred_x0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One gl_ddim_step: UNet(x, t) into the engine's own eps buffer, then ONE launch for the CFG combine, pred_x0 and
        x_out = sqrt_aprev * pred_x0 + dir_coef * e + sigma * noise (ddim.py:111-135).  ``x_out`` may be ``x``; ``noise`` None = the
        reference's ``0 * randn`` (skipped); ``pred_x0`` optionally receives the x0 prediction."""
        self._check_step(x, reps, [("x_out", x_out), ("noise", noise), ("pred_x0", pred_x0)])
        a = DdimStepArgs()
        a.x, a.x_out = x.data_ptr(), x_out.data_ptr()
        a.noise = None if noise is None else noise.data_ptr()
        a.pred_x0 = None if pred_x0 is None else pred_x0.data_ptr()
        a.sqrt_at, a.s1m, a.sqrt_aprev, a.dir_coef, a.sigma = float(sqrt_at), float(s1m), float(sqrt_aprev), float(dir_coef), float(sigma)
        self._run_step("gl_ddim_step", a, t, reps, guidance, fuser_scale, sd_conv)
        return x_out

    @torch.no_grad()
    def dpmpp_step(self, x: torch.Tensor, x_out: torch.Tensor, x0_out: torch.Tensor, *, t: float, reps: int, guidance: float, fuser_scale: float,
                   sd_conv: bool, sqrt_at: float, s1m: float, c_x: float, c_d: float, w1: float = 1.0, w0: float = 0.0,
                   x0_old: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One gl_dpmpp_step: UNet(x, t) into the engine's own eps buffer, then ONE launch for the CFG combine, x0 = (x - s1m * e) / sqrt_at,
        D = w1 * x0 + w0 * x0_old and x_out = c_x * x + c_d * D (DPM-Solver++(2M), host.dpm_step_coefs).  ``x_out`` may be ``x``; ``x0_out``
        receives x0 and may be ``x0_old``; ``x0_old`` None = a first-order step (``w0`` must be 0)."""
        self._check_step(x, reps, [("x_out", x_out), ("x0_out", x0_out), ("x0_old", x0_old)], required=("x_out", "x0_out"))
        if x0_old is None and w0 != 0:
            raise ValueError(f"w0 = {w0} without x0_old: a first-order step has no history term")
        a = DpmppStepArgs()
        a.x, a.x_out, a.x0_out = x.data_ptr(), x_out.data_ptr(), x0_out.data_ptr()
        a.x0_old = None if x0_old is None else x0_old.data_ptr()
        a.sqrt_at, a.s1m, a.c_x, a.c_d, a.w1, a.w0 = float(sqrt_at), float(s1m), float(c_x), float(c_d), float(w1), float(w0)
        self._run_step("gl_dpmpp_step", a, t, reps, guidance, fuser_scale, sd_conv)
        return x_out

    @torch.no_grad()
    def cfg3_eval(self, x: torch.Tensor, e_out: torch.Tensor, *, t: float, fuser_scale: float, sd_conv: bool, s_text: float,
                  s_layout: float) -> torch.Tensor:
        """One gl_cfg3_eval: UNet(x, t) over the [cond ; text-only ; uncond] conditioning batch (reps = 3) into the engine's own eps buffer,
        then ONE launch for e_out = (e_u + s_text * (e_t - e_u)) + s_layout * (e_c - e_t).  No latent is updated: ``e_out`` goes to
        ``ops.plms_update``, or to ``ops.ddim_update`` / ``ops.dpmpp_update`` as a B-sized eps."""
        self._check_step(x, 3, [("e_out", e_out)], required=("e_out",))
        a = Cfg3EvalArgs()
        a.x, a.e_out = x.data_ptr(), e_out.data_ptr()
        a.s_text, a.s_layout = float(s_text), float(s_layout)
        self._run_step("gl_cfg3_eval", a, t, 3, s_text, fuser_scale, sd_conv)      # (guidance: not read by the entry)
        return e_out
