"""The two samplers with the reference's call surface: PLMS (GLIGEN/ldm/models/diffusion/plms.py:10-163) and DDIM with eta
(GLIGEN/ldm/models/diffusion/ddim.py:9-135); and one the reference does not have, DPM-Solver++(2M) (``DPMSolverSampler``, below).

    PLMSSampler(diffusion, model, alpha_generator_func=..., set_alpha_scale=...)
        .sample(S, shape, input, uc, guidance_scale, mask=None, x0=None) -> latent
    DDIMSampler(diffusion, model, alpha_generator_func=..., set_alpha_scale=..., eta=0.0, discretize="uniform")
        .sample(S, shape, input, uc, guidance_scale, mask=None, x0=None) -> latent
    DPMSolverSampler(diffusion, model, alpha_generator_func=..., set_alpha_scale=..., order=2, discretize="logsnr")
        .sample(S, shape, input, uc, guidance_scale, mask=None, x0=None) -> latent
    every class: .sample_from(S, shape, input, uc, guidance_scale, init_latent, strength, mask=None, x0=None, layout_guidance_scale=None)
        -> latent: image-to-image (SDEdit), the schedule's tail from the noised ``init_latent`` (not in the reference; see the method)

Same loops, same side effects (per-step fuser scale via set_alpha_scale, permanent SD first-conv switch on every scale-0 step; PLMS: step-0
double evaluation, Adams-Bashforth history of <= 3 eps), but:

  * cond + uncond run as ONE 2B-sized UNet evaluation (result-identical per sample): the
    conditioning batch is [real grounding + prompt ; null grounding + ""], hoisted once per image;
  * PLMS: the CFG combine and the x_prev update are two tiny fused HIP kernels on fp32 latents; DDIM: ONE kernel (gl_ddim_update) reads the 2B
    output and does the combine, pred_x0 and x_prev.  Both evaluate in the reference's operation order (bit-identical to torch fp32 given
    the same eps);
  * DPM-Solver++(2M): ONE kernel too (gl_dpmpp_update: the combine, the x0 prediction, the multistep difference with the x0 of the step
    before, x_prev), bit-identical to the torch fp32 expression; its history is one buffer;
  * the schedule tables are computed once per S (DDIM: per (S, discretisation, eta); DPM-Solver++: per (S, discretisation));
  * an inpaint_mode model's ``input["inpainting_extra_input"]`` (the same tensor for the cond and the uncond pass, plms.py:118-121) is handed
    to the engine once per ``sample()``, not per step;
  * a map model (canny / hed / depth / normal, sem) takes ``input["grounding_extra_input"]`` (required there, ignored elsewhere): its tokenizer
    runs once per ``sample()``, the unconditional half takes the cached null tokens, both halves read the same extra (UNetModel.condition);
  * inpainting (``mask`` / ``x0``, plms.py:95-99, ddim.py:101-105): each step first replaces the known region,
    x = q_sample(x0, t) * mask + (1 - mask) * x, as one fused in-place fp32 HIP kernel (gl_latent_blend, bit-identical to
    the torch expression), with the q_sample noise drawn by ``torch.randn_like(x0)`` before the step's own draws.

Separate text and layout scales (every class: ``.sample_layout(S, shape, input, uc, guidance_scale, layout_guidance_scale, mask=None, x0=None)``,
not in the reference; ``sample()`` keeps the reference's parameter list): the conditioning batch becomes [cond ; text-only ; uncond],
one step = ``Engine.cfg3_eval`` (the 3B evaluation + gl_cfg3_combine: e = (e_u + s_t (e_t - e_u)) + s_l (e_c - e_t)) into a guided-eps buffer,
then the sampler's op-level update (``ops.plms_update``, ``ops.ddim_update`` / ``ops.dpmpp_update`` on a B-sized eps) -- same coefficients,
history and RNG draws as the two-branch step.  Where a step cannot see the grounding (fuser scale 0 on a model without the relation chain)
e_c == e_t, and the sampler issues the existing two-branch step on [cond ; uncond] instead (``_Sampler._needs_text_branch``).

One path: ``_Sampler`` owns ``sample()``, the loop, the schedule cache and what every step does first (the hoisted conditioning, the running
latent, the per-step fuser scale and first-conv switch, the masked blend); a class adds its schedule tables, what it allocates before the loop
and one step.  The switch is stated once as well: one ``SamplerSpec`` record per sampler (its ``args`` keys with defaults, validators and the
constructor keyword each feeds, and what it refuses of the others' keys) in ``SAMPLER_TABLE``, read by ``resolve_sampler`` -- the only place
that turns the per-call keys into a class and its keywords; interface.py, gligen_inference.py, txt2img.py and train_rl.py go through it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np
import torch

from . import host, ops


class _Sampler(object):
    """``sample()``, the loop and the schedule cache of every sampler.  A subclass supplies ``tag`` (the prefix of its engine buffers),
    ``make_schedule`` with its own signature and refusals (it hands ``_schedule`` a key and the tables' maker), ``_sample_schedule`` (what
    ``sample()`` passes to ``make_schedule`` behind S), ``_alloc`` (what it allocates before the loop) and ``_step`` (one step)."""
    tag = None
    _sample_schedule = ()
    _guided_eps = None          # set per step by _sampling under three-branch guidance

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None):
        self.diffusion = diffusion
        self.model = model
        self.device = model.device if hasattr(model, "device") else diffusion.betas.device
        self.ddpm_num_timesteps = diffusion.num_timesteps
        self.schedule = schedule
        self.alpha_generator_func = alpha_generator_func
        self.set_alpha_scale = set_alpha_scale
        self._sched_key = None

    def _schedule(self, key, make) -> None:
        """the one schedule cache: ``make()`` gives the tables of ``key`` unless they are the ones in place"""
        if self._sched_key != key:
            self._set_tables(make())
            self._sched_key = key

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None):
        self.make_schedule(S, *self._sample_schedule)
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    @torch.no_grad()
    def sample_layout(self, S, shape, input, uc, guidance_scale, layout_guidance_scale, mask=None, x0=None):
        """``sample()`` with the layout's own guidance scale (``_sampling``'s ``layout_guidance_scale``; None: ``sample()`` exactly).  A
        method of its own: ``sample()`` keeps the reference's parameter list."""
        self.make_schedule(S, *self._sample_schedule)
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0, layout_guidance_scale=layout_guidance_scale)

    @torch.no_grad()
    def sample_from(self, S, shape, input, uc, guidance_scale, init_latent, strength, mask=None, x0=None, layout_guidance_scale=None):
        """Image-to-image (SDEdit, Meng et al., arXiv 2108.01073): ``sample()`` / ``sample_layout()`` started from ``init_latent`` (fp32
        [1|B, C, h, w], the encoded image) noised to a timestep inside the schedule, instead of from pure noise at its top.  Of the n nodes
        of the schedule ``S`` gives this sampler, the last ``host.img2img_run_steps(n, strength)`` run; ``strength`` in (0, 1], 1 = all of
        them (the image then only shifts the starting noise by sqrt(acp[t_top]) * init_latent).  ``input["x"]`` is the noise the image is
        mixed with (drawn here when None, like ``sample()``'s starting latent); the start itself draws nothing.

        ``alpha_generator_func`` is asked for the number of steps that RUN, so the fuser schedule (``alpha_type``) spans them: taking the tail
        of the full schedule's scales instead would leave a [0.3, 0, 0.7] run at strength 0.5 with the grounding switched off on every step,
        and the layout ignored.  PLMS starts its history empty (the first step that runs evaluates twice), DPM-Solver++ starts first order
        and counts the nodes that run for its lower-order final step; the masked blend and three-branch guidance belong to the loop and
        compose unchanged."""
        self.make_schedule(S, *self._sample_schedule)
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0, layout_guidance_scale=layout_guidance_scale,
                              init_latent=init_latent, strength=strength)

    @torch.no_grad()
    def _sampling(self, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, layout_guidance_scale=None, init_latent=None, strength=None):
        """The loop over the schedule in place (``plms_sampling`` / ``ddim_sampling`` / ``dpm_sampling`` by the classes' own names).
        ``layout_guidance_scale``: None = one scale for text and layout, the [cond ; uncond] batch; a number = the layout's own scale s_l
        next to s_t = ``guidance_scale`` (three-branch guidance, see ``_needs_text_branch``).  ``init_latent`` + ``strength``: both or
        neither; the loop runs the schedule's tail from the noised ``init_latent`` (``sample_from``)."""
        layout = layout_guidance_scale
        if layout is not None and uc is None:
            raise ValueError("layout_guidance_scale needs uc, the unconditional context: the text-only and the unconditional branch are "
                             "evaluated whatever guidance_scale is")
        if (init_latent is None) != (strength is None):
            raise ValueError("strength needs init_latent, the latent of the image to start from" if init_latent is None else
                             "init_latent needs strength, the share of the schedule to run")
        x_a, reps, time_range, alphas, blend = self._begin(self.tag, shape, input, uc, guidance_scale, mask, x0, layout is not None,
                                                           init_latent=init_latent, strength=strength)
        model = self.model
        total_steps = len(time_range)           # the nodes that run: the whole schedule, or its tail under image-to-image
        state = self._alloc(x_a)

        def at(t):
            """the evaluation's arguments of an engine step at timestep ``t``, read when the step is issued"""
            return dict(t=float(int(t)), reps=reps, guidance=float(guidance_scale), fuser_scale=model.fuser_scale, sd_conv=model.use_sd_conv)

        def guided_eps(x_eval, t, e_out=None):
            """one three-branch evaluation at timestep ``t``: the guided eps into ``e_out`` (default: the buffer ``<tag>.e3``)"""
            if e_out is None:
                e_out = model.engine.buf(f"{self.tag}.e3", tuple(x_a.shape), torch.float32)
            return model.engine.cfg3_eval(x_eval, e_out, t=float(int(t)), fuser_scale=model.fuser_scale, sd_conv=model.use_sd_conv,
                                          s_text=float(guidance_scale), s_layout=float(layout))

        self._guided_eps = None         # what a step reads: None = the fused two-branch step, else the evaluation its op-level update follows
        try:
            for i, step in enumerate(time_range):
                self._step_prologue(i, step, alphas, blend)
                if layout is not None:
                    want = 3 if self._needs_text_branch(model.fuser_scale) else 2
                    if want != reps:            # the conditioning form in place is the other one: once per image with [0.3, 0, 0.7]
                        reps = model.condition(input, uc, always_extra=True, text_branch=want == 3)
                    self._guided_eps = guided_eps if reps == 3 else None
                self._step(state, x_a, at, i, time_range, total_steps - i - 1)
        finally:
            self._guided_eps = None
        input["x"] = x_a.clone()
        return input["x"]

    def _needs_text_branch(self, fuser_scale) -> bool:
        """Whether a step at this fuser scale needs the text-only branch.  Without the relation chain a scale-0 step skips the fuser, the only
        reader of the grounding: e_c == e_t there, the layout term vanishes and [cond ; uncond] with ``guidance_scale`` is the whole
        formula.  The relation chain reads the boxes at every scale, so a relation model always runs three branches."""
        return bool(self.model.cfg.relation) or fuser_scale != 0

    def _alloc(self, x_a):
        return None

    def _acp(self) -> np.ndarray:
        acp = self.diffusion.alphas_cumprod.detach().cpu().numpy().astype(np.float32)
        assert acp.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        return acp

    def _set_tables(self, s) -> None:
        self.ddim_timesteps = s["ddim_timesteps"]
        self.ddim_alphas = s["ddim_alphas"]
        self.ddim_alphas_prev = s["ddim_alphas_prev"]
        self.ddim_sqrt_one_minus_alphas = s["ddim_sqrt_one_minus_alphas"]
        self.ddim_sigmas = s["ddim_sigmas"]
        self._sched = s

    def _begin(self, tag, shape, input, uc, guidance_scale, mask, x0, layout=False, init_latent=None, strength=None):
        """Everything before the loop: the starting latent in the engine buffer ``<tag>.x``, the conditioning hoisted once, the fuser scales of
        the steps and the masked blend of one step (None without a mask).  ``layout``: three-branch guidance -- the conditioning takes the form
        the first step needs.  ``init_latent`` / ``strength`` (image-to-image): ``time_range`` is the tail of the schedule that runs and the
        starting latent q_sample(init_latent, time_range[0]) with ``input["x"]`` as its noise, one gl_q_sample launch into ``<tag>.x``.
        Returns (x_a, reps, time_range, alphas, blend)."""
        if mask is not None and x0 is None:
            raise AssertionError("a mask needs x0, the latent of the image to keep (plms.py:96)")       # before the model is touched
        if strength is not None:
            strength = host.check_strength(strength)
        model, eng = self.model, self.model.engine
        dev = self.device
        b = shape[0]
        img = input["x"]
        if img is None:
            img = torch.randn(shape, device=dev)
            input["x"] = img
        x = img.to(dev, torch.float32).contiguous().clone()

        time_range = np.flip(self.ddim_timesteps)
        init_d = None
        if init_latent is not None:
            if not torch.is_tensor(init_latent) or init_latent.dtype != torch.float32 or init_latent.dim() != 4 or \
                    init_latent.shape[1:] != x.shape[1:] or init_latent.shape[0] not in (1, x.shape[0]):
                got = f"{init_latent.dtype} {tuple(init_latent.shape)}" if torch.is_tensor(init_latent) else type(init_latent).__name__
                raise ValueError(f"init_latent must be fp32 [1|{x.shape[0]}, {tuple(x.shape[1:])}], got {got}")
            init_d = init_latent.to(dev, torch.float32).contiguous()
            n = len(time_range)
            time_range = time_range[n - host.img2img_run_steps(n, strength):]       # the last n_run nodes; step i reads table index n_run - i - 1
        alphas = self.alpha_generator_func(len(time_range)) if self.alpha_generator_func is not None else None

        # ---- conditioning, once per image: [cond ; uncond] when CFG is active (plms.py:115-124)
        # every missing input raises before any kernel runs; the grounding extra of a map family is handed over whatever conv is switched in
        if layout:
            first = alphas[0] if alphas is not None and len(alphas) else model.fuser_scale
            reps = model.condition(input, uc, always_extra=True, text_branch=self._needs_text_branch(first))
        else:
            reps = model.condition(input, uc if uc is not None and guidance_scale != 1 else None, always_extra=True)

        x_a = eng.buf(f"{tag}.x", tuple(x.shape), torch.float32)    # running latent (the engine copies it per forward)
        if init_d is None:
            x_a.copy_(x)
        else:
            # q_sample(init_latent, t0) with the caller's noise; the coefficients from the fp32 buffers, as the blend reads them (ldm.py:19-22)
            t0 = int(time_range[0])
            sac = self.diffusion.sqrt_alphas_cumprod.detach().cpu().numpy()
            s1ac = self.diffusion.sqrt_one_minus_alphas_cumprod.detach().cpu().numpy()
            ops.q_sample(init_d, x, float(sac[t0]), float(s1ac[t0]), out=x_a)

        blend = None
        if mask is not None:
            # q_sample coefficients of every step, read from the fp32 buffers (ldm.py:19-22); the x0 / mask operands, once
            sac = self.diffusion.sqrt_alphas_cumprod.detach().cpu().numpy()
            s1ac = self.diffusion.sqrt_one_minus_alphas_cumprod.detach().cpu().numpy()
            x0_d = x0.to(dev, torch.float32).contiguous()
            mask_d = mask.to(dev, torch.float32).contiguous()
            if x0_d.shape[1:] != x.shape[1:] or x0_d.shape[0] not in (1, b) or tuple(mask_d.shape[1:]) != (1,) + tuple(x.shape[2:]) \
                    or mask_d.shape[0] not in (1, b):
                raise ValueError(f"x0 must be [1|{b}, {tuple(x.shape[1:])}] and mask [1|{b}, 1, {tuple(x.shape[2:])}], got "
                                 f"{tuple(x0.shape)} and {tuple(mask.shape)}")

            def blend(step):
                # plms.py:95-99: img = q_sample(x0, ts) * mask + (1 - mask) * img; the noise is randn_like(x0) on x0's device
                noise = torch.randn_like(x0).to(dev, torch.float32).contiguous()
                ops.latent_blend(x_a, x0_d, noise, mask_d, float(sac[int(step)]), float(s1ac[int(step)]))
        return x_a, reps, time_range, alphas, blend

    def _step_prologue(self, i, step, alphas, blend) -> None:
        """what every step does before it evaluates the UNet: the fuser scale, the permanent first-conv switch, the masked blend"""
        if alphas is not None:
            self.set_alpha_scale(self.model, alphas[i])
            if alphas[i] == 0:
                self.model.restore_first_conv_from_SD()
        if blend is not None:
            blend(step)


class PLMSSampler(_Sampler):
    tag = "plms"
    plms_sampling = _Sampler._sampling

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None):
        super().__init__(diffusion, model, schedule, alpha_generator_func, set_alpha_scale)
        self.mirror_rng = True     # plms.py:138 draws randn_like(x) * 0 on every update

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=False):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        if ddim_discretize != "uniform":
            raise NotImplementedError(ddim_discretize)
        self._schedule((ddim_num_steps,), lambda: host.make_schedule(ddim_num_steps, self._acp()))

    def _alloc(self, x_a):
        eng = self.model.engine
        ring = [eng.buf(f"plms.e{j}", tuple(x_a.shape), torch.float32) for j in range(4)]
        # old: the eps history, newest last, <= 3 entries; its tensors and the free ones are slots of `ring`
        return dict(x_mid=eng.buf("plms.xmid", tuple(x_a.shape), torch.float32), old=[], free=list(ring))

    def _step(self, st, x_a, at, i, time_range, index):
        old, free = st["old"], st["free"]

        def step_eval(x_eval, t_val, e_out, e_terms, coefs, div, x_out):
            """one gl_plms_step: UNet (2B batch) -> CFG combine into e_out -> e' -> x_out = update of x_a"""
            sq_at, s1m, sq_ap, dirc = host.step_coefs(self._sched, index)
            if self.mirror_rng:
                torch.randn_like(x_a)          # plms.py:138 draws noise * sigma (= 0) on every update: keep the RNG stream aligned
            if self._guided_eps is not None:
                # three branches: the guided eps into the same slot, then the op-level update over the same terms
                self._guided_eps(x_eval, t_val, e_out)
                ops.plms_update(x_a, e_terms[0], e_terms[1:], coefs, div, sq_at, s1m, sq_ap, dirc, x_out)
                return
            a = at(t_val)              # plms_step takes its arguments by position: callers wrap it with that signature
            self.model.engine.plms_step(x_eval, x_a, x_out, e_out, e_terms, coefs, div, a["t"], a["reps"], a["guidance"], a["fuser_scale"],
                                        a["sd_conv"], sq_at, s1m, sq_ap, dirc)

        e_t = free.pop()
        if len(old) == 0:
            # step 0 evaluates twice (plms.py:144-150): x_mid from e_t alone, then e' = (e_t + e(x_mid, t_next)) / 2
            step_eval(x_a, time_range[i], e_t, [e_t], (1.0,), 1.0, st["x_mid"])
            e_next = free[-1]                                   # scratch slot, not kept
            coefs, div = host.PLMS_COEFS[0]
            step_eval(st["x_mid"], time_range[min(i + 1, len(time_range) - 1)], e_next, [e_t, e_next], coefs, div, x_a)
        else:
            coefs, div = host.PLMS_COEFS[min(len(old), 3)]
            step_eval(x_a, time_range[i], e_t, [e_t] + old[::-1][:len(coefs) - 1], coefs, div, x_a)
        old.append(e_t)
        if len(old) >= 4:
            free.append(old.pop(0))


class DDIMSampler(_Sampler):
    """ddim.py:9-135 on the HIP engine.  One step = one 2B UNet evaluation + ONE kernel (``Engine.ddim_step``).

    Two deliberate differences from the reference:

      * ``sample()`` samples with the constructor's ``eta`` and ``discretize``.  The reference's ``sample()`` re-makes the schedule with its
        defaults on every call (ddim.py:56), so eta > 0 and "quad" are only reachable there through ``make_schedule`` + ``ddim_sampling``
        -- which work here the same way.
      * classifier-free guidance runs on a model with the relation chain.  The reference builds its unconditional input without
        ``"relations"`` (ddim.py:116) and fails in the relation UNet (``KeyError: 'relations'``, openaimodel.py:444); here the unconditional
        half reads the same relations as the conditional one, as plms.py:121 has it.

    RNG order per step, as in the reference: with a mask ``torch.randn_like(x0)`` (q_sample) first, then one ``torch.randn_like`` of the
    latent's shape -- drawn when sigma is 0 too (ddim.py:132 multiplies it by 0) and then not handed to the kernel."""
    tag = "ddim"
    ddim_sampling = _Sampler._sampling

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None, eta=0.0, discretize="uniform"):
        super().__init__(diffusion, model, schedule, alpha_generator_func, set_alpha_scale)
        self.eta = host.check_ddim_eta(eta)
        if discretize not in host.DDIM_DISCRETIZE:
            raise ValueError(f"ddim_discretize = {discretize!r}: one of {host.DDIM_DISCRETIZE}")
        self.discretize = discretize
        # unlike the reference's, sample() does NOT reset eta to 0 (nor the discretisation to "uniform"): it uses the constructor's
        self._sample_schedule = (self.discretize, self.eta)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.):
        self._schedule((int(ddim_num_steps), ddim_discretize, float(ddim_eta)),
                       lambda: host.make_ddim_schedule(ddim_num_steps, self._acp(), ddim_discretize, ddim_eta))

    def _step(self, st, x_a, at, i, time_range, index):
        sq_at, s1m, sq_ap, dirc, sigma = host.ddim_step_coefs(self._sched, index)
        noise = torch.randn_like(x_a)      # ddim.py:132 draws on every step, sigma 0 included: keep the RNG stream aligned
        if self._guided_eps is not None:
            ops.ddim_update(self._guided_eps(x_a, time_range[i]), x_a, x_a, sqrt_at=sq_at, s1m=s1m, sqrt_aprev=sq_ap, dir_coef=dirc, sigma=sigma,
                            noise=noise.to(self.device, torch.float32).contiguous() if sigma != 0 else None)
            return
        self.model.engine.ddim_step(x_a, x_a, **at(time_range[i]), sqrt_at=sq_at, s1m=s1m, sqrt_aprev=sq_ap, dir_coef=dirc, sigma=sigma,
                                    noise=noise.to(self.device, torch.float32).contiguous() if sigma != 0 else None)


class DPMSolverSampler(_Sampler):
    """DPM-Solver++(2M) (Lu et al., arXiv 2211.01095, Algorithm 2: the data-prediction multistep solver) on the HIP engine -- not in the
    reference.  One step = one 2B UNet evaluation + ONE kernel (``Engine.dpmpp_step``):

        x0 = (x - s1m * e) / sqrt_at;  D = w1 * x0 + w0 * x0_old;  x_prev = c_x * x + c_d * D       (host.dpm_step_coefs)

    The steps sit on the half log-SNR grid by default (``discretize`` "logsnr"; "uniform" / "quad" are DDIM's timesteps without repeats), so
    ``S`` steps are n <= S evaluations; ``alpha_generator_func`` gets n.  ``order`` 2: the first step, and the last one of fewer than 15, are
    first order; ``order`` 1 is DDIM with eta 0 in exponential-integrator form.  The history is ONE engine buffer, ``dpmpp.x0`` (the kernel
    reads the old x0 and writes the new one in place).  The sampler draws no noise: without a mask the result does not depend on the torch
    seed; with one, the only draw of a step is the blend's ``torch.randn_like(x0)``.  Everything in ``_Sampler`` is inherited unchanged."""
    tag = "dpmpp"
    dpm_sampling = _Sampler._sampling

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None, order=2, discretize="logsnr"):
        super().__init__(diffusion, model, schedule, alpha_generator_func, set_alpha_scale)
        if isinstance(order, bool) or order not in host.DPM_ORDERS:
            raise ValueError(f"dpm_order = {order!r}: one of {host.DPM_ORDERS}")
        if discretize not in host.DPM_DISCRETIZE:
            raise ValueError(f"dpm_discretize = {discretize!r}: one of {host.DPM_DISCRETIZE}")
        self.order = int(order)
        self.discretize = discretize

    def make_schedule(self, num_steps, discretize=None):
        discretize = self.discretize if discretize is None else discretize
        self._schedule((int(num_steps), discretize), lambda: host.make_dpm_schedule(num_steps, self._acp(), discretize))

    def _alloc(self, x_a):
        # hist: the x0 prediction of the step before, rewritten in place; prev: that step's node
        return dict(hist=self.model.engine.buf("dpmpp.x0", tuple(x_a.shape), torch.float32), prev=None)

    def _step(self, st, x_a, at, i, time_range, index):
        sq_at, s1m, c_x, c_d, w1, w0 = host.dpm_step_coefs(self._sched, index, st["prev"], self.order, n_nodes=len(time_range))
        if self._guided_eps is not None:
            ops.dpmpp_update(self._guided_eps(x_a, time_range[i]), x_a, x_a, st["hist"], sqrt_at=sq_at, s1m=s1m, c_x=c_x, c_d=c_d, w1=w1, w0=w0,
                             x0_old=st["hist"] if w0 != 0 else None)
        else:
            self.model.engine.dpmpp_step(x_a, x_a, st["hist"], **at(time_range[i]), sqrt_at=sq_at, s1m=s1m, c_x=c_x, c_d=c_d, w1=w1, w0=w0,
                                         x0_old=st["hist"] if w0 != 0 else None)
        st["prev"] = index


# ------------------------------------------------------------------------------------------- the switch: one record per sampler
@dataclass(frozen=True)
class Key:
    name: str                                    # the per-call ``args`` key
    default: object
    kwarg: str                                   # the constructor keyword it feeds
    check: Callable                              # value -> the validated value, or ValueError naming the key


@dataclass(frozen=True)
class SamplerSpec:
    name: str                                    # args["sampler"]
    cls: type
    keys: Tuple[Key, ...] = ()                   # the args keys it owns
    refuses: Tuple[Tuple[Tuple[str, ...], str], ...] = ()     # (keys of another sampler, the message when one of them is off its default)

    def kwargs(self, values) -> dict:
        """the constructor keywords out of resolve_sampler's values"""
        return {k.kwarg: values[k.name] for k in self.keys}


def _one_of(key, choices):
    def check(v):
        if v not in choices:
            raise ValueError(f"{key} = {v!r}: one of {choices}")
        return v
    return check


def _dpm_order(v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v not in host.DPM_ORDERS:
        raise ValueError(f"dpm_order = {v!r}: one of {host.DPM_ORDERS}")
    return int(v)


# the wording of the cross-sampler refusals is irregular and kept as text
_NEEDS_DPM = ((("dpm_order",), "dpm_order = {dpm_order} with sampler = {sampler!r}: it needs sampler = 'dpmpp_2m'"),
              (("dpm_discretize",), "dpm_discretize = {dpm_discretize!r} with sampler = {sampler!r}: it needs sampler = 'dpmpp_2m'"))
DEFAULT_SAMPLER = "plms"
SAMPLER_TABLE = {s.name: s for s in (         # in the order the samplers arrived, which is the order of the refusals
    SamplerSpec("plms", PLMSSampler, refuses=(
        (("ddim_eta", "ddim_discretize"), "ddim_eta = {ddim_eta} / ddim_discretize = {ddim_discretize!r} with sampler = 'plms': PLMS is "
                                          "deterministic on uniform steps; eta and 'quad' need sampler = 'ddim'"),) + _NEEDS_DPM),
    SamplerSpec("ddim", DDIMSampler, keys=(Key("ddim_eta", 0.0, "eta", host.check_ddim_eta),
                                           Key("ddim_discretize", "uniform", "discretize", _one_of("ddim_discretize", host.DDIM_DISCRETIZE))),
                refuses=_NEEDS_DPM),
    SamplerSpec("dpmpp_2m", DPMSolverSampler, keys=(Key("dpm_order", 2, "order", _dpm_order),
                                                   Key("dpm_discretize", "logsnr", "discretize", _one_of("dpm_discretize", host.DPM_DISCRETIZE))),
                refuses=((("ddim_eta",), "ddim_eta = {ddim_eta} with sampler = 'dpmpp_2m': the solver is deterministic; eta needs sampler = 'ddim'"),
                         (("ddim_discretize",), "ddim_discretize = {ddim_discretize!r} with sampler = 'dpmpp_2m': its grid is args[\"dpm_discretize\"]"))),
)}
SAMPLERS = tuple(SAMPLER_TABLE)                                                        # ("plms", "ddim", "dpmpp_2m")
SAMPLER_KEYS = ("sampler",) + tuple(k.name for s in SAMPLER_TABLE.values() for k in s.keys)      # every per-call key of the switch


def resolve_sampler(keys, upto=None) -> Tuple[SamplerSpec, dict]:
    """The sampler switch, checked in one place before any encoder or kernel runs.  ``keys``: a mapping that may hold any of SAMPLER_KEYS (a
    whole ``args`` dict will do; what is absent is at its default).  Returns the sampler's record and every key's validated value by name
    (``spec.kwargs(values)``: the constructor's keywords).  ValueError, in this order: an unknown sampler; then per sampler of the table its
    own keys' values (eta negative or not finite, an unknown discretisation, an order that is no int of DPM_ORDERS), followed by the refusals
    between that sampler and the ones before it -- a key off its default under a sampler that does not own it.  ``upto``: stop behind that
    sampler's stage, leaving the later samplers' keys unjudged and out of the values (interface.check_sampler_args, which stops at "ddim")."""
    name = keys.get("sampler", DEFAULT_SAMPLER)
    if name not in SAMPLERS:
        raise ValueError(f"sampler = {name!r}: one of {SAMPLERS}")
    spec = SAMPLER_TABLE[name]
    values, defaults, pending, chosen = {"sampler": name}, {}, list(spec.refuses), False
    for owner in SAMPLER_TABLE.values():
        for k in owner.keys:
            values[k.name], defaults[k.name] = k.check(keys.get(k.name, k.default)), k.default
        chosen = chosen or owner is spec
        for refusal in [r for r in pending if chosen and all(k in values for k in r[0])]:
            pending.remove(refusal)
            if any(values[k] != defaults[k] for k in refusal[0]):
                raise ValueError(refusal[1].format(**values))
        if owner.name == upto:
            break
    return spec, values
