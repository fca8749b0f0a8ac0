"""fp32 CPU restatement of the DDIM sampler loop (GLIGEN/ldm/models/diffusion/ddim.py:65-135) over an ``eps_fn`` -- test infrastructure in the
style of oracle/plms_ref.py and tests/norel_ref.py: the denoiser is passed in, so this file pins the *sampler* arithmetic and its RNG order
independently of the UNet.

Pinned by tests/test_ddim_host.py against latents produced by the reference's own DDIMSampler (tools/make_ddim_goldens.py), with the
reference's noise draws replayed; it serves what has no reference run (classifier-free guidance on the relation UNet, rectangular latents).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from layoutllm_t2i_amd import host
from oracle import plms_ref


def ddim_sample(eps_fn: Callable[[torch.Tensor, torch.Tensor, int, float], torch.Tensor], x: torch.Tensor, sched, alpha_type=None,
                mask: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None, acp64: Optional[np.ndarray] = None) -> torch.Tensor:
    """DDIM loop over ``sched`` (host.make_ddim_schedule).

    ``eps_fn(x, t_long[B], step_index_i, fuser_alpha)`` returns the *guided* epsilon, as for oracle.plms_ref.plms_sample.  Noise comes from
    ``torch.randn_like`` (patch it to replay recorded draws): per step q_sample's draw on ``x0`` when a mask is given (ddim.py:101-105,
    ldm.py:19-22), then one draw of the latent's shape, taken when sigma is 0 too (ddim.py:132).  ``acp64``: the float64 alphas_cumprod of
    q_sample's two coefficient tables (default: the linear schedule's)."""
    ts = sched["ddim_timesteps"]
    time_range = np.flip(ts)
    total = ts.shape[0]
    alphas = plms_ref.alpha_generator(len(time_range), alpha_type)
    b = x.shape[0]
    if mask is not None:
        assert x0 is not None
        if acp64 is None:
            acp64 = np.cumprod(1.0 - (torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2).numpy(), axis=0)
        sac, s1ac = np.sqrt(acp64).astype(np.float32), np.sqrt(1.0 - acp64).astype(np.float32)
    for i, step in enumerate(time_range):
        index = total - i - 1
        t = torch.full((b,), int(step), dtype=torch.long)
        if mask is not None:
            img_orig = float(sac[int(step)]) * x0 + float(s1ac[int(step)]) * torch.randn_like(x0)
            x = img_orig * mask + (1. - mask) * x
        e = eps_fn(x, t, i, alphas[i])
        # the five scalars as float32 (host.ddim_step_coefs: numpy float32 square roots, IEEE correctly rounded like the reference's)
        sqrt_at, s1m, sqrt_aprev, dir_coef, sigma = (torch.full((b, 1, 1, 1), v) for v in host.ddim_step_coefs(sched, index))
        pred_x0 = (x - s1m * e) / sqrt_at
        dir_xt = dir_coef * e
        noise = sigma * torch.randn_like(x)
        x = sqrt_aprev * pred_x0 + dir_xt + noise
    return x
