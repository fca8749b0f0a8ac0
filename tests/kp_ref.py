"""fp32 CPU restatement of the keypoint PositionNet (keypoint_grounding_net.py:34-58), test infrastructure like tests/ti_ref.py: built on
the pieces of oracle/unet_ref.py (``fourier_embed``, ``_lin``), and ``unet_forward`` runs the upstream-block UNet of tests/norel_ref.py with
``oracle.unet_ref.position_net`` patched for the call -- the UNet handles the 17 P tokens unchanged.

Pinned to the reference's own outputs (tests/golden/kp_*.npz, tools/make_kp_goldens.py) by tests/test_kp_host.py.
"""
from __future__ import annotations

from unittest import mock

import torch
import torch.nn.functional as F

import norel_ref
from oracle import unet_ref

KEYS = ("points", "masks")


def mlp_input(sd, points, masks, num_freqs: int = 8) -> torch.Tensor:
    """[B, 17 P, D + 4 F]: the table sum first, then the blends (keypoint_grounding_net.py:39-56)"""
    p = "position_net"
    pe, ke = sd[p + ".person_embeddings"], sd[p + ".keypoint_embeddings"]
    P = pe.shape[0]
    m = masks.unsqueeze(-1)
    person = (pe.unsqueeze(1).repeat(1, 17, 1).reshape(P * 17, -1) + torch.cat([ke] * P, dim=0)).unsqueeze(0).repeat(points.shape[0], 1, 1)
    xy = unet_ref.fourier_embed(points, num_freqs)
    person = person * m + (1 - m) * sd[p + ".null_person_feature"].view(1, 1, -1)
    xy = xy * m + (1 - m) * sd[p + ".null_xy_feature"].view(1, 1, -1)
    return torch.cat([person, xy], dim=-1)


def position_net(sd, points, masks, num_freqs: int = 8) -> torch.Tensor:
    p = "position_net"
    h = mlp_input(sd, points, masks, num_freqs)
    h = F.silu(unet_ref._lin(sd, p + ".linears.0", h))
    h = F.silu(unet_ref._lin(sd, p + ".linears.2", h))
    return unet_ref._lin(sd, p + ".linears.4", h)


def unet_forward(sd, cfg, x, timesteps, context, grounding, fuser_scale: float = 1.0, first_conv=None) -> torch.Tensor:
    """UNetModel.forward on the upstream block with the keypoint PositionNet; ``grounding``: points and masks (null grounding = zeros)."""
    objs = position_net(sd, grounding["points"], grounding["masks"], cfg.fourier_freqs)
    text = dataclasses_text(cfg)
    with mock.patch.object(unet_ref, "position_net", lambda *a, **k: objs):
        return norel_ref.unet_forward(sd, text, x, timesteps, context, dict(boxes=None, masks=None, positive_embeddings=None),
                                      fuser_scale=fuser_scale, first_conv=first_conv)


def dataclasses_text(cfg):
    """the config as norel_ref dispatches on it: the text branch, whose position_net is the patched one"""
    import dataclasses
    return dataclasses.replace(cfg, grounding="text")


def null_grounding(grounding):
    return {k: torch.zeros_like(grounding[k]) for k in KEYS}


def make_eps_fn(sd, cfg, inp, guidance, first_conv_sd):
    """Guided epsilon for oracle.plms_ref.plms_sample with the sampler's side effects (fuser scale per step, the permanent first-conv switch on
    the first scale-0 step), as tests/norel_ref.py::make_eps_fn."""
    state = dict(sd_conv=False)
    g = {k: inp[k] for k in KEYS}
    gn = null_grounding(g)

    def eps_fn(x, t, i, alpha):
        if alpha == 0:
            state["sd_conv"] = True
        fc = first_conv_sd if state["sd_conv"] else None
        e_c = unet_forward(sd, cfg, x, t, inp["context"], g, fuser_scale=alpha, first_conv=fc)
        e_u = unet_forward(sd, cfg, x, t, inp["uc"], gn, fuser_scale=alpha, first_conv=fc)
        return e_u + guidance * (e_c - e_u)
    return eps_fn
