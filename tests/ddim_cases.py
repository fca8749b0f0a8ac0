"""Case table of the DDIM goldens (tests/golden/ddim_*.npz), shared by tools/make_ddim_goldens.py (reference side, build container only),
tests/test_ddim_host.py and tests/test_gpu_ddim.py, plus the recorder / replayer of the reference's ``torch.randn_like`` draws.

Like tests/golden_cases.py every case is data.  The inputs are those of ``plms_tiny`` (relation UNet) / ``norel_plms_tiny`` (upstream UNet);
the fixtures hold the reference's OUTPUTS, and every noise tensor its ``torch.randn_like`` was given, in call order (``noise_###`` with
``draw_shapes``, as the inpainting goldens store them): per step q_sample's draw on ``x0`` first when a mask is given, then the latent's.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from layoutllm_t2i_amd import recipe

import golden_cases as gc
import norel_cases as nc

# (S, discretize, eta): uniform S = 6 gives 7 timesteps (range(0, 1000, 166)); quad S = 50 repeats timesteps at its low end
SCHEDULE_CASES = [(10, "uniform", 0.0), (10, "uniform", 1.0), (6, "uniform", 1.0), (8, "quad", 0.5), (50, "quad", 0.3)]
SCHEDULE_KEYS = ("ddim_timesteps", "ddim_alphas", "ddim_alphas_prev", "ddim_sqrt_one_minus_alphas", "ddim_sigmas")


def schedule_tag(S, discretize, eta):
    return f"s{S}_{discretize}_eta{int(round(eta * 10)):02d}"


_COMMON = dict(B=2, h=16, w=16, alpha_type=[0.3, 0.0, 0.7], mask=False)
CASES = [
    dict(_COMMON, name="ddim_norel_eta0", unet="norel", S=10, discretize="uniform", eta=0.0, guidance=7.5),
    dict(_COMMON, name="ddim_norel_eta1", unet="norel", S=10, discretize="uniform", eta=1.0, guidance=7.5),
    dict(_COMMON, name="ddim_norel_quad", unet="norel", S=8, discretize="quad", eta=0.5, guidance=7.5),
    # 7 steps; x0 and mask of batch 1, a rectangle of zeros (regenerate) in a mask of ones (keep)
    dict(_COMMON, name="ddim_norel_mask", unet="norel", S=6, discretize="uniform", eta=1.0, guidance=7.5, mask=True),
    # the relation UNet: the reference's DDIM runs on it only without guidance (its unconditional input has no "relations", ddim.py:116)
    dict(_COMMON, name="ddim_rel_g1", unet="rel", S=10, discretize="uniform", eta=0.5, guidance=1.0),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def plms_case(case):
    """the PLMS golden case of the same model: its inputs are this case's inputs"""
    return nc.by_name("norel_plms_tiny") if case["unet"] == "norel" else next(c for c in gc.CASES if c["name"] == "plms_tiny")


def case_inputs(case):
    """Numpy inputs (weights excluded); a mask case adds ``x0`` [1, 4, h, w] and ``mask`` [1, 1, h, w]."""
    pc = plms_case(case)
    inp = dict((nc if case["unet"] == "norel" else gc).case_inputs(pc))
    if case["mask"]:
        inp.update(mask_inputs(case["h"], case["w"]))
    return inp


def mask_inputs(h, w):
    """x0 [1, 4, h, w] and a mask [1, 1, h, w] of ones with one rectangle of zeros that touches no border"""
    x0 = (recipe.normal("ddim.x0", (1, 4, h, w), 5) * np.float32(0.8)).astype(np.float32)
    mask = np.ones((1, 1, h, w), np.float32)
    mask[:, :, h // 4:h - h // 4, w // 8:w // 2 + 1] = 0
    return dict(x0=x0, mask=mask)


# ------------------------------------------------------------------------------------------- torch.randn_like, recorded and replayed
def recorder(tag):
    """(randn_like stand-in, list): every call returns deterministic recipe noise of the asked shape and appends it to the list"""
    rec = []

    def randn_like(t, *a, **k):
        arr = recipe.normal(f"{tag}.{len(rec)}", tuple(t.shape), 7)
        rec.append(arr)
        return torch.from_numpy(arr).to(t.device, t.dtype)
    return randn_like, rec


def pack_draws(rec):
    """the recorded draws as npz entries: ``draw_shapes`` [n, 4] and ``noise_000`` ..."""
    out = dict(draw_shapes=np.array([list(a.shape) for a in rec], np.int64).reshape(len(rec), -1))
    out.update({f"noise_{i:03d}": a for i, a in enumerate(rec)})
    return out


def unpack_draws(npz):
    return [np.asarray(npz[f"noise_{i:03d}"]) for i in range(len(npz["draw_shapes"]))]


def replayer(draws):
    """(randn_like stand-in, state): call k returns draws[k]; a call of another shape than the recorded one, or one call too many, fails --
    which is the test of the RNG order.  ``state["n"]`` counts the calls."""
    state = dict(n=0)

    def randn_like(t, *a, **k):
        i = state["n"]
        assert i < len(draws), f"draw {i}: the reference drew only {len(draws)} times"
        assert tuple(draws[i].shape) == tuple(t.shape), f"draw {i}: asked for {tuple(t.shape)}, the reference drew {tuple(draws[i].shape)}"
        state["n"] = i + 1
        return torch.from_numpy(np.ascontiguousarray(draws[i])).to(t.device, t.dtype)
    return randn_like, state


@contextlib.contextmanager
def patched_randn_like(fn):
    real = torch.randn_like
    torch.randn_like = fn
    try:
        yield
    finally:
        torch.randn_like = real
