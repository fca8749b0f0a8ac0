#!/usr/bin/env python3
"""Generate the DDIM goldens (tests/golden/ddim_*.npz) by running the REFERENCE's own DDIMSampler (build container only), like
tools/make_norel_goldens.py: the reference path, ``fill`` and the ast-extracted interface functions come from tools/make_goldens.py, the
upstream (pre-modification) UNet from tools/make_norel_goldens.py, by import.

    python tools/make_ddim_goldens.py [name ...]        # ddim_schedule and the cases of tests/ddim_cases.py

Recipe weights, recipe inputs, OUTPUTS only -- plus every tensor the run's ``torch.randn_like`` returned, in call order (recipe noise, so that
re-running rewrites the same bytes).  eta and "quad" go through ``make_schedule`` + ``ddim_sampling``: the reference's ``sample()`` re-makes
the schedule with eta 0.  The relation UNet runs with guidance 1 only (with guidance the reference's unconditional input lacks
``"relations"``, ddim.py:116).
"""
from __future__ import annotations

import os
import sys
from functools import partial

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (puts the reference, the repo and tests/ on sys.path)
import make_norel_goldens as mng  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ddim_cases as dc  # noqa: E402
import norel_cases as nc  # noqa: E402

from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402

T = torch.from_numpy


def diffusion():
    return mg.LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)


def schedule():
    """the tables of make_schedule in the reference's dtypes, and per index the five float32 scalars as p_sample_ddim forms them"""
    out = {}
    for S, disc, eta in dc.SCHEDULE_CASES:
        s = DDIMSampler(diffusion(), model=None)
        s.make_schedule(S, ddim_discretize=disc, ddim_eta=eta)
        tag = dc.schedule_tag(S, disc, eta)
        for k in dc.SCHEDULE_KEYS:
            v = getattr(s, k)
            out[f"{tag}.{k}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
        coefs = []
        for index in range(len(s.ddim_timesteps)):
            full = lambda v: torch.full((1, 1, 1, 1), v)
            a_t, a_prev, sigma_t, s1m = (full(getattr(s, k)[index]) for k in ("ddim_alphas", "ddim_alphas_prev", "ddim_sigmas",
                                                                               "ddim_sqrt_one_minus_alphas"))
            assert all(v.dtype == torch.float32 for v in (a_t, a_prev, sigma_t, s1m))
            # the three float32 square roots are recorded correctly rounded (float64 sqrt of the float32 operand, rounded once more: exact for
            # sqrt), which is what the reference gets on its GPU; torch's vectorised CPU sqrt is 1 ulp off on some hosts (oracle/plms_ref.py)
            ieee_sqrt = lambda v: v.double().sqrt().float()
            row = []
            for v, root in ((a_t, True), (s1m, False), (a_prev, True), (1. - a_prev - sigma_t**2, True), (sigma_t, False)):
                assert v.dtype == torch.float32
                if root:
                    assert abs(float(v.sqrt()) - float(ieee_sqrt(v))) <= float(np.spacing(np.float32(float(ieee_sqrt(v)))))
                row.append(float(ieee_sqrt(v) if root else v))
            coefs.append(row)
        out[f"{tag}.coefs"] = np.asarray(coefs, np.float32)
    return out


@torch.no_grad()
def run_case(case):
    inp = {a: T(v) for a, v in dc.case_inputs(case).items()}
    if case["unet"] == "norel":
        m = mng.tiny_unet(nc.NR_TINY)
        set_alpha_scale, alpha_generator = mng.upstream_interface_fns()
        relations = torch.zeros(1)          # never read by the upstream model
    else:
        m = mg.tiny_unet()
        set_alpha_scale, alpha_generator = mg.ref_interface_fns()
        relations = inp["relations"]
    sampler = DDIMSampler(diffusion(), m, alpha_generator_func=partial(alpha_generator, type=case["alpha_type"]), set_alpha_scale=set_alpha_scale)
    g = m.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
    d = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], relations=relations, grounding_input=g,
             inpainting_extra_input=None, grounding_extra_input=None)
    sampler.make_schedule(case["S"], ddim_discretize=case["discretize"], ddim_eta=case["eta"])
    fake, rec = dc.recorder(f"{case['name']}.noise")
    with dc.patched_randn_like(fake):
        out = sampler.ddim_sampling((case["B"], 4, case["h"], case["w"]), d, inp["uc"], case["guidance"],
                                    mask=inp.get("mask"), x0=inp.get("x0"))
    res = dict(out=out.numpy(), ddim_timesteps=np.asarray(sampler.ddim_timesteps))
    res.update(dc.pack_draws(rec))
    return res


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    jobs = [("ddim_schedule", schedule)] + [(c["name"], partial(run_case, c)) for c in dc.CASES]
    for name, fn in jobs:
        if only and name not in only:
            continue
        res = fn()
        path = os.path.join(outdir, name + ".npz")
        np.savez_compressed(path, **res)
        print(f"{name:20s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {len(res)} arrays")


if __name__ == "__main__":
    main()
