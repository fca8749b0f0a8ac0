#!/usr/bin/env python3
"""Generate the rectangular goldens (tests/golden/*_rect*.npz) by running the REFERENCE itself (build container only), like
tools/make_inpaint_goldens.py: the reference path, tiny_unet(), the ast-extracted interface functions come from
tools/make_goldens.py by import, the replayed randn_like and the autoencoder from tools/make_inpaint_goldens.py.

    python tools/make_rect_goldens.py [name ...]        # writes only the cases of tests/rect_cases.py

The reference computes rectangular outputs already (SpatialTransformer takes h, w from x.shape, RelationCrossAttention scales box
x by w and box y by h, the sampler uses input["x"] as given): every module is called exactly as tools/make_goldens.py calls it,
on an h != w input.  Re-running this tool rewrites the same bytes (recipe tensors in, np.savez_compressed out).
"""
from __future__ import annotations

import os
import sys
from functools import partial

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (puts the reference, the repo and tests/ on sys.path)
import make_inpaint_goldens as mig  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from layoutllm_t2i_amd import recipe  # noqa: E402
from layoutllm_t2i_amd.arch import VAE_TINY  # noqa: E402
import rect_cases as rc  # noqa: E402

T = torch.from_numpy
A = mg.A
SEED = 1234


def sampler_and_input(case, inp):
    m = mg.tiny_unet()
    set_alpha_scale, alpha_generator = mg.ref_interface_fns()
    diff = mg.LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    sampler = mg.PLMSSampler(diff, m, alpha_generator_func=partial(alpha_generator, type=case["alpha_type"]), set_alpha_scale=set_alpha_scale)
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
    g = m.grounding_tokenizer_input.prepare(batch, None)
    d = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], relations=inp["relations"], grounding_input=g,
             inpainting_extra_input=None, grounding_extra_input=None)
    return sampler, d


@torch.no_grad()
def run_case(case):
    k, nm = case["kind"], case["name"]
    h, w = case["h"], case["w"]
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    tag = f"golden.{nm}"
    if k == "rela":
        C, H = case["C"], case["heads"]
        m = mg.fill(A.RelationCrossAttention(C, rc.CTX, rc.CTX, H, C // H), tag)
        return dict(out=m(inp["x"], inp["relations"], inp["boxes"], inp["masks"], h, w).numpy())
    if k == "spatial_transformer":
        C, H = case["C"], case["heads"]
        m = mg.fill(A.SpatialTransformer(C, rc.CTX, rc.CTX, H, C // H, depth=1, fuser_type="gatedSA"), tag)
        for mod in m.modules():
            if type(mod) == A.GatedSelfAttentionDense:
                mod.scale = case["scale"]
        return dict(out=m(inp["x"], inp["context"], inp["objs"], inp["relations"], inp["boxes"], inp["masks"]).numpy())
    if k == "down":
        m = mg.fill(mg.Downsample(case["C"], True, dims=2, out_channels=case["C"]), tag)
        return dict(out=m(inp["x"]).numpy())
    if k == "up":
        m = mg.fill(mg.Upsample(case["C"], True, dims=2, out_channels=case["C"]), tag)
        return dict(out=m(inp["x"]).numpy())
    if k == "unet":
        m = mg.tiny_unet()
        set_alpha_scale, _ = mg.ref_interface_fns()
        set_alpha_scale(m, case["scale"])
        if case["sdconv"]:
            m.restore_first_conv_from_SD()
        batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
        g = m.grounding_tokenizer_input.prepare(batch, None)
        d = dict(x=inp["x"], timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
                 inpainting_extra_input=None, grounding_extra_input=None, grounding_input=g)
        return dict(out=m(d).numpy())
    if k == "vae":
        m = mig.autoencoder(VAE_TINY)
        sd = {n: T(np.asarray(v)) for n, v in recipe.vae_state_dict(VAE_TINY, 0).items()}
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(x.startswith(("encoder.", "quant_conv.")) for x in missing), (missing[:3], unexpected)
        return dict(out=m.decode(inp["z"]).numpy())
    if k == "vae_enc":
        m = mig.autoencoder(VAE_TINY)
        sd = {n: T(np.asarray(v)) for n, v in {**recipe.vae_state_dict(VAE_TINY, 0), **recipe.vae_encoder_state_dict(VAE_TINY, 0)}.items()}
        m.load_state_dict(sd, strict=True)
        x = inp["x"]
        mean = torch.chunk(m.quant_conv(m.encoder(x)), 2, dim=1)[0]
        torch.manual_seed(SEED)
        z = m.encode(x)
        torch.manual_seed(SEED)
        noise = torch.randn(mean.shape)
        return dict(x=x.numpy(), noise=noise.numpy(), mean=mean.numpy(), z=z.numpy(), seed=np.int64(SEED))
    if k == "plms":
        sampler, d = sampler_and_input(case, inp)
        out = sampler.sample(S=case["S"], shape=(case["B"], 4, h, w), input=d, uc=inp["uc"], guidance_scale=case["guidance"])
        return dict(out=out.numpy())
    if k == "plms_inpaint":
        sampler, d = sampler_and_input(case, inp)
        # the per-axis rectangle mask in plain numpy (the reference's mask function is square only; its sampler takes any mask that
        # broadcasts against the latent)
        mask = rc.rect_mask_rule(inp["boxes"].numpy(), h, w)
        fake, rec = mig.replay_noise("inpaint.rect.noise")
        real = torch.randn_like
        torch.randn_like = fake
        try:
            out = sampler.sample(S=case["S"], shape=(case["B"], 4, h, w), input=d, uc=inp["uc"], guidance_scale=case["guidance"], mask=T(mask),
                                 x0=inp["x0"])
        finally:
            torch.randn_like = real
        res = dict(out=out.numpy(), x0=inp["x0"].numpy(), mask=mask, draw_shapes=np.array([list(a.shape) for a in rec], np.int64))
        res.update({f"noise_{i:03d}": a for i, a in enumerate(rec)})
        return res
    raise ValueError(k)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    total = 0
    for case in rc.CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = os.path.join(outdir, case["name"] + ".npz")
        np.savez_compressed(path, **res)
        total += len(res)
        print(f"{case['name']:24s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {len(res)} arrays")
    print(f"{total} arrays")


if __name__ == "__main__":
    main()
