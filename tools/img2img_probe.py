#!/usr/bin/env python3
"""What image-to-image sampling costs (GPU box): the full configuration with the relation chain, B = 4 latents, 64 x 64, random weights.

    python tools/img2img_probe.py [--out DIR] [--rounds R] [--image-rounds N]

q_sample: gl_q_sample alone at the sampler's latent shape (B = 4, 64 x 64, one image for the batch), a graph of 100 launches replayed.
images  : interface.denoise, PLMS with steps = 50 (50 nodes, 51 evaluations) of B = 4 latents at alpha_type [0.3, 0, 0.7]: without an image
          (the call as it was before the feature) next to strength 0.3 / 0.5 / 0.75 on the VAE-encoded image (one B = 1 512 x 512 encode inside
          the timed call, as interface._run issues it), alternating, device events around each call, medians.
          Expected: the time of the call without an image times (evaluations run) / 51, plus one encode; the table says what was measured.
          -> DIR/img2img_step.txt

Weights are weights.random_state_dict / recipe.vae_*_state_dict: only shapes matter here, and nothing can be said about what a strength does to
a real picture.  No threshold is attached to any figure.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cfg3_probe import full_model, line, measure
from layoutllm_t2i_amd import host, ops, recipe
from layoutllm_t2i_amd.arch import UNetConfig, VAEConfig
from layoutllm_t2i_amd.interface import denoise
from layoutllm_t2i_amd.model import LatentDiffusion
from layoutllm_t2i_amd.vae import VAEDecoder

DEV = "cuda:0"
T = torch.from_numpy
STRENGTHS = (0.3, 0.5, 0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--image-rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/img2img_probe.py measures on the GPU: none found")
    B, hw, S = 4, 64, 50
    lines = [f"# tools/img2img_probe.py: full configuration (relation chain), B = {B}, {hw} x {hw} latents, {torch.cuda.get_device_name(0)}",
             "# device events around the calls, variants alternating per round; per-call figures"]

    # ---- the kernel alone
    x0, noise, out = torch.randn(1, 4, hw, hw, device=DEV), torch.randn(B, 4, hw, hw, device=DEV), torch.empty(B, 4, hw, hw, device=DEV)
    ops.q_sample(x0, noise, 0.5, 0.5, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(100):
            ops.q_sample(x0, noise, 0.5, 0.5, out=out)
    q = measure({"gl_q_sample": g.replay}, args.rounds, 1)["gl_q_sample"]
    nbytes = 4 * (x0.numel() + 2 * noise.numel())
    lines.append(f"# q_sample: B = {B}, 4 x {hw} x {hw}, x0_batch = 1 (float4 path), a graph of 100 launches replayed, {args.rounds} rounds")
    lines.append(f"gl_q_sample{'':41s} median {statistics.median(q) * 10:9.2f} us per launch   min {min(q) * 10:9.2f}   max {max(q) * 10:9.2f}   "
                 f"({nbytes} bytes moved per launch)")

    # ---- a 50-step PLMS call, with and without an image
    cfg = UNetConfig()
    model = full_model(cfg)
    vcfg = VAEConfig()
    vae = VAEDecoder({**recipe.vae_state_dict(vcfg, 0), **recipe.vae_encoder_state_dict(vcfg, 0)}, vcfg, DEV)
    inp = {k: T(v).to(DEV) for k, v in recipe.synth_inputs(cfg, B, hw, n_boxes=8, n_rel=3, seed=4321).items()}
    img = T(np.clip(recipe.normal("probe.img", (1, 3, 8 * hw, 8 * hw), 1) * np.float32(0.5), -1, 1)).to(DEV)
    am = (model, vae, None, LatentDiffusion(device=DEV), {})
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])

    def image(strength=None):
        model.first_conv_type = "GLIGEN"
        kw = {} if strength is None else dict(init_latent=vae.encode(img), strength=strength)
        return denoise(am, inp["context"], inp["uc"], inp["relations"], batch, inp["x"], [0.3, 0.0, 0.7], 7.5, steps=S, **kw)
    n = len(host.make_schedule(S, host.alphas_cumprod())["ddim_timesteps"])
    evals = {None: n + 1, **{s: host.img2img_run_steps(n, s) + 1 for s in STRENGTHS}}       # PLMS evaluates its first step twice
    variants = {"plms 50, no image": image, **{f"plms 50, strength {s} ({evals[s]} evaluations) + encode": (lambda s=s: image(s)) for s in STRENGTHS},
                "vae.encode B = 1, 512 x 512 alone": lambda: vae.encode(img)}
    res = measure(variants, args.image_rounds, 1, warm=1)
    lines.append(f"# images: interface.denoise, PLMS steps = {S} ({n} nodes, {n + 1} evaluations) of B = {B}, alpha_type [0.3, 0, 0.7], guidance 7.5; "
                 f"{args.image_rounds} rounds of one call each")
    lines += [line(name, ms) for name, ms in res.items()]
    med = {name: statistics.median(ms) for name, ms in res.items()}
    full, enc = med["plms 50, no image"], med["vae.encode B = 1, 512 x 512 alone"]
    for s in STRENGTHS:
        got = med[f"plms 50, strength {s} ({evals[s]} evaluations) + encode"]
        want = full * evals[s] / evals[None] + enc
        lines.append(f"# strength {s}: measured {got:.1f} ms; (no image) x {evals[s]} / {evals[None]} + encode = {want:.1f} ms; measured / expected = "
                     f"{got / want:.3f}; measured / no image = {got / full:.3f}")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "img2img_step.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(f"-> {path}")


if __name__ == "__main__":
    main()
