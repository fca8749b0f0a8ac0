#!/usr/bin/env python3
"""What a DPM-Solver++(2M) step costs next to a DDIM and a PLMS step, and what 20 of them buy (GPU box): one handle of the full
configuration, 2B = 8 ([cond ; uncond] of 4 latents), 64 x 64.

    python tools/dpmpp_probe.py [--out DIR] [--rounds R] [--iters K] [--image-rounds N]

tail  : the work behind the UNet forward, on buffers of the step's size.  DPM-Solver++: ONE launch (gl_dpmpp_update: CFG combine + x0 +
        the multistep difference + x_prev; first and second order).  DDIM: ONE launch (gl_ddim_update, eta 0).  PLMS: TWO launches
        (gl_cfg_combine, then gl_plms_update with the full 4-term history).  Device events around K back-to-back repetitions, the variants
        alternating within every round, median over the rounds and the spread.  Launch-bound kernels: mostly the cost of a launch.
step  : a whole gl_dpmpp_step against a whole gl_ddim_step and gl_plms_step on the same handle (graph replay, fuser on), the same way.
images: interface.denoise + the VAE decode, B = 4 images per call: sampler "dpmpp_2m" at steps = 20 (20 evaluations) next to PLMS at
        steps = 50 (51 evaluations), alternating, device events around each call, medians.
        -> DIR/dpmpp_step.txt

Weights are weights.random_state_dict / random_vae_state_dict (magnitudes of the recipe, generated on the device): only shapes matter here,
and nothing can be said about image quality.  No threshold is attached to any figure.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from layoutllm_t2i_amd import host, ops, recipe
from layoutllm_t2i_amd.arch import UNetConfig, VAEConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.interface import denoise
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.vae import VAEDecoder
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict, random_vae_state_dict

DEV = "cuda:0"
T = torch.from_numpy


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(variants, rounds, iters, warm=3):
    """{name: callable} -> {name: [ms per call, one per round]}, the variants alternating within every round"""
    for fn in variants.values():
        timed(fn, warm)                   # warm-up: code objects, graph capture
    res = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            res[n].append(timed(fn, iters))
    return res


def line(name, ms, unit="us", k=1e3):
    return f"{name:44s} median {statistics.median(ms) * k:9.2f} {unit}   min {min(ms) * k:9.2f}   max {max(ms) * k:9.2f}"


def facade(packed, cfg):
    """the model facade around already-packed weights (UNetModel.__init__ packs from a state_dict)"""
    m = UNetModel.__new__(UNetModel)
    m.cfg, m.device = packed.cfg, DEV
    m.image_size, m.in_channels, m.out_channels, m.model_channels = cfg.image_size, cfg.in_channels, cfg.out_channels, cfg.model_channels
    m.first_conv_restorable, m.first_conv_type = True, "GLIGEN"
    m.grounding_tokenizer_input = GroundingNetInput()
    m.fuser_scale, m.training, m._cond_key = 1.0, False, None
    m.engine = UNetEngine(packed)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--image-rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dpmpp_probe.py measures on the GPU: none found")
    B, hw = 4, 64
    cfg = UNetConfig()
    gfc = torch.Generator(device=DEV)
    gfc.manual_seed(2)
    fc = {"weight": torch.randn(cfg.model_channels, cfg.in_channels, 3, 3, device=DEV, generator=gfc) * 0.16,
          "bias": torch.zeros(cfg.model_channels, device=DEV)}
    model = facade(pack_state_dict(random_state_dict(cfg, DEV, 0), cfg, DEV, fc), cfg)
    eng = model.engine
    inp = {k: T(v).to(DEV) for k, v in recipe.synth_inputs(cfg, B, hw, n_boxes=8, n_rel=3, seed=4321).items()}
    z, cat = torch.zeros_like, lambda a, b: torch.cat([a, b], 0)
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), hw)
    x0 = inp["x"].contiguous()
    x, hist, e_out = x0.clone(), torch.randn_like(x0), torch.empty_like(x0)
    eps2b = torch.randn(2 * B, 4, hw, hw, device=DEV)
    old = [torch.randn_like(x0) for _ in range(3)]
    sched = host.make_dpm_schedule(20, host.alphas_cumprod())
    names = ("sqrt_at", "s1m", "c_x", "c_d", "w1", "w0")
    k2, k1 = dict(zip(names, host.dpm_step_coefs(sched, 10, 11, 2))), dict(zip(names, host.dpm_step_coefs(sched, 19, None, 2)))
    sq_at, s1m, sq_ap, dirc, _ = host.ddim_step_coefs(host.make_ddim_schedule(50, host.alphas_cumprod(), "uniform", 0.0), 30)
    dkw = dict(sqrt_at=sq_at, s1m=s1m, sqrt_aprev=sq_ap, dir_coef=dirc)
    coefs, div = host.PLMS_COEFS[3]
    out, p_out = torch.empty_like(x0), torch.empty_like(x0)      # out of place: the operands stay put over the repetitions

    def plms_tail():
        ops.cfg_combine(eps2b, 7.5, e_out)
        ops.plms_update(x, e_out, old, coefs, div, sq_at, s1m, sq_ap, dirc, out)
    tail = measure({"dpmpp tail, 2nd order (1 launch, + history)": lambda: ops.dpmpp_update(eps2b, x, out, p_out, x0_old=hist, guidance=7.5, **k2),
                    "dpmpp tail, 1st order (1 launch)": lambda: ops.dpmpp_update(eps2b, x, out, p_out, guidance=7.5, **k1),
                    "ddim tail, eta 0 (1 launch)": lambda: ops.ddim_update(eps2b, x, out, guidance=7.5, **dkw),
                    "plms tail (2 launches, 4 eps terms)": plms_tail}, args.rounds, 10 * args.iters)
    skw = dict(t=601.0, reps=2, guidance=7.5, fuser_scale=1.0, sd_conv=False)
    step = measure({"dpmpp step, 2nd order": lambda: eng.dpmpp_step(x, out, p_out, x0_old=hist, **skw, **k2),
                    "ddim step, eta 0": lambda: eng.ddim_step(x, out, **skw, **dkw),
                    "plms step (4 eps terms)": lambda: eng.plms_step(x, x, out, e_out, [e_out] + old, coefs, div, 601.0, 2, 7.5, 1.0, False, sq_at,
                                                                     s1m, sq_ap, dirc)}, args.rounds, args.iters)
    launches = eng.num_launches()

    # ---- whole images: denoise + VAE decode
    vae = VAEDecoder(random_vae_state_dict(VAEConfig(), DEV, seed=1), VAEConfig(), DEV)
    am = (model, vae, None, LatentDiffusion(device=DEV), {})
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])

    def images(**kw):
        model.first_conv_type = "GLIGEN"
        return vae.decode(denoise(am, inp["context"], inp["uc"], inp["relations"], batch, inp["x"], [0.3, 0.0, 0.7], 7.5, **kw))
    img = measure({"dpmpp_2m, steps = 20 (20 evaluations)": lambda: images(steps=20, sampler="dpmpp_2m"),
                   "plms, steps = 50 (51 evaluations)": lambda: images(steps=50)}, args.image_rounds, 1, warm=1)

    lines = [f"# tools/dpmpp_probe.py: full configuration, 2B = {2 * B}, {hw} x {hw} latents ({x0.numel()} elements), {torch.cuda.get_device_name(0)}",
             f"# device events around back-to-back calls, variants alternating per round, {args.rounds} rounds; per-call figures",
             f"# tail: {10 * args.iters} calls per round (launch-bound kernels: mostly the cost of a launch)"]
    lines += [line(n, ms) for n, ms in tail.items()]
    lines += [f"# step: {args.iters} calls per round, graph replay, fuser on, {launches} kernel launches per forward"]
    lines += [line(n, ms, "ms", 1.0) for n, ms in step.items()]
    d, p = (statistics.median(step[k]) for k in ("dpmpp step, 2nd order", "plms step (4 eps terms)"))
    lines.append(f"# dpmpp step / plms step = {d / p:.4f} (medians); the spread of either is the max - min above")
    lines.append(f"# images: interface.denoise + VAE decode of B = {B} images (512 x 512) per call, default mode, {args.image_rounds} rounds of one call each")
    lines += [line(n, ms, "ms", 1.0) + f"   {B / (statistics.median(ms) * 1e-3):6.2f} images/s" for n, ms in img.items()]
    a, b = (statistics.median(img[k]) for k in img)
    lines.append(f"# images/s, dpmpp_2m at 20 over plms at 50 = {b / a:.2f} (medians).  Random weights: a cost figure only; that 20 steps of this "
                 "solver match 50 of PLMS in quality rests on the literature, not on this run")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "dpmpp_step.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(f"-> {path}")


if __name__ == "__main__":
    main()
