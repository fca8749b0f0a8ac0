#!/usr/bin/env python3
"""What a DDIM step costs next to a PLMS step (GPU box): one handle of the full configuration, 2B = 8 ([cond ; uncond] of 4 latents), 64 x 64.

    python tools/ddim_probe.py [--out DIR] [--rounds R] [--iters K]

tail : the work behind the UNet forward, on buffers of the step's size.  DDIM: ONE launch (gl_ddim_update: CFG combine + pred_x0 + x_prev,
       with and without the noise term).  PLMS: TWO launches (gl_cfg_combine, then gl_plms_update with the full 4-term history).  Device
       events around K back-to-back repetitions, the variants alternating within every round, median over the rounds and the spread.  The
       latent has 65536 elements: these are launch-bound kernels, the figure is mostly the cost of a launch.
step : a whole gl_ddim_step against a whole gl_plms_step on the same handle (graph replay, fuser on), measured the same way.
       -> DIR/ddim_step.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes matter here.  No threshold is attached:
the UNet dominates a step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from layoutllm_t2i_amd import host, ops, recipe
from layoutllm_t2i_amd.arch import UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

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


def measure(variants, rounds, iters):
    """{name: callable} -> {name: [ms per call, one per round]}, the variants alternating within every round"""
    for fn in variants.values():
        timed(fn, 3)                      # warm-up: code objects, graph capture
    res = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            res[n].append(timed(fn, iters))
    return res


def line(name, ms, unit="us", k=1e3):
    return f"{name:44s} median {statistics.median(ms) * k:9.2f} {unit}   min {min(ms) * k:9.2f}   max {max(ms) * k:9.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ddim_probe.py measures on the GPU: none found")
    B, hw = 4, 64
    cfg = UNetConfig()
    eng = UNetEngine(pack_state_dict(random_state_dict(cfg, DEV, 0), cfg, DEV))
    inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, B, hw, n_boxes=8, n_rel=3, seed=4321).items()}
    z, cat = torch.zeros_like, lambda a, b: torch.cat([a, b], 0).to(DEV)
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), hw)
    x0 = inp["x"].to(DEV).contiguous()
    x, noise, e_out = x0.clone(), torch.randn_like(x0), torch.empty_like(x0)
    eps2b = torch.randn(2 * B, 4, hw, hw, device=DEV)
    old = [torch.randn_like(x0) for _ in range(3)]
    sq_at, s1m, sq_ap, dirc, sigma = host.ddim_step_coefs(host.make_ddim_schedule(50, host.alphas_cumprod(), "uniform", 1.0), 30)
    kw = dict(sqrt_at=sq_at, s1m=s1m, sqrt_aprev=sq_ap, dir_coef=dirc)
    coefs, div = host.PLMS_COEFS[3]
    out = torch.empty_like(x0)            # out of place: the operands stay put over the repetitions

    def plms_tail():
        ops.cfg_combine(eps2b, 7.5, e_out)
        ops.plms_update(x, e_out, old, coefs, div, sq_at, s1m, sq_ap, dirc, out)
    tail = measure({"ddim tail, eta 0 (1 launch)": lambda: ops.ddim_update(eps2b, x, out, guidance=7.5, **kw),
                    "ddim tail, eta 1 (1 launch, + noise)": lambda: ops.ddim_update(eps2b, x, out, guidance=7.5, sigma=sigma, noise=noise, **kw),
                    "plms tail (2 launches, 4 eps terms)": plms_tail}, args.rounds, 10 * args.iters)
    step_kw = dict(t=601.0, reps=2, guidance=7.5, fuser_scale=1.0, sd_conv=False)
    step = measure({"ddim step, eta 0": lambda: eng.ddim_step(x, out, **step_kw, **kw),
                    "ddim step, eta 1": lambda: eng.ddim_step(x, out, sigma=sigma, noise=noise, **step_kw, **kw),
                    "plms step (4 eps terms)": lambda: eng.plms_step(x, x, out, e_out, [e_out] + old, coefs, div, 601.0, 2, 7.5, 1.0, False, sq_at,
                                                                     s1m, sq_ap, dirc)}, args.rounds, args.iters)
    lines = [f"# tools/ddim_probe.py: full configuration, 2B = {2 * B}, {hw} x {hw} latents ({x0.numel()} elements), {torch.cuda.get_device_name(0)}",
             f"# device events around back-to-back calls, variants alternating per round, {args.rounds} rounds; per-call figures",
             f"# tail: {10 * args.iters} calls per round (launch-bound kernels: mostly the cost of a launch)"]
    lines += [line(n, ms) for n, ms in tail.items()]
    lines += [f"# step: {args.iters} calls per round, graph replay, fuser on, {eng.num_launches()} kernel launches per forward"]
    lines += [line(n, ms, "ms", 1.0) for n, ms in step.items()]
    d, p = (statistics.median(step[k]) for k in ("ddim step, eta 0", "plms step (4 eps terms)"))
    lines.append(f"# ddim step / plms step = {d / p:.4f} (medians); the spread of either is the max - min above")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ddim_step.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(f"-> {path}")


if __name__ == "__main__":
    main()
