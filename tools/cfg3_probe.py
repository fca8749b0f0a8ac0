#!/usr/bin/env python3
"""What the text-only third branch of three-branch guidance costs (GPU box): handles of the full configuration, with and without the
relation chain, B = 4 latents, 64 x 64.

    python tools/cfg3_probe.py [--out DIR] [--rounds R] [--iters K] [--image-rounds N]

forward: gl_unet_forward with reps = 3 on [cond ; text-only ; uncond] (3B = 12) next to reps = 2 on [cond ; uncond] (2B = 8), fuser on and
         off, graph replay.  Device events around K back-to-back calls, the variants alternating within every round, medians and the spread.
         (reps = 2 has the shared cond / uncond prefix, option 44; reps = 3 does not.)
images : interface.denoise, 50 PLMS steps (51 evaluations) of B = 4 latents at alpha_type [0.3, 0, 0.7], with layout_guidance_scale = 12 and
         without the key, on both handles, alternating, device events around each call, medians.  The no-relation handle runs three branches on
         the 16 fuser-on evaluations only (the two-branch rule, sampler._Sampler._needs_text_branch); "no rule" is the same run with the rule
         switched off, which is what the rule saves.
tiny   : the end-to-end rel-L2 between layout_guidance_scale == guidance_scale and the plain two-branch run on the TINY models (informational).
         -> DIR/cfg3_step.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes matter here, and nothing can be said
about image quality.  No threshold is attached to any figure.
"""
import argparse
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import TINY, UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.interface import denoise
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.sampler import _Sampler
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


def measure(variants, rounds, iters, warm=3):
    """{name: callable} -> {name: [ms per call, one per round]}, the variants alternating within every round"""
    for fn in variants.values():
        timed(fn, warm)                   # warm-up: code objects, graph capture
    res = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            res[n].append(timed(fn, iters))
    return res


def line(name, ms):
    return f"{name:52s} median {statistics.median(ms):9.2f} ms   min {min(ms):9.2f}   max {max(ms):9.2f}"


def facade(packed, cfg):
    """the model facade around already-packed weights (UNetModel.__init__ packs from a state_dict)"""
    m = UNetModel.__new__(UNetModel)
    m.cfg, m.device = packed.cfg, torch.device(DEV)
    m.image_size, m.in_channels, m.out_channels, m.model_channels = cfg.image_size, cfg.in_channels, cfg.out_channels, cfg.model_channels
    m.first_conv_restorable, m.first_conv_type = True, "GLIGEN"
    m.grounding_tokenizer_input = GroundingNetInput()
    m.fuser_scale, m.training, m._cond_key = 1.0, False, None
    m.engine = UNetEngine(packed)
    return m


def full_model(cfg):
    gfc = torch.Generator(device=DEV)
    gfc.manual_seed(2)
    fc = {"weight": torch.randn(cfg.model_channels, cfg.in_channels, 3, 3, device=DEV, generator=gfc) * 0.16,
          "bias": torch.zeros(cfg.model_channels, device=DEV)}
    return facade(pack_state_dict(random_state_dict(cfg, DEV, 0), cfg, DEV, fc), cfg)


def set_cond(model, inp, hw, three):
    z = torch.zeros_like
    n = 3 if three else 2
    ctx = torch.cat([inp["context"]] * (n - 1) + [inp["uc"]], 0)
    rel = torch.cat([inp["relations"]] * n, 0) if model.cfg.relation else None
    g = [torch.cat([t] + [z(t)] * (n - 1), 0) for t in (inp["boxes"], inp["masks"], inp["positive_embeddings"])]
    model.engine.set_conditioning(ctx, rel, *g, hw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--image-rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cfg3_probe.py measures on the GPU: none found")
    B, hw = 4, 64
    lines = [f"# tools/cfg3_probe.py: full configuration, B = {B}, {hw} x {hw} latents, {torch.cuda.get_device_name(0)}",
             f"# device events around back-to-back calls, variants alternating per round; per-call figures",
             f"# forward: {args.iters} calls per round, {args.rounds} rounds, graph replay; reps = 3 on 3B = {3 * B}, reps = 2 on 2B = {2 * B}"]
    fwd_ratio, img_stats = {}, {}
    for tag, cfg in (("relation", UNetConfig()), ("no relation", dataclasses.replace(UNetConfig(), relation=False))):
        model = full_model(cfg)
        eng = model.engine
        inp = {k: T(v).to(DEV) for k, v in recipe.synth_inputs(cfg, B, hw, n_boxes=8, n_rel=3, seed=4321).items()}
        x = inp["x"].contiguous()
        # ---- one forward.  The conditioning form is fixed per measurement: a variant is (form, fuser)
        res = {}
        for three in (False, True):
            set_cond(model, inp, hw, three)
            reps = 3 if three else 2
            part = measure({f"{tag}: forward reps = {reps}, fuser on": lambda: eng.forward(x, 601.0, 1.0, False, reps),
                            f"{tag}: forward reps = {reps}, fuser off (SD conv)": lambda: eng.forward(x, 601.0, 0.0, True, reps)},
                           args.rounds, args.iters)
            res.update(part)
        lines += [line(n, ms) for n, ms in res.items()]
        for f in ("fuser on", "fuser off (SD conv)"):
            r = statistics.median(res[f"{tag}: forward reps = 3, {f}"]) / statistics.median(res[f"{tag}: forward reps = 2, {f}"])
            fwd_ratio[(tag, f)] = r
            lines.append(f"# {tag}: reps = 3 / reps = 2, {f} = {r:.3f} (medians; 1.5 = cost per sample unchanged)")

        # ---- a 50-step PLMS image
        am = (model, None, None, LatentDiffusion(device=DEV), {})
        batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])

        def image(**kw):
            model.first_conv_type = "GLIGEN"
            return denoise(am, inp["context"], inp["uc"], inp["relations"] if cfg.relation else None, batch, inp["x"], [0.3, 0.0, 0.7], 7.5,
                           steps=50, **kw)
        rule = _Sampler._needs_text_branch

        def image_no_rule():
            _Sampler._needs_text_branch = lambda self, fuser_scale: True
            try:
                return image(layout_guidance_scale=12.0)
            finally:
                _Sampler._needs_text_branch = rule
        variants = {f"{tag}: plms 50, key absent": image, f"{tag}: plms 50, layout_guidance_scale = 12": lambda: image(layout_guidance_scale=12.0)}
        if not cfg.relation:
            variants[f"{tag}: plms 50, layout_guidance_scale = 12, no rule"] = image_no_rule
        img = measure(variants, args.image_rounds, 1, warm=1)
        img_stats[tag] = {n: statistics.median(ms) for n, ms in img.items()}
        lines.append(f"# images ({tag} handle): interface.denoise, 50 PLMS steps (51 evaluations) of B = {B}, alpha_type [0.3, 0, 0.7], "
                     f"{args.image_rounds} rounds of one call each")
        lines += [line(n, ms) for n, ms in img.items()]
        med = list(img_stats[tag].values())
        lines.append(f"# {tag}: with the key / without = {med[1] / med[0]:.3f} (medians)")
        if not cfg.relation:
            lines.append(f"# {tag}: the two-branch rule saves {med[2] - med[1]:.1f} ms of {med[2]:.1f} ms per call ({100 * (1 - med[1] / med[2]):.1f} %); "
                         f"without the rule the key costs {med[2] / med[0]:.3f} x")
        del model, eng, am
        torch.cuda.empty_cache()

    # ---- TINY: equal scales against the plain run, end to end
    from functools import partial
    from layoutllm_t2i_amd import interface as itf
    from layoutllm_t2i_amd.sampler import PLMSSampler
    lines.append("# tiny: PLMS, S = 50, B = 2, 16 x 16, guidance 7.5: rel_l2(layout_guidance_scale = 7.5, key absent) -- the two runs differ in the batch "
                 "form of every three-branch step and in the rounding of the combine")
    for tag, cfg in (("relation", TINY), ("no relation", dataclasses.replace(TINY, relation=False))):
        m = UNetModel(cfg, recipe.state_dict(cfg, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(cfg, 0))
        m.grounding_tokenizer_input = GroundingNetInput()
        inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, 2, 16, n_boxes=4, n_rel=3, seed=99).items()}
        outs = []
        for layout in (None, 7.5):
            m.first_conv_type = "GLIGEN"
            s = PLMSSampler(LatentDiffusion(device=DEV), m, alpha_generator_func=partial(itf.alpha_generator, type=[0.3, 0.0, 0.7]),
                            set_alpha_scale=itf.set_alpha_scale)
            g = m.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
            d = dict(x=inp["x"].to(DEV), timesteps=None, context=inp["context"], relations=inp["relations"], grounding_input=g)
            outs.append(s.sample_layout(S=50, shape=tuple(inp["x"].shape), input=d, uc=inp["uc"], guidance_scale=7.5,
                                        layout_guidance_scale=layout).double().cpu())
        lines.append(f"tiny, {tag:12s} rel_l2 = {float((outs[1] - outs[0]).norm() / outs[0].norm()):.3e}")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "cfg3_step.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(f"-> {path}")


if __name__ == "__main__":
    main()
