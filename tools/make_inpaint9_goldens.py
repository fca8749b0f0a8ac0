#!/usr/bin/env python3
"""Generate the inpaint_mode goldens (tests/golden/ip9_*.npz) by running the REFERENCE itself (build container only), like
tools/make_ti_goldens.py: the reference path, ``fill`` and the ast-extracted interface functions come from tools/make_goldens.py by
import, the reference's mask function and the replayed randn_like from tools/make_inpaint_goldens.py.

    python tools/make_inpaint9_goldens.py [name ...]        # writes only the cases of tests/inpaint9_cases.py

The reference's UNetModel is built with ``inpaint_mode=True`` (a 9-channel first conv, openaimodel.py:293-299) for the text and the
text_image PositionNet; recipe weights by name, recipe inputs, OUTPUTS only.  Re-running rewrites the same bytes.
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

import inpaint9_cases as ic  # noqa: E402

from grounding_input.text_image_grounding_tokinzer_input import GroundingNetInput as TIGroundingNetInput  # noqa: E402

T = torch.from_numpy
TARGETS = {"text": "ldm.modules.diffusionmodules.text_grounding_net.PositionNet",
           "text_image": "ldm.modules.diffusionmodules.text_image_grounding_net.PositionNet"}


def tiny_unet(cfg):
    m = mg.UNetModel(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                     out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks,
                     attention_resolutions=list(cfg.attention_resolutions), channel_mult=list(cfg.channel_mult),
                     num_heads=cfg.num_heads, context_dim=cfg.context_dim, fuser_type="gatedSA", inpaint_mode=True,
                     grounding_tokenizer=dict(target=TARGETS[cfg.grounding], params=dict(in_dim=cfg.pos_in_dim, out_dim=cfg.pos_out_dim)))
    assert tuple(m.input_blocks[0][0].weight.shape) == (cfg.model_channels, cfg.first_conv_in, 3, 3) and not m.first_conv_restorable
    mg.fill(m, "", 0)
    m.grounding_tokenizer_input = TIGroundingNetInput() if cfg.grounding == "text_image" else mg.GroundingNetInput()
    return m


def grounding_of(m, cfg, inp):
    if cfg.grounding == "text_image":
        return m.grounding_tokenizer_input.prepare({a: inp[a] for a in ic.TI_KEYS})
    return m.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)


@torch.no_grad()
def run_case(case):
    k = case["kind"]
    raw = ic.case_inputs(case)
    inp = {a: T(v) for a, v in raw.items() if isinstance(v, np.ndarray)}
    if k == "extra":
        # gligen_inference.py:400-407 with the recipe z0 in the place of autoencoder.encode(input_image)
        mask = mig.ref_draw_masks_from_boxes()(inp["boxes"], case["hw"])
        return dict(out=torch.cat([inp["z0"] * mask, mask], dim=1).numpy())
    cfg = ic.cfg_of(case)
    m = tiny_unet(cfg)
    set_alpha_scale, alpha_generator = mg.ref_interface_fns()
    if k == "unet":
        set_alpha_scale(m, case["scale"])
        if case["restore"]:
            m.restore_first_conv_from_SD()              # the reference's own method: prints and keeps the conv
            assert tuple(m.input_blocks[0][0].weight.shape)[1] == cfg.first_conv_in
        d = dict(x=inp["x"], timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
                 inpainting_extra_input=inp["extra"], grounding_extra_input=None)
        if case["grounding"] == "real":
            d["grounding_input"] = grounding_of(m, cfg, inp)
        else:
            grounding_of(m, cfg, inp)                   # sets the shapes get_null_input() reads
            d["context"] = inp["uc"]
        return dict(out=m(d).numpy())
    if k == "plms":
        diff = mg.LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
        sampler = mg.PLMSSampler(diff, m, alpha_generator_func=partial(alpha_generator, type=case["alpha_type"]), set_alpha_scale=set_alpha_scale)
        d = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], relations=inp["relations"], grounding_input=grounding_of(m, cfg, inp),
                 inpainting_extra_input=inp["extra"], grounding_extra_input=None)
        noises = raw["noises"]
        count = [0]

        def randn_like(t, *a, **kw):
            arr = noises[count[0]]
            assert tuple(arr.shape) == tuple(t.shape), (count[0], arr.shape, t.shape)
            count[0] += 1
            return T(arr).to(t.device, t.dtype)
        real = torch.randn_like
        torch.randn_like = randn_like
        try:
            out = sampler.sample(S=case["S"], shape=(case["B"], 4, case["hw"], case["hw"]), input=d, uc=inp["uc"],
                                 guidance_scale=case["guidance"], mask=inp["mask"], x0=inp["x0"])
        finally:
            torch.randn_like = real
        assert count[0] == len(noises)
        return dict(out=out.numpy())
    raise ValueError(k)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    for case in ic.CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = os.path.join(outdir, case["name"] + ".npz")
        np.savez_compressed(path, **res)
        print(f"{case['name']:26s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {res['out'].shape}")


if __name__ == "__main__":
    main()
