#!/usr/bin/env python3
"""Generate the text_image goldens (tests/golden/ti_*.npz) by running the REFERENCE itself (build container only), like
tools/make_goldens.py, from which the reference path, ``fill`` and the ast-extracted interface functions come by import.

    python tools/make_ti_goldens.py [name ...]        # writes only the cases of tests/ti_cases.py

The reference's UNetModel is built with the text_image PositionNet (configs/GoldG+SBU+CC3M+O365_box_text_image.yaml) and its own
grounding-tokenizer input; recipe weights by name, recipe inputs, OUTPUTS only.  Re-running rewrites the same bytes.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (puts the reference, the repo and tests/ on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from layoutllm_t2i_amd import recipe  # noqa: E402
import ti_cases as tc  # noqa: E402

from ldm.modules.diffusionmodules.text_image_grounding_net import PositionNet  # noqa: E402
from grounding_input.text_image_grounding_tokinzer_input import GroundingNetInput  # noqa: E402

T = torch.from_numpy
KEYS = ("boxes", "masks", "text_masks", "image_masks", "text_embeddings", "image_embeddings")


def tiny_unet():
    cfg = tc.TI_TINY
    m = mg.UNetModel(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                     out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks,
                     attention_resolutions=list(cfg.attention_resolutions), channel_mult=list(cfg.channel_mult),
                     num_heads=cfg.num_heads, context_dim=cfg.context_dim, fuser_type="gatedSA",
                     grounding_tokenizer=dict(target="ldm.modules.diffusionmodules.text_image_grounding_net.PositionNet",
                                              params=dict(in_dim=cfg.pos_in_dim, out_dim=cfg.pos_out_dim)))
    mg.fill(m, "", 0)
    m.grounding_tokenizer_input = GroundingNetInput()

    def restore_sd():
        sdw = recipe.sd_first_conv(cfg, 0)
        conv = torch.nn.Conv2d(cfg.in_channels, cfg.model_channels, 3, padding=1)
        conv.load_state_dict({k: T(v) for k, v in sdw.items()})
        m.input_blocks[0][0] = conv
        m.first_conv_type = "SD"
    m.restore_first_conv_from_SD = restore_sd
    return m


@torch.no_grad()
def run_case(case):
    k = case["kind"]
    inp = {a: T(v) for a, v in tc.case_inputs(case).items()}
    if k == "position_net":
        m = mg.fill(PositionNet(in_dim=768, out_dim=768), "position_net", 0)
        return dict(out=m(*(inp[a] for a in KEYS)).numpy())
    if k == "unet":
        m = tiny_unet()
        set_alpha_scale, _ = mg.ref_interface_fns()
        set_alpha_scale(m, case["scale"])
        if case["sdconv"]:
            m.restore_first_conv_from_SD()
        g = m.grounding_tokenizer_input.prepare({a: inp[a] for a in KEYS})
        d = dict(x=inp["x"], timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
                 inpainting_extra_input=None, grounding_extra_input=None, grounding_input=g)
        return dict(out=m(d).numpy())
    raise ValueError(k)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    for case in tc.CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = os.path.join(outdir, case["name"] + ".npz")
        np.savez_compressed(path, **res)
        print(f"{case['name']:24s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {res['out'].shape}")


if __name__ == "__main__":
    main()
