#!/usr/bin/env python3
"""Generate the keypoint goldens (tests/golden/kp_*.npz) by running the REFERENCE itself (build container only), like
tools/make_norel_goldens.py, from which the upstream UNet class, the alias of ``ldm.modules.attention`` and ``fill`` come by import.

    python tools/make_kp_goldens.py [name ...]        # writes only the cases of tests/kp_cases.py

The reference's ``keypoint_grounding_net.PositionNet`` and its ``keypoint_grounding_tokinzer_input.GroundingNetInput`` run alone and inside
``openaimodel_original.UNetModel``; recipe weights by name, recipe inputs, OUTPUTS only.  ``kp_params`` records the names and shapes of the
reference model's state dict; ``kp_prepare_batch`` runs the reference's own ``prepare_batch_kp`` on its own two-person meta (both read from
gligen_inference.py at run time with ``ast``: the file imports packages this container lacks).  Re-running rewrites the same bytes.
"""
from __future__ import annotations

import ast
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_norel_goldens as mn  # noqa: E402  (puts the reference, the repo and tests/ on sys.path)

mg = mn.mg

import numpy as np  # noqa: E402
import torch  # noqa: E402

from layoutllm_t2i_amd import recipe  # noqa: E402
import kp_cases as kc  # noqa: E402

from ldm.modules.diffusionmodules.keypoint_grounding_net import PositionNet  # noqa: E402
from grounding_input.keypoint_grounding_tokinzer_input import GroundingNetInput  # noqa: E402

T = torch.from_numpy


def tiny_unet(cfg):
    m = mn.upstream_unet_class()(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                                 out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks,
                                 attention_resolutions=list(cfg.attention_resolutions), channel_mult=list(cfg.channel_mult),
                                 num_heads=cfg.num_heads, context_dim=cfg.context_dim, fuser_type="gatedSA",
                                 grounding_tokenizer=dict(target=kc.KP_TARGET, params=dict(max_persons_per_image=cfg.max_persons,
                                                                                           out_dim=cfg.pos_out_dim)))
    mg.fill(m, "", 0)
    m.grounding_tokenizer_input = GroundingNetInput()

    def restore_sd():  # the reference hard-codes a 4->320 conv; same semantics, tiny width (as tools/make_goldens.py)
        sdw = recipe.sd_first_conv(cfg, 0)
        conv = torch.nn.Conv2d(cfg.in_channels, cfg.model_channels, 3, padding=1)
        conv.load_state_dict({k: T(v) for k, v in sdw.items()})
        m.input_blocks[0][0] = conv
        m.first_conv_type = "SD"
    m.restore_first_conv_from_SD = restore_sd
    return m


def reference_meta_and_batch_fn():
    """the keypoint entry of the reference's meta_list and its prepare_batch_kp, straight from the reference file"""
    tree = ast.parse(open(os.path.join(mg.REF, "gligen_inference.py")).read())
    meta = None
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "dict":
            kw = {k.arg: k.value for k in n.keywords}
            if "ckpt" in kw and "keypoint" in ast.literal_eval(kw["ckpt"]):
                meta = {k: ast.literal_eval(v) for k, v in kw.items()}
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "prepare_batch_kp"]
    ns = {"torch": torch, "device": "cpu", "batch_to_device": lambda batch, device: {k: v.to(device) for k, v in batch.items()}}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "gligen_inference.py[subset]", "exec"), ns)
    return meta, ns["prepare_batch_kp"]


@torch.no_grad()
def run_case(case):
    k = case["kind"]
    cfg = kc.cfg_of(case)
    if k == "params":
        sd = tiny_unet(cfg).state_dict()
        return dict(names=np.array(list(sd)), shapes=np.array([",".join(str(s) for s in v.shape) for v in sd.values()]))
    if k == "prepare_batch":
        meta, fn = reference_meta_and_batch_fn()
        out = fn(meta, case["B"], case["P"])
        return dict(locations=np.asarray(meta["locations"], np.float64), points=out["points"].numpy(), masks=out["masks"].numpy())
    inp = {a: T(v) for a, v in kc.case_inputs(case).items()}
    if k == "position_net":
        m = mg.fill(PositionNet(max_persons_per_image=cfg.max_persons, out_dim=cfg.pos_out_dim), "position_net", 0)
        return dict(out=m(inp["points"], inp["masks"]).numpy())
    if k == "unet":
        m = tiny_unet(cfg)
        set_alpha_scale, _ = mn.upstream_interface_fns()
        set_alpha_scale(m, case["scale"])
        if case["sdconv"]:
            m.restore_first_conv_from_SD()
        g = m.grounding_tokenizer_input.prepare({a: inp[a] for a in kc.KEYS})
        if case["grounding"] == "null":
            g = m.grounding_tokenizer_input.get_null_input()
        d = dict(x=inp["x"], timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], inpainting_extra_input=None,
                 grounding_extra_input=None, grounding_input=g)
        return dict(out=m(d).numpy())
    raise ValueError(k)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    for case in kc.CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = os.path.join(outdir, case["name"] + ".npz")
        np.savez_compressed(path, **res)
        print(f"{case['name']:24s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {[v.shape for v in res.values()]}")


if __name__ == "__main__":
    main()
