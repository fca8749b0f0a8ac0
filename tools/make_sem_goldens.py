#!/usr/bin/env python3
"""Generate the semantic-map goldens (tests/golden/sem_*.npz) by running the REFERENCE itself (build container only), built as
tools/make_sp_goldens.py is and on top of it: the timm stand-in, the upstream UNet class and ``fill`` come from there by import.

    python tools/make_sem_goldens.py [name ...]        # writes only the cases of tests/sem_cases.py

The reference's ``sem_grounding_net.PositionNet``, ``sem_grounding_downsampler.GroundingDownsampler`` and ``openaimodel_original.UNetModel``
with both run on recipe weights by name; their input is the float one-hot of the case's uint8 class map, built here and never stored: OUTPUTS
only.  It works offline: ``convnext_tiny`` (which would fetch pretrained weights through torch.hub) is replaced in the grounding-net module by
a function returning ``ConvNeXt(depths, dims)`` of the case's size -- nothing calls torch.hub.  ``sem_params`` records the names and shapes of
the reference model's state dict; ``sem_prepare_batch`` runs the reference's own ``prepare_batch_sem`` (read from gligen_inference.py at run
time with ``ast``; torchvision's ``center_crop`` / ``PILToTensor`` get stand-ins of their documented arithmetic, and its colour visualisation
fails inside its own try / except and writes nothing), asserts that the result is exactly one-hot and stores the uint8 class map it argmaxes
to with a sha256 of the one-hot bytes.  Re-running rewrites the same bytes.
"""
from __future__ import annotations

import ast
import hashlib
import importlib
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_sp_goldens as ms  # noqa: E402  (the timm stand-in; puts the reference, the repo and tests/ on sys.path)

mn, mg = ms.mn, ms.mg

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from layoutllm_t2i_amd import recipe  # noqa: E402
import sem_cases as sm  # noqa: E402

T = torch.from_numpy


def net_module(cfg):
    """sem_grounding_net with ``convnext_tiny`` replaced by the case's backbone (no download)"""
    mod = importlib.import_module("ldm.modules.diffusionmodules.sem_grounding_net")
    mod.convnext_tiny = lambda pretrained=False, **kw: ms.ref_convnext.ConvNeXt(depths=list(cfg.convnext_depths), dims=list(cfg.convnext_dims))
    return mod


def ds_class():
    return importlib.import_module("ldm.modules.diffusionmodules.sem_grounding_downsampler").GroundingDownsampler


def tiny_unet(cfg):
    net_module(cfg)
    tok, ds = sm.targets()
    m = mn.upstream_unet_class()(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                                 out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks,
                                 attention_resolutions=list(cfg.attention_resolutions), channel_mult=list(cfg.channel_mult),
                                 num_heads=cfg.num_heads, context_dim=cfg.context_dim, fuser_type="gatedSA",
                                 grounding_downsampler=dict(target=ds, params=dict(in_dim=cfg.sem_classes, resize_input=cfg.ds_resize_input,
                                                                                   out_dim=cfg.ds_out)),
                                 grounding_tokenizer=dict(target=tok, params=dict(in_dim=cfg.sem_classes, resize_input=cfg.sp_resize_input,
                                                                                  out_dim=cfg.pos_out_dim)))
    mg.fill(m, "", 0)
    m.grounding_tokenizer_input = importlib.import_module("grounding_input.sem_grounding_tokinzer_input").GroundingNetInput()
    m.grounding_downsampler_input = importlib.import_module("grounding_input.sem_grounding_downsampler_input").GroundingDSInput()

    def restore_sd():  # the reference hard-codes a 4->320 conv; same semantics, tiny width (as tools/make_goldens.py)
        sdw = recipe.sd_first_conv(cfg, 0)
        conv = torch.nn.Conv2d(cfg.in_channels, cfg.model_channels, 3, padding=1)
        conv.load_state_dict({k: T(v) for k, v in sdw.items()})
        m.input_blocks[0][0] = conv
        m.first_conv_type = "SD"
    m.restore_first_conv_from_SD = restore_sd
    return m


def reference_prepare_batch_sem():
    """prepare_batch_sem of the reference file, with stand-ins for the two torchvision calls it makes"""
    tree = ast.parse(open(os.path.join(mg.REF, "gligen_inference.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "prepare_batch_sem"]

    def center_crop(img, size):       # torchvision.transforms.functional.center_crop on a PIL image no smaller than the crop
        w, h = img.size
        top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
        return img.crop((left, top, left + size, top + size))

    class PILToTensor:
        def __call__(self, pic):      # an "L" image: [1, H, W]
            a = T(np.array(pic, dtype=np.uint8))
            return (a.unsqueeze(0) if a.dim() == 2 else a.permute(2, 0, 1)).contiguous()
    ns = {"torch": torch, "np": np, "device": "cpu", "Image": Image, "TF": types.SimpleNamespace(center_crop=center_crop),
          "transforms": types.SimpleNamespace(PILToTensor=PILToTensor), "batch_to_device": lambda batch, device: {k: v.to(device) for k, v in batch.items()}}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "gligen_inference.py[subset]", "exec"), ns)
    return ns["prepare_batch_sem"]


@torch.no_grad()
def run_case(case):
    k = case["kind"]
    cfg = sm.cfg_of(case)
    if k == "params":
        sd = tiny_unet(cfg).state_dict()
        return dict(names=np.array(list(sd)), shapes=np.array([",".join(str(s) for s in v.shape) for v in sd.values()]))
    if k == "prepare_batch":
        fn = reference_prepare_batch_sem()
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "sem.png")
            Image.fromarray(sm.test_image(), "L").save(path)
            os.chdir(d)                  # (should the visualisation ever succeed, its side file lands in the temporary directory)
            try:
                out = fn({"sem": path}, case["B"])
            finally:
                os.chdir(cwd)
        ref = out["sem"]
        assert tuple(ref.shape) == (case["B"], sm.CLASSES, 512, 512) and ref.dtype == torch.float32 and torch.equal(ref[0], ref[1])
        assert bool(((ref == 0) | (ref == 1)).all()) and bool((ref.sum(1) == 1).all()), "the reference's tensor is exactly one-hot"
        u8 = ref[0].argmax(0).to(torch.uint8)
        assert int(u8.min()) == 0 and int(u8.max()) == sm.CLASSES - 1
        return dict(map_u8=u8.numpy(), mask=out["mask"].numpy(), shape=np.array(ref.shape),
                    sha256=np.array(hashlib.sha256(ref.numpy().tobytes()).hexdigest()))
    inp = {a: T(v) for a, v in sm.case_inputs(case).items()}
    assert int(inp["sem"].min()) == 0 and int(inp["sem"].max()) == case["classes"] - 1
    oh = T(sm.onehot(inp["sem"].numpy(), case["classes"]))
    if k == "position_net":
        m = mg.fill(net_module(cfg).PositionNet(resize_input=cfg.sp_resize_input, in_dim=cfg.sem_classes, out_dim=cfg.pos_out_dim),
                    "position_net", 0)
        return dict(out=m(oh, inp["mask"]).numpy())
    if k == "downsampler":
        m = mg.fill(ds_class()(resize_input=cfg.ds_resize_input, in_dim=cfg.sem_classes, out_dim=cfg.ds_out), "downsample_net", 0)
        return dict(out=m(oh).numpy())
    if k == "unet":
        m = tiny_unet(cfg)
        set_alpha_scale, _ = mn.upstream_interface_fns()
        set_alpha_scale(m, case["scale"])
        if case["sdconv"]:
            m.restore_first_conv_from_SD()
        batch = {"sem": oh, "mask": inp["mask"]}
        g = m.grounding_tokenizer_input.prepare(batch)
        ctx = inp["context"]
        if case["grounding"] == "null":       # the unconditional pass of plms.py:118-121: null tokens, the SAME grounding_extra_input
            g, ctx = m.grounding_tokenizer_input.get_null_input(), inp["uc"]
        d = dict(x=inp["x"], timesteps=torch.tensor(case["t"], dtype=torch.long), context=ctx, inpainting_extra_input=None,
                 grounding_extra_input=m.grounding_downsampler_input.prepare(batch), grounding_input=g)
        seen = {}
        hooks = [m.position_net.register_forward_hook(lambda mod, a, o: seen.__setitem__("objs", o.numpy().copy())),
                 m.input_blocks[0].register_forward_hook(lambda mod, a, o: seen.__setitem__("h0", o.numpy().copy()))]
        out = m(d).numpy()
        for h in hooks:
            h.remove()
        return dict(out=out, objs=seen["objs"], h0=seen["h0"])
    raise ValueError(k)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    for case in sm.CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = os.path.join(outdir, case["name"] + ".npz")
        np.savez_compressed(path, **res)
        print(f"{case['name']:24s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {[v.shape for v in res.values()]}")


if __name__ == "__main__":
    main()
