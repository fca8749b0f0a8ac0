#!/usr/bin/env python3
"""Generate the spatial-grounding goldens (tests/golden/sp_*.npz) by running the REFERENCE itself (build container only), like
tools/make_kp_goldens.py, from which the upstream UNet class, the alias of ``ldm.modules.attention`` and ``fill`` come by import.

    python tools/make_sp_goldens.py [name ...]        # writes only the cases of tests/sp_cases.py

The reference's four ``*_grounding_net.PositionNet``, its three conv ``*_grounding_downsampler.GroundingDownsampler`` and the hed one, its
``convnext.ConvNeXt`` and ``openaimodel_original.UNetModel`` with a downsampler run on recipe weights by name and recipe inputs; OUTPUTS only.
It works offline: ``convnext.py`` imports three names from ``timm``, which get a stand-in module before the import, and ``convnext_tiny`` (which
would fetch pretrained weights through torch.hub) is replaced in each grounding-net module by a function returning ``ConvNeXt(depths, dims)`` of
the case's size -- nothing calls torch.hub.  ``sp_params`` records the names and shapes of the reference model's state dict;
``sp_prepare_batch`` runs the reference's own ``crop_and_resize`` / ``prepare_batch_{canny,hed,depth,normal}`` (read from gligen_inference.py at
run time with ``ast``: the file imports packages this container lacks; torchvision's ``center_crop`` / ``PILToTensor`` get stand-ins of their
documented arithmetic).  Re-running rewrites the same bytes.
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


def _timm_stand_in():
    """the three names convnext.py imports; none of them is used by a forward pass with drop_path = 0"""
    import torch

    class DropPath(torch.nn.Identity):
        def __init__(self, p=0.0):
            super().__init__()

    layers = types.ModuleType("timm.models.layers")
    layers.trunc_normal_ = lambda t, std=1.0: t
    layers.DropPath = DropPath
    registry = types.ModuleType("timm.models.registry")
    registry.register_model = lambda fn: fn
    models = types.ModuleType("timm.models")
    timm = types.ModuleType("timm")
    timm.models, models.layers, models.registry = models, layers, registry
    for name, mod in (("timm", timm), ("timm.models", models), ("timm.models.layers", layers), ("timm.models.registry", registry)):
        sys.modules.setdefault(name, mod)


_timm_stand_in()
import make_norel_goldens as mn  # noqa: E402  (puts the reference, the repo and tests/ on sys.path)

mg = mn.mg

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from layoutllm_t2i_amd import recipe  # noqa: E402
import sp_cases as sc  # noqa: E402

from ldm.modules.diffusionmodules import convnext as ref_convnext  # noqa: E402

T = torch.from_numpy
FAMS = ("canny", "hed", "depth", "normal")
MAP_KEY = dict(canny="canny_edge", hed="hed_edge", depth="depth", normal="normal")


def net_module(family, cfg):
    """the family's grounding-net module with ``convnext_tiny`` replaced by the case's backbone (no download)"""
    mod = importlib.import_module(f"ldm.modules.diffusionmodules.{family}_grounding_net")
    mod.convnext_tiny = lambda pretrained=False, **kw: ref_convnext.ConvNeXt(depths=list(cfg.convnext_depths), dims=list(cfg.convnext_dims))
    return mod


def ds_class(family):
    return importlib.import_module(f"ldm.modules.diffusionmodules.{family}_grounding_downsampler").GroundingDownsampler


def tiny_unet(cfg, family):
    net_module(family, cfg)
    tok, ds = sc.targets(family)
    dsp = dict(out_dim=cfg.ds_out) if family == "hed" else dict(resize_input=cfg.ds_resize_input, out_dim=cfg.ds_out)
    m = mn.upstream_unet_class()(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                                 out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks,
                                 attention_resolutions=list(cfg.attention_resolutions), channel_mult=list(cfg.channel_mult),
                                 num_heads=cfg.num_heads, context_dim=cfg.context_dim, fuser_type="gatedSA",
                                 grounding_downsampler=dict(target=ds, params=dsp),
                                 grounding_tokenizer=dict(target=tok, params=dict(resize_input=cfg.sp_resize_input, out_dim=cfg.pos_out_dim)))
    mg.fill(m, "", 0)
    m.grounding_tokenizer_input = importlib.import_module(f"grounding_input.{family}_grounding_tokinzer_input").GroundingNetInput()
    m.grounding_downsampler_input = importlib.import_module(f"grounding_input.{family}_grounding_downsampler_input").GroundingDSInput()

    def restore_sd():  # the reference hard-codes a 4->320 conv; same semantics, tiny width (as tools/make_goldens.py)
        sdw = recipe.sd_first_conv(cfg, 0)
        conv = torch.nn.Conv2d(cfg.in_channels, cfg.model_channels, 3, padding=1)
        conv.load_state_dict({k: T(v) for k, v in sdw.items()})
        m.input_blocks[0][0] = conv
        m.first_conv_type = "SD"
    m.restore_first_conv_from_SD = restore_sd
    return m


def reference_batch_fns():
    """crop_and_resize and the four prepare_batch_* of the reference file, with stand-ins for the two torchvision calls they make"""
    tree = ast.parse(open(os.path.join(mg.REF, "gligen_inference.py")).read())
    names = ["crop_and_resize"] + [f"prepare_batch_{f}" for f in FAMS]
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]

    def center_crop(img, size):       # torchvision.transforms.functional.center_crop on a PIL image no smaller than the crop
        w, h = img.size
        top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
        return img.crop((left, top, left + size, top + size))

    class PILToTensor:
        def __call__(self, pic):
            return T(np.array(pic, dtype=np.uint8)).permute(2, 0, 1).contiguous()
    ns = {"torch": torch, "device": "cpu", "Image": Image, "TF": types.SimpleNamespace(center_crop=center_crop),
          "transforms": types.SimpleNamespace(PILToTensor=PILToTensor), "batch_to_device": lambda batch, device: {k: v.to(device) for k, v in batch.items()}}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "gligen_inference.py[subset]", "exec"), ns)
    return {f: ns[f"prepare_batch_{f}"] for f in FAMS}


@torch.no_grad()
def run_case(case):
    k = case["kind"]
    cfg = sc.cfg_of(case)
    if k == "params":
        sd = tiny_unet(cfg, case["family"]).state_dict()
        return dict(names=np.array(list(sd)), shapes=np.array([",".join(str(s) for s in v.shape) for v in sd.values()]))
    if k == "prepare_batch":
        fns = reference_batch_fns()
        meta_key = dict(canny="canny_image", hed="hed_image", depth="depth", normal="normal")
        res = {}
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "map.png")
            Image.fromarray(sc.test_image()).save(path)
            outs = {f: fns[f]({meta_key[f]: path}, case["B"]) for f in FAMS}
        ref = outs["canny"]["canny_edge"]
        for f in FAMS:      # the four loaders are one computation
            assert torch.equal(outs[f][MAP_KEY[f]], ref) and torch.equal(outs[f]["mask"], outs["canny"]["mask"])
        u8 = torch.round((ref[0] * 0.5 + 0.5) * 255).to(torch.uint8)
        assert torch.equal((u8.float() / 255 - 0.5) / 0.5, ref[0]) and torch.equal(ref[0], ref[1])       # the stored bytes ARE the result
        res = dict(map_u8=u8.numpy(), mask=outs["canny"]["mask"].numpy(), shape=np.array(ref.shape),
                   sha256=np.array(hashlib.sha256(ref.numpy().tobytes()).hexdigest()))
        return res
    inp = {a: T(v) for a, v in sc.case_inputs(case).items()}
    if k == "position_net":
        res = {}
        for f in FAMS:
            m = mg.fill(net_module(f, cfg).PositionNet(resize_input=cfg.sp_resize_input, out_dim=cfg.pos_out_dim), "position_net", 0)
            res["out_" + f] = m(inp["map"], inp["mask"]).numpy()
        for f in FAMS[1:]:
            assert np.array_equal(res["out_" + f], res["out_canny"])
        if case["name"] != "sp_posnet_t4":
            res = dict(out_canny=res["out_canny"])
        return res
    if k == "downsampler":
        f = case["family"]
        m = ds_class(f)(out_dim=cfg.ds_out) if f == "hed" else ds_class(f)(resize_input=cfg.ds_resize_input, out_dim=cfg.ds_out)
        m = mg.fill(m, "downsample_net", 0)
        return dict(out=m(inp["map"]).numpy())
    if k == "unet":
        f = case["family"]
        m = tiny_unet(cfg, f)
        set_alpha_scale, _ = mn.upstream_interface_fns()
        set_alpha_scale(m, case["scale"])
        if case["sdconv"]:
            m.restore_first_conv_from_SD()
        batch = {MAP_KEY[f]: inp["map"], "mask": inp["mask"]}
        g = m.grounding_tokenizer_input.prepare(batch)
        ctx = inp["context"]
        if case["grounding"] == "null":       # the unconditional pass of plms.py:118-121: null tokens, the SAME grounding_extra_input
            g, ctx = m.grounding_tokenizer_input.get_null_input(), inp["uc"]
        d = dict(x=inp["x"], timesteps=torch.tensor(case["t"], dtype=torch.long), context=ctx, inpainting_extra_input=None,
                 grounding_extra_input=m.grounding_downsampler_input.prepare(batch), grounding_input=g)
        # two intermediates next to the output: the grounding tokens and the first conv's output (every sc.H0_STRIDE-th pixel of a large latent),
        # where the families' own arithmetic ends and the transformer blocks have not yet amplified rounding differences
        seen = {}
        hooks = [m.position_net.register_forward_hook(lambda mod, a, o: seen.__setitem__("objs", o.numpy().copy())),
                 m.input_blocks[0].register_forward_hook(lambda mod, a, o: seen.__setitem__("h0", o.numpy().copy()))]
        out = m(d).numpy()
        for h in hooks:
            h.remove()
        s = sc.h0_stride(case)
        return dict(out=out, objs=seen["objs"], h0=np.ascontiguousarray(seen["h0"][:, :, ::s, ::s]))
    raise ValueError(k)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    for case in sc.CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = os.path.join(outdir, case["name"] + ".npz")
        np.savez_compressed(path, **res)
        print(f"{case['name']:24s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {[v.shape for v in res.values()]}")


if __name__ == "__main__":
    main()
