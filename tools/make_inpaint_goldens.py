#!/usr/bin/env python3
"""Generate the inpainting goldens (tests/golden/vae_enc_*.npz, inpaint_*.npz, plms_inpaint_tiny.npz) by running the
REFERENCE itself (build container only), like tools/make_goldens.py, whose helpers are reused by import.

    python tools/make_inpaint_goldens.py            # writes only the files listed in OUTPUTS

  * vae_enc_tiny       AutoencoderKL.encode (autoencoder.py:34-38) at VAE_TINY on recipe weights, x [2, 3, 32, 32]; the CPU
                       noise that DiagonalGaussianDistribution.sample draws under torch.manual_seed(SEED), the posterior mean, z
  * vae_enc_names      names / shapes of encoder.* and quant_conv.* of the reference module at VAEConfig() and VAE_TINY
  * inpaint_masks      draw_masks_from_boxes (inpaint_mask_func.py:16-41, extracted with ast so that cv2 is not needed) on
                       border, sub-pixel, reversed, overlapping and all-zero boxes
  * inpaint_schedule   the reference's sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod buffers (ddpm.py:39-40)
  * plms_inpaint_tiny  PLMSSampler.sample(mask=..., x0=...) (plms.py:95-99) on the tiny UNet of plms_tiny, x0 of batch 1, mask
                       from the case's boxes; torch.randn_like replays a recorded noise list, stored with the draw shapes
"""
from __future__ import annotations

import ast
import contextlib
import io
import os
import random
import sys
from functools import partial

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (puts the reference, the repo and tests/ on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from layoutllm_t2i_amd import recipe  # noqa: E402
from layoutllm_t2i_amd.arch import VAE_TINY, VAEConfig  # noqa: E402
import golden_cases as gc  # noqa: E402

T = torch.from_numpy
SEED = 1234
OUTPUTS = ("vae_enc_tiny", "vae_enc_names", "inpaint_masks", "inpaint_schedule", "plms_inpaint_tiny")

# ltrb boxes (normalised) per sample, 4 rows each; all-zero rows are the padding of a real batch
MASK_BOXES = np.array([
    [[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]],          # whole image
    [[0.9, 0.9, 1.2, 1.3], [-0.1, 0.5, 0.2, 0.7], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]],         # past the borders
    [[0.30, 0.30, 0.31, 0.31], [0.5, 0.5, 0.5, 0.9], [0.7, 0.2, 0.6, 0.4], [0.8, 0.9, 0.9, 0.1]],      # sub-pixel, empty, reversed
    [[0.1, 0.1, 0.6, 0.6], [0.4, 0.4, 0.9, 0.8], [0.05, 0.7, 0.33, 0.99], [0.0, 0.0, 0.0, 0.0]],       # overlapping
    [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]],          # no box
], np.float32)
MASK_SIZES = (64, 16, 13)


def ref_draw_masks_from_boxes():
    src = open(os.path.join(mg.REF, "inpaint_mask_func.py")).read()
    keep = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "draw_masks_from_boxes"]
    ns = {"torch": torch, "random": random}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "inpaint_mask_func.py[subset]", "exec"), ns)
    return ns["draw_masks_from_boxes"]


def autoencoder(cfg: VAEConfig):
    from ldm.models.autoencoder import AutoencoderKL
    dd = dict(double_z=True, z_channels=cfg.z_channels, resolution=256, in_channels=cfg.out_ch, out_ch=cfg.out_ch, ch=cfg.ch,
              ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks, attn_resolutions=[], dropout=0.0)
    with contextlib.redirect_stdout(io.StringIO()):
        return AutoencoderKL(dd, cfg.embed_dim, scale_factor=cfg.scale_factor).eval()


def enc_inputs():
    return np.clip(recipe.normal("inpaint.enc.x", (2, 3, 32, 32), 5) * np.float32(0.5), -1, 1).astype(np.float32)


def plms_inputs():
    case = next(c for c in gc.CASES if c["name"] == "plms_tiny")
    inp = gc.case_inputs(case)
    x0 = (recipe.normal("inpaint.plms.x0", (1, 4, case["hw"], case["hw"]), 5) * np.float32(0.8)).astype(np.float32)
    return case, inp, x0


def replay_noise(tag: str):
    """A torch.randn_like stand-in: deterministic recipe noise per call, recorded (values and shapes)."""
    rec = []

    def randn_like(t, *a, **k):
        arr = recipe.normal(f"{tag}.{len(rec)}", tuple(t.shape), 7)
        rec.append(arr)
        return T(arr).to(t.device, t.dtype)
    return randn_like, rec


@torch.no_grad()
def run(name):
    if name == "vae_enc_tiny":
        m = autoencoder(VAE_TINY)
        sd = {n: T(np.asarray(v)) for n, v in {**recipe.vae_state_dict(VAE_TINY, 0), **recipe.vae_encoder_state_dict(VAE_TINY, 0)}.items()}
        m.load_state_dict(sd, strict=True)
        x = T(enc_inputs())
        moments = m.quant_conv(m.encoder(x))
        mean = torch.chunk(moments, 2, dim=1)[0]
        torch.manual_seed(SEED)
        z = m.encode(x)
        torch.manual_seed(SEED)
        noise = torch.randn(mean.shape)
        return dict(x=x.numpy(), noise=noise.numpy(), mean=mean.numpy(), z=z.numpy(), seed=np.int64(SEED))
    if name == "vae_enc_names":
        out = {}
        for tag, cfg in (("full", VAEConfig()), ("tiny", VAE_TINY)):
            sd = {k: v for k, v in autoencoder(cfg).state_dict().items() if k.startswith(("encoder.", "quant_conv."))}
            out[f"{tag}_names"] = np.array(list(sd), dtype="U96")
            out[f"{tag}_shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)
        return out
    if name == "inpaint_masks":
        draw = ref_draw_masks_from_boxes()
        out = dict(boxes=MASK_BOXES)
        for s in MASK_SIZES:
            out[f"mask_{s}"] = draw(T(MASK_BOXES), s).numpy()
        return out
    if name == "inpaint_schedule":
        diff = mg.LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
        return dict(sqrt_alphas_cumprod=diff.sqrt_alphas_cumprod.numpy(),
                    sqrt_one_minus_alphas_cumprod=diff.sqrt_one_minus_alphas_cumprod.numpy())
    if name == "plms_inpaint_tiny":
        case, inp, x0 = plms_inputs()
        inp = {k: T(v) for k, v in inp.items()}
        m = mg.tiny_unet()
        set_alpha_scale, alpha_generator = mg.ref_interface_fns()
        diff = mg.LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
        sampler = mg.PLMSSampler(diff, m, alpha_generator_func=partial(alpha_generator, type=case["alpha_type"]),
                                 set_alpha_scale=set_alpha_scale)
        batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
        g = m.grounding_tokenizer_input.prepare(batch, None)
        d = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], relations=inp["relations"],
                 grounding_input=g, inpainting_extra_input=None, grounding_extra_input=None)
        mask = ref_draw_masks_from_boxes()(inp["boxes"], case["hw"])
        shape = (case["B"], 4, case["hw"], case["hw"])
        fake, rec = replay_noise("inpaint.plms.noise")
        real = torch.randn_like
        torch.randn_like = fake
        try:
            out = sampler.sample(S=case["S"], shape=shape, input=d, uc=inp["uc"], guidance_scale=case["guidance"], mask=mask, x0=T(x0))
        finally:
            torch.randn_like = real
        res = dict(out=out.numpy(), x0=x0, mask=mask.numpy(), draw_shapes=np.array([list(a.shape) for a in rec], np.int64))
        res.update({f"noise_{i:03d}": a for i, a in enumerate(rec)})
        return res
    raise ValueError(name)


def main():
    outdir = os.path.join(mg.REPO, "tests", "golden")
    only = set(sys.argv[1:])
    for name in OUTPUTS:
        if only and name not in only:
            continue
        res = run(name)
        path = os.path.join(outdir, name + ".npz")
        np.savez_compressed(path, **res)
        print(f"{name:20s} -> {os.path.getsize(path) / 1024:8.1f} KiB  {sorted(res)[:6]}")


if __name__ == "__main__":
    main()
