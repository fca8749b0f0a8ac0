"""Digest of the samplers' Python side on the GPU box, for A/B parity of two checkouts (tools/engine_digest.py does the same for two builds of
the library): a fixed list of tiny runs through ``interface.denoise`` -- TINY config, random weights from a fixed seed, an 8 x 8 latent,
S = 4 -- over every sampler, with and without a mask, with and without guidance, and each sampler's own keys; per case one line
    <case> latent=<sha256 of the final latent> rng=<sha256 of torch.get_rng_state() + torch.cuda.get_rng_state()> pool=<gl_pool_bytes>
The rng digest pins the number and order of the torch draws, the pool bytes the engine buffers' names and sizes.  Copy this file into the other
checkout's tools/ and run it there too; two checkouts that sample the same way print identical lines.
    timeout -k 10 240 python tools/sampler_digest.py > a.txt && (cd other && timeout -k 10 240 python tools/sampler_digest.py) > b.txt && diff a.txt b.txt
(each run a process of its own under its own time limit, the second only after the first ended clean)
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import TINY
from layoutllm_t2i_amd.interface import denoise
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel

dev = "cuda:0"
S, B, HW = 4, 2, 8
FUSER_ON = [1.0, 0.0, 0.0]


def case(name, sampler, mask=False, guidance=7.5, alpha_type=FUSER_ON, **keys):
    return dict(name=name, sampler=sampler, mask=mask, guidance=guidance, alpha_type=alpha_type, keys=keys)


CASES = [case(f"{s}{'_mask' if m else ''}_g{g}", s, mask=m, guidance=g) for s in ("plms", "ddim", "dpmpp_2m") for m in (False, True) for g in (1, 7.5)]
CASES += [
    case("plms_scale0_switches_first_conv", "plms", alpha_type=[0.3, 0.0, 0.7]),           # a scale-0 step: the SD first conv from then on
    case("ddim_scale0_switches_first_conv", "ddim", alpha_type=[0.3, 0.0, 0.7]),
    case("dpmpp_2m_scale0_switches_first_conv", "dpmpp_2m", alpha_type=[0.3, 0.0, 0.7]),
    case("ddim_eta1", "ddim", ddim_eta=1.0),
    case("ddim_eta1_mask", "ddim", mask=True, ddim_eta=1.0),
    case("ddim_quad", "ddim", ddim_discretize="quad"),
    case("dpmpp_2m_order1", "dpmpp_2m", dpm_order=1),
    case("dpmpp_2m_uniform", "dpmpp_2m", dpm_discretize="uniform"),
]

sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
model = UNetModel(TINY, recipe.state_dict(TINY, 0), device=dev, sd_first_conv=recipe.sd_first_conv(TINY, 0))
model.grounding_tokenizer_input = GroundingNetInput()
all_models = (model, None, None, LatentDiffusion(device=dev), {})
inp = {k: torch.from_numpy(v) for k, v in recipe.synth_inputs(TINY, B, HW, n_boxes=4, n_rel=3, seed=5).items()}
batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
g = torch.Generator().manual_seed(7)
x0 = torch.randn(1, 4, HW, HW, generator=g).to(dev)                      # batch 1: shared by the samples
mask = (torch.rand(B, 1, HW, HW, generator=g) > 0.5).float().to(dev)

for c in CASES:
    model.first_conv_type = "GLIGEN"                                     # the switch to the SD conv is permanent: every case starts before it
    torch.manual_seed(1234)
    lat = denoise(all_models, inp["context"], inp["uc"], inp["relations"], batch, inp["x"].to(dev), c["alpha_type"], c["guidance"], steps=S,
                  mask=mask if c["mask"] else None, x0=x0 if c["mask"] else None, sampler=c["sampler"], **c["keys"])
    torch.cuda.synchronize()
    rng = hashlib.sha256(torch.get_rng_state().numpy().tobytes() + torch.cuda.get_rng_state(0).numpy().tobytes()).hexdigest()
    print(f"{c['name']:40s} latent={sha(lat)} rng={rng} pool={model.engine.pool_bytes()}", flush=True)
