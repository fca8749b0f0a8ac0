"""VAE encode vs decode and masked vs unmasked sampling, same process on the GPU box.

    python tools/vae_encode_probe.py [reps] [--sampling]
    python tools/vae_encode_probe.py --trace          # only 10 graph-replayed B = 4 512^2 encodes (for rocprofv3 --kernel-trace --stats)

  * encode / decode of the real VAE with graph replay, interleaved, device-synchronised, >= 20 reps after warm-up, at
    (B = 1, 512^2), (B = 4, 512^2), (B = 2, 768^2); achieved TF/s from flops.vae_encoder_flops
  * gl_latent_blend alone at the 50-step sampler's latent shape (B = 4, 64 x 64)
  * --sampling: 50-step CFG sampling of the full UNet at bench configs[1]'s shape (B = 4, 8 boxes), masked vs unmasked
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from layoutllm_t2i_amd import flops, host, ops, recipe  # noqa: E402
from layoutllm_t2i_amd.arch import VAEConfig  # noqa: E402
from layoutllm_t2i_amd.vae import VAEDecoder  # noqa: E402

DEV = "cuda:0"
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args else 20


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    cfg = VAEConfig()
    sd = {**recipe.vae_state_dict(cfg, 0), **recipe.vae_encoder_state_dict(cfg, 0)}
    vae = VAEDecoder(sd, cfg, DEV)
    if "--trace" in sys.argv:
        x = torch.from_numpy(np.clip(recipe.normal("probe.x.4.512", (4, 3, 512, 512), 1) * np.float32(0.5), -1, 1)).to(DEV)
        n = torch.randn(4, 4, 64, 64, device=DEV)
        for _ in range(10):
            vae.encode(x, n)
        torch.cuda.synchronize()
        return
    print(f"[probe] device {torch.cuda.get_device_name(0)}, reps {REPS}")
    for B, side in ((1, 512), (4, 512), (2, 768)):
        x = torch.from_numpy(np.clip(recipe.normal(f"probe.x.{B}.{side}", (B, 3, side, side), 1) * np.float32(0.5), -1, 1)).to(DEV)
        n = torch.randn(B, 4, side // 8, side // 8, device=DEV)
        z = vae.encode(x, n)
        vae.decode(z)
        for _ in range(3):                                           # warm-up (capture happened above)
            vae.encode(x, n), vae.decode(z)
        te, td = [], []
        for _ in range(REPS):                                        # interleaved
            te += timed(lambda: vae.encode(x, n), 1)
            td += timed(lambda: vae.decode(z), 1)
        me, md = float(np.median(te)), float(np.median(td))
        tf = flops.vae_encoder_flops(cfg, B, side) / (me * 1e-3) / 1e12
        print(f"[probe] B={B} side={side}: encode {me:.3f} ms (min {min(te):.3f}, {tf:.1f} TF/s), decode {md:.3f} ms "
              f"(min {min(td):.3f}), encode/decode {me / md:.3f}")
    x = torch.randn(4, 4, 64, 64, device=DEV)
    x0, nz = torch.randn(1, 4, 64, 64, device=DEV), torch.randn(1, 4, 64, 64, device=DEV)
    m = host.draw_masks_from_boxes(torch.rand(4, 8, 4), 64).to(DEV)
    g = torch.cuda.CUDAGraph()
    ops.latent_blend(x, x0, nz, m, 0.5, 0.5)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        for _ in range(100):
            ops.latent_blend(x, x0, nz, m, 0.5, 0.5)
    g.replay()
    tb = timed(g.replay, REPS)
    print(f"[probe] gl_latent_blend B=4 64x64: {float(np.median(tb)) * 10:.2f} us per launch (100-launch graph replay)")
    if "--sampling" in sys.argv:
        sampling(vae)


def sampling(vae):
    from layoutllm_t2i_amd.arch import UNetConfig
    from layoutllm_t2i_amd.interface import denoise
    from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
    cfg = UNetConfig()
    model = UNetModel(cfg, recipe.state_dict(cfg, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(cfg, 0))
    model.grounding_tokenizer_input = GroundingNetInput()
    inp = {k: torch.from_numpy(v) for k, v in recipe.synth_inputs(cfg, 4, 64, n_boxes=8, seed=7).items()}
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
    am = (model, vae, None, LatentDiffusion(device=DEV), {})
    img = torch.from_numpy(np.clip(recipe.normal("probe.img", (1, 3, 512, 512), 1) * np.float32(0.5), -1, 1)).to(DEV)
    mask = host.draw_masks_from_boxes(inp["boxes"], 64).to(DEV)

    def run(masked):
        model.first_conv_type = "GLIGEN"
        mk, z0 = (mask, vae.encode(img)) if masked else (None, None)
        return denoise(am, inp["context"], inp["uc"], inp["relations"], batch, inp["x"].to(DEV), [0.3, 0.0, 0.7], 7.5, steps=50,
                       mask=mk, x0=z0)
    run(False), run(True)
    tu, tm = [], []
    for _ in range(3):
        tu += timed(lambda: run(False), 1)
        tm += timed(lambda: run(True), 1)
    mu, mm = float(np.median(tu)), float(np.median(tm))
    print(f"[probe] 50-step sampling B=4 64x64, 8 boxes: unmasked {mu:.1f} ms, masked incl. one B=1 encode {mm:.1f} ms "
          f"({100 * (mm / mu - 1):+.2f} %)")


if __name__ == "__main__":
    main()
