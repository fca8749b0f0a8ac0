"""Do rectangles run on the same fast paths as squares?  One process, one GPU: the 2B = 8 default-mode forward of the full model
(hipGraph replay) at 64 x 64, 64 x 96, 96 x 64 and 80 x 80, fuser on and off, interleaved rounds, median of the rounds.

80 x 80 (6400 tokens) is larger than 64 x 96 (6144) in every term, the N^2 attention included, and is a square: the yardstick.  A
rectangle slower than 80 x 80 in the same run points at a fallback tile or a lost graph.

    python tools/rect_probe.py [--rounds N] [--square-only] [--out FILE]

--square-only: 64 x 64 through the square entry alone; with GLIGEN_HIP_LIB=<another build of the library> this also loads a build
that predates the *_hw entries (the 64 x 64 before / after comparison).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
SQUARE_ONLY = "--square-only" in args
ROUNDS = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 7
OUT = args[args.index("--out") + 1] if "--out" in args else None
import layoutllm_t2i_amd._lib as _L
if SQUARE_ONLY:
    for name in ("gl_set_conditioning_hw", "gl_vae_decode_hw", "gl_vae_encode_hw"):
        _L.PROTOTYPES.pop(name, None)
from layoutllm_t2i_amd import flops, recipe
from layoutllm_t2i_amd.arch import UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

B, REPS_TIMED = 4, 10
SHAPES = [64] if SQUARE_ONLY else [64, (64, 96), (96, 64), 80]
dev = torch.device("cuda:0")
cfg = UNetConfig()
P = pack_state_dict(random_state_dict(cfg, dev, seed=0), cfg, dev, recipe.sd_first_conv(cfg, 0))
eng = UNetEngine(P)
z = torch.zeros_like
cat = lambda a, b: torch.cat([a, b], 0)
inputs = {s: {k: torch.from_numpy(v) for k, v in recipe.synth_inputs(cfg, B, s, n_boxes=8, n_rel=3, seed=1).items()} for s in SHAPES}


def condition(s):
    i = inputs[s]
    eng.set_conditioning(cat(i["context"], i["uc"]), cat(i["relations"], i["relations"]), cat(i["boxes"], z(i["boxes"])),
                         cat(i["masks"], z(i["masks"])), cat(i["positive_embeddings"], z(i["positive_embeddings"])), s)


res = {(s, fs): [] for s in SHAPES for fs in (1.0, 0.0)}
launches = {}
for rnd in range(ROUNDS + 1):                    # round 0 warms every shape up (code objects, pool growth) and is dropped
    for s in SHAPES:
        condition(s)
        x = inputs[s]["x"].to(dev)
        for fs in (1.0, 0.0):
            eng.forward(x, 481.0, fs, fs == 0.0, 2)          # capture for this shape
            eng.forward(x, 481.0, fs, fs == 0.0, 2)          # first replay
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS_TIMED):
                out = eng.forward(x, 481.0, fs, fs == 0.0, 2)
            e1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            if rnd:
                res[s, fs].append(e0.elapsed_time(e1) / REPS_TIMED)
            launches[s, fs] = eng.num_launches()

lines = [f"lib {os.path.basename(_L.LIB_PATH)}; 2B = {2 * B}, default mode, graph replay, {ROUNDS} interleaved rounds x {REPS_TIMED} forwards; ms per forward"]
med = {}
for s in SHAPES:
    h, w = (s, s) if isinstance(s, int) else s
    for fs in (1.0, 0.0):
        v = sorted(res[s, fs])
        med[s, fs] = v[len(v) // 2]
        tf = 2 * B * flops.unet_forward_flops(cfg, (h, w), fuser_on=fs != 0.0) / (med[s, fs] * 1e-3) / 1e12
        lines.append(f"{h:3d} x {w:3d} ({h * w:5d} tokens) fuser {'on ' if fs else 'off'}: median {med[s, fs]:7.3f} ms  min {v[0]:7.3f}  max {v[-1]:7.3f}  "
                     f"{tf:6.1f} TFLOP/s  {launches[s, fs]} launches")
if not SQUARE_ONLY:
    for fs in (1.0, 0.0):
        for s in ((64, 96), (96, 64)):
            lines.append(f"{s[0]} x {s[1]} / 80 x 80, fuser {'on ' if fs else 'off'}: {med[s, fs] / med[80, fs]:.3f} (tokens 0.960)")
print("\n".join(lines))
if OUT:
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")
