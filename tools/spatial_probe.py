#!/usr/bin/env python3
"""What spatial grounding costs (GPU box): the ConvNeXt tokenizer stage and the grounding downsampler of a canny checkpoint at full size
(convnext_tiny, resize_input 256, 64 grounding tokens, 512 x 512 maps), and a canny handle next to a text handle on the upstream block, in ONE
process.

    python tools/spatial_probe.py [--out DIR] [--rounds R] [--iters K]

Tokenizer and downsampler: ms per call at B = 1 and B = 4 (host clock around the call and a synchronise: both run once per image, launch by
launch, no graph), median after two warm-up calls, and the tokenizer's launch count.  Forward: ms per UNet forward at 2B = 8 (4 latents of
64 x 64, [cond ; null]), fuser on (scale 1, the GLIGEN 12-channel first conv reading cat([x, extra])) and off (scale 0, the SD conv), default mode,
graph replay, device events around K forwards, the two handles alternating within every round, median over the rounds.
-> DIR/sp_forward.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes matter here.  The forwards launch the
same kernels; the canny handle's fuser sees N + 64 keys where the text handle's sees N + 30, and its first pack launch also reads the 8
extra channels.  No threshold is applied: the file reports the numbers.
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.spatial import SpatialDownsampler, SpatialTokenizer
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

DEV = "cuda:0"
T = torch.from_numpy
NAMES = ("text", "canny")


def configs():
    text = dataclasses.replace(UNetConfig(), relation=False)
    return {"text": text, "canny": dataclasses.replace(text, grounding="spatial", max_objs=64, ds_kind="conv", ds_in=1, ds_out=8,
                                                       ds_resize_input=256, sp_resize_input=256)}


def host_ms(fn, n=7):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[2:]), ts[0]


def timed(eng, x, scale, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        eng.forward(x, 481.0, scale, scale == 0.0 and eng.P.has_sd_conv, 2)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def report(rounds, iters, B=4):
    cfgs = configs()
    lines = ["## tokenizer stage and downsampler (once per image)"]
    body = random_state_dict(cfgs["text"], DEV, 0)
    sp_sd = random_state_dict(cfgs["canny"], DEV, 0)
    tok, ds = SpatialTokenizer(sp_sd, cfgs["canny"], DEV), SpatialDownsampler(sp_sd, cfgs["canny"], DEV)
    for b in (1, 4):
        m = (torch.rand(b, 3, 512, 512, device=DEV) * 2 - 1).contiguous()
        mask = torch.ones(b, device=DEV)
        med, first = host_ms(lambda: tok.tokens(m, mask))
        lines.append(f"tokenizer   B = {b}: {med:8.3f} ms (median of 5 after 2 warm-up calls; first call {first:.1f} ms)")
        med, first = host_ms(lambda: ds(m))
        lines.append(f"downsampler B = {b}: {med:8.3f} ms (first call {first:.1f} ms)")
    depths = cfgs["canny"].convnext_depths
    lines.append(f"tokenizer launches: {3 + sum(depths) * 4 + 3 * 2 + 1 + 3} (stem 3, {sum(depths)} blocks x 4, 3 downsamples x 2, assembly 1, linears 3)")
    lines.append("## default mode forward")
    engines = {}
    fc = {k: T(v).to(DEV) for k, v in recipe.sd_first_conv(cfgs["text"], 0).items()}
    for name in NAMES:
        cfg = cfgs[name]
        sd = dict(sp_sd) if name == "canny" else dict(body)
        if name == "canny":       # one set of tensors for both handles outside the first conv and position_net
            sd.update({k: v for k, v in body.items() if not k.startswith("position_net.") and k != "input_blocks.0.0.weight"})
        eng = UNetEngine(pack_state_dict(sd, cfg, DEV, fc))
        inp = {k: T(v) for k, v in recipe.synth_inputs(cfgs["text"], B, 64, n_boxes=8, n_rel=3, seed=4321).items()}
        ctx = torch.cat([inp["context"], inp["uc"]], 0).to(DEV)
        if name == "canny":
            m = (torch.rand(B, 3, 512, 512, device=DEV) * 2 - 1).contiguous()
            objs = torch.cat([tok.tokens(m, torch.ones(B)), tok.null_tokens().expand(B, -1, -1)], 0)
            extra = ds(m)
            set_cond = lambda eng=eng, ctx=ctx, objs=objs, extra=extra: (eng.set_conditioning_tokens(ctx, objs, 64), eng.set_grounding_extra(extra))
        else:
            z = torch.zeros_like
            cat = lambda a, b: torch.cat([a, b], 0).to(DEV)
            pe = inp["positive_embeddings"]
            bx, mk, pe = cat(inp["boxes"], z(inp["boxes"])), cat(inp["masks"], z(inp["masks"])), cat(pe, z(pe))
            set_cond = lambda eng=eng, ctx=ctx, bx=bx, mk=mk, pe=pe: eng.set_conditioning(ctx, None, bx, mk, pe, 64)
        sc, first = host_ms(set_cond)
        engines[name] = (eng, inp["x"].to(DEV), sc, first)
    del body, sp_sd
    torch.cuda.empty_cache()
    res = {(n, s): [] for n in NAMES for s in (1.0, 0.0)}
    for n, (eng, x, _, _) in engines.items():          # warm-up: capture both graphs of both handles
        for s in (1.0, 0.0):
            timed(eng, x, s, 3)
    for r in range(rounds):
        for s in (1.0, 0.0):
            for n in (NAMES if r % 2 == 0 else NAMES[::-1]):
                eng, x, _, _ = engines[n]
                res[(n, s)].append(timed(eng, x, s, iters))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in res.items()}
    for s, tag in ((1.0, "fuser on,  GLIGEN conv"), (0.0, "fuser off, SD conv    ")):
        for n in NAMES:
            v = res[(n, s)]
            lines.append(f"forward {tag} {n:5s}: {med[(n, s)]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f})")
        lines.append(f"forward {tag} canny / text = {med[('canny', s)] / med[('text', s)]:.4f} (+{med[('canny', s)] - med[('text', s)]:.3f} ms)")
    for n, (eng, _, sc, first) in engines.items():
        lines.append(f"set_conditioning {n:5s}: {sc:8.3f} ms (median of 5 after 2 warm-up calls; first call {first:.1f} ms)")
        lines.append(f"bytes {n:5s}: packed weights {eng.P.nbytes() / 2**20:9.1f} MiB, pool {eng.pool_bytes() / 2**20:9.1f} MiB")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/spatial_probe.py measures on the GPU; none found")
    os.makedirs(a.out, exist_ok=True)
    lines = [f"# tools/spatial_probe.py: full configuration on the upstream block, convnext_tiny tokenizer (resize 256, 64 tokens), 2B = 8, "
             f"64 x 64 latents, graph replay, {a.rounds} rounds x {a.iters} forwards, handles alternating per round"]
    lines += report(a.rounds, a.iters)
    with open(os.path.join(a.out, "sp_forward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
