#!/usr/bin/env python3
"""What a forward costs without the rela_fuse chain (GPU box): a relation handle and a no-relation handle (UNetConfig.relation = False, the
upstream GLIGEN block) of the full configuration in ONE process.

    python tools/norel_probe.py [--out DIR] [--rounds R] [--iters K] [--no-strict]

ms per UNet forward at 2B = 8 (4 latents of 64 x 64, [cond ; uncond]), fuser on (scale 1) and off (scale 0), default mode and strict mode
(handles with the split weight layout), graph replay, device events around K forwards, the two handles alternating within every round,
median over the rounds (and the spread); set_conditioning ms (host clock around the call and a synchronise, median); kernel launches per
forward; bytes of the packed weights and of the activation pool.  -> DIR/norel_forward.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes and magnitudes matter here; the
no-relation handle's weights are the relation handle's minus the rela_fuse tensors.  The no-relation forward launches a strict subset of
the relation forward's kernels plus one LayerNorm(norm2) per transformer block that the relation handle fuses into rela_merge.  No
threshold is applied: the file reports the numbers.
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
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

DEV = "cuda:0"
T = torch.from_numpy
NAMES = ("relation", "no_relation")


def cond_args(cfg, inp):
    """[cond ; uncond] conditioning: the positional arguments of UNetEngine.set_conditioning"""
    z = torch.zeros_like
    cat = lambda a, b: torch.cat([a, b], 0).to(DEV)
    pe = inp["positive_embeddings"]
    rel = cat(inp["relations"], inp["relations"]) if cfg.relation else None
    return [cat(inp["context"], inp["uc"]), rel, cat(inp["boxes"], z(inp["boxes"])), cat(inp["masks"], z(inp["masks"])), cat(pe, z(pe)), 64]


def timed(eng, x, scale, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        eng.forward(x, 481.0, scale, False, 2)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def mode_report(strict, rounds, iters, B=4):
    mode = "strict" if strict else "default"
    lines = [f"## {mode} mode" + (" (split weight layout, option 50)" if strict else "")]
    engines = {}
    sd = random_state_dict(UNetConfig(), DEV, 0)        # one set of tensors for both handles
    for name in NAMES:
        cfg = dataclasses.replace(UNetConfig(), relation=name == "relation", split_weights=strict)
        eng = UNetEngine(pack_state_dict(sd, cfg, DEV))
        if strict:
            eng.set_option(50, 1)
        inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, B, 64, n_boxes=8, n_rel=3, seed=4321).items()}
        args = cond_args(cfg, inp)
        sc = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.set_conditioning(*args)
            torch.cuda.synchronize()
            sc.append((time.perf_counter() - t0) * 1e3)
        engines[name] = (eng, inp["x"].to(DEV), sc)
    del sd
    torch.cuda.empty_cache()
    res = {(n, s): [] for n in NAMES for s in (1.0, 0.0)}
    for n, (eng, x, _) in engines.items():          # warm-up: capture both graphs of both handles
        for s in (1.0, 0.0):
            timed(eng, x, s, 3)
    for r in range(rounds):
        for s in (1.0, 0.0):
            for n in (NAMES if r % 2 == 0 else NAMES[::-1]):
                eng, x, _ = engines[n]
                res[(n, s)].append(timed(eng, x, s, iters))
    launches = {}
    for n, (eng, x, _) in engines.items():
        eng.use_graphs = False
        for s in (1.0, 0.0):
            eng.forward(x, 481.0, s, False, 2)
            launches[(n, s)] = eng.num_launches()
        eng.use_graphs = True
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in res.items()}
    for s, tag in ((1.0, "fuser on "), (0.0, "fuser off")):
        for n in NAMES:
            v = res[(n, s)]
            lines.append(f"forward {tag} {n:11s}: {med[(n, s)]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f}), {launches[(n, s)]} launches")
        lines.append(f"forward {tag} no_relation / relation = {med[('no_relation', s)] / med[('relation', s)]:.4f}")
    for n, (eng, _, sc) in engines.items():
        lines.append(f"set_conditioning {n:11s}: {statistics.median(sc[2:]):8.3f} ms (median of {len(sc) - 2} after 2 warm-up calls; first call {sc[0]:.1f} ms)")
        lines.append(f"bytes {n:11s}: packed weights {eng.P.nbytes() / 2**20:9.1f} MiB, pool {eng.pool_bytes() / 2**20:9.1f} MiB")
    del engines
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-strict", action="store_true", help="default mode only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/norel_probe.py measures on the GPU; none found")
    os.makedirs(a.out, exist_ok=True)
    lines = [f"# tools/norel_probe.py: full configuration, 2B = 8, 64 x 64 latents, graph replay, {a.rounds} rounds x {a.iters} forwards, "
             "handles alternating per round"]
    for strict in ((False,) if a.no_strict else (False, True)):
        lines += mode_report(strict, a.rounds, a.iters)
    with open(os.path.join(a.out, "norel_forward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
