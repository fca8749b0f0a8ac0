#!/usr/bin/env python3
"""What keypoint grounding costs (GPU box): a text handle on the upstream block (UNetConfig.relation = False) and a keypoint handle (8 persons,
136 grounding tokens) of the full configuration in ONE process.

    python tools/kp_probe.py [--out DIR] [--rounds R] [--iters K]

ms per UNet forward at 2B = 8 (4 latents of 64 x 64, [cond ; null]), fuser on (scale 1) and off (scale 0), default mode, graph replay, device
events around K forwards, the two handles alternating within every round, median over the rounds (and the spread); set_conditioning ms (host
clock around the call and a synchronise, median); kernel launches per forward; bytes of the packed weights and of the activation pool.
-> DIR/kp_forward.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes and magnitudes matter here; the two
handles share every tensor outside position_net.  The forwards launch the same kernels; the keypoint handle's fuser sees N + 136 keys where
the text handle's sees N + 30: 67 / 19 / 7 / 4 key tiles of 64 per level against 65 / 17 / 5 / 2, and 106 more LayerNorm and QKV rows per
sample.  With the fuser off nothing of a forward depends on the family.  No threshold is applied: the file reports the numbers.
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
NAMES = ("text", "keypoint")


def configs():
    text = dataclasses.replace(UNetConfig(), relation=False)
    return {"text": text, "keypoint": dataclasses.replace(text, grounding="keypoint", max_objs=17 * 8)}


def conditioner(name, eng, cfg, B):
    """a no-argument callable that sets the [cond ; null] conditioning of the handle"""
    z = torch.zeros_like
    cat = lambda a, b: torch.cat([a, b], 0).to(DEV)
    inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, B, 64, n_boxes=8, n_rel=3, seed=4321).items()}
    ctx = cat(inp["context"], inp["uc"])
    if name == "keypoint":
        pts, m = cat(inp["points"], z(inp["points"])), cat(inp["masks"], z(inp["masks"]))
        return inp["x"].to(DEV), lambda: eng.set_conditioning_kp(ctx, pts, m, 64)
    pe = inp["positive_embeddings"]
    bx, m, pe = cat(inp["boxes"], z(inp["boxes"])), cat(inp["masks"], z(inp["masks"])), cat(pe, z(pe))
    return inp["x"].to(DEV), lambda: eng.set_conditioning(ctx, None, bx, m, pe, 64)


def timed(eng, x, scale, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        eng.forward(x, 481.0, scale, False, 2)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def report(rounds, iters, B=4):
    lines = ["## default mode"]
    engines = {}
    cfgs = configs()
    body = random_state_dict(cfgs["text"], DEV, 0)        # one set of tensors for both handles outside position_net
    for name in NAMES:
        cfg = cfgs[name]
        sd = {k: v for k, v in body.items() if not k.startswith("position_net.")}
        sd.update({k: v for k, v in random_state_dict(cfg, DEV, 0).items() if k.startswith("position_net.")} if name == "keypoint"
                  else {k: v for k, v in body.items() if k.startswith("position_net.")})
        eng = UNetEngine(pack_state_dict(sd, cfg, DEV))
        x, set_cond = conditioner(name, eng, cfg, B)
        sc = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            set_cond()
            torch.cuda.synchronize()
            sc.append((time.perf_counter() - t0) * 1e3)
        engines[name] = (eng, x, sc)
        del sd
    del body
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
            lines.append(f"forward {tag} {n:8s}: {med[(n, s)]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f}), {launches[(n, s)]} launches")
        lines.append(f"forward {tag} keypoint / text = {med[('keypoint', s)] / med[('text', s)]:.4f} "
                     f"(+{med[('keypoint', s)] - med[('text', s)]:.3f} ms)")
    for n, (eng, _, sc) in engines.items():
        lines.append(f"set_conditioning {n:8s}: {statistics.median(sc[2:]):8.3f} ms (median of {len(sc) - 2} after 2 warm-up calls; first call {sc[0]:.1f} ms)")
        lines.append(f"bytes {n:8s}: packed weights {eng.P.nbytes() / 2**20:9.1f} MiB, pool {eng.pool_bytes() / 2**20:9.1f} MiB")
    del engines
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kp_probe.py measures on the GPU; none found")
    os.makedirs(a.out, exist_ok=True)
    lines = [f"# tools/kp_probe.py: full configuration on the upstream block, 2B = 8, 64 x 64 latents, graph replay, {a.rounds} rounds x "
             f"{a.iters} forwards, handles alternating per round; keypoint = 8 persons, 136 grounding tokens (text: 30)"]
    lines += report(a.rounds, a.iters)
    with open(os.path.join(a.out, "kp_forward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
