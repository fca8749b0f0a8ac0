#!/usr/bin/env python3
"""What the inpaint_mode first conv costs (GPU box): a text handle and an inpaint handle of the full configuration in ONE process, like
tools/ti_probe.py, whose timing and profiler helpers are reused by import.

    python tools/inpaint9_probe.py [--out DIR] [--rounds R] [--iters K] [--no-parity] [--no-kernels] [--text-parity]

forward : ms per UNet forward at 2B = 8 (4 latents of 64 x 64, [cond ; uncond]), fuser on (scale 1) and off (scale 0), graph replay, device
          events around K forwards, the two handles alternating within every round, median over the rounds (and the spread); ms per
          set_inpaint_extra (host clock around the call and a synchronise); kernel launches per forward; then, from eager forwards under
          torch.profiler, the kernels whose device time differs most between the two handles.
          -> DIR/inpaint9_forward.txt
parity  : one sample, default and strict mode of an inpaint handle (with --text-parity: and of a text handle on the same inputs), rel-L2
          against tests/inpaint9_ref.py (fp32, CPU) on the same random weights. -> DIR/inpaint9_parity.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes and magnitudes matter here.
The inpaint forward differs from the text forward in ONE launch: the pack kernel reads 5 more fp32 channels per pixel and fills 27 instead
of 12 of the 64 padded fp16 channels; the first conv multiplies the same one 64-channel K block either way.
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import ti_probe
from layoutllm_t2i_amd import host, recipe
from layoutllm_t2i_amd.arch import UNetConfig

DEV = "cuda:0"
T = torch.from_numpy
NAMES = ("text", "inpaint")


def extra_of(inp, B, hw=64):
    """cat([z0 * mask, mask]) from a random z0 and the mask of the sample's own boxes"""
    mask = host.draw_masks_from_boxes(inp["boxes"], hw)
    z0 = T(recipe.normal("probe.inpaint9.z0", (1, 4, hw, hw), 5)) * 0.8
    return torch.cat([z0 * mask, mask], 1)[:B].contiguous()


def forward_report(rounds, iters, B=4, kernels=True):
    lines = [f"# tools/inpaint9_probe.py forward: full configuration, 2B = {2 * B}, 64 x 64 latents, graph replay, {rounds} rounds x {iters} forwards, "
             "handles alternating per round"]
    engines, extra_ms = {}, []
    for name in NAMES:
        cfg = dataclasses.replace(UNetConfig(), inpaint_mode=name == "inpaint")
        eng, _ = ti_probe.build(cfg)
        inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, B, 64, n_boxes=8, n_rel=3, seed=4321).items()}
        args, kw = ti_probe.cond_args(cfg, inp, B)
        eng.set_conditioning(*args, **kw)
        if cfg.inpaint_mode:
            extra = extra_of(inp, B).to(DEV)
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.set_inpaint_extra(extra)
                torch.cuda.synchronize()
                extra_ms.append((time.perf_counter() - t0) * 1e3)
        engines[name] = (eng, inp["x"].to(DEV), None)
    res = {(n, s): [] for n in engines for s in (1.0, 0.0)}
    for n, (eng, x, _) in engines.items():          # warm-up: capture both graphs of both handles
        for s in (1.0, 0.0):
            ti_probe.timed(eng, x, s, 3)
    for r in range(rounds):
        for s in (1.0, 0.0):
            for n in (NAMES if r % 2 == 0 else NAMES[::-1]):
                eng, x, _ = engines[n]
                res[(n, s)].append(ti_probe.timed(eng, x, s, iters))
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
        for n in engines:
            v = res[(n, s)]
            lines.append(f"forward {tag} {n:8s}: {med[(n, s)]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f}), {launches[(n, s)]} launches")
        spread = max(max(res[(n, s)]) - min(res[(n, s)]) for n in engines)
        lines.append(f"forward {tag} inpaint / text = {med[('inpaint', s)] / med[('text', s)]:.4f}; inpaint - text = "
                     f"{med[('inpaint', s)] - med[('text', s)]:+.3f} ms, larger spread (max - min) of the two = {spread:.3f} ms")
    lines.append(f"set_inpaint_extra (Bs = {B}): {statistics.median(extra_ms[2:]):8.3f} ms (median of {len(extra_ms) - 2} after 2 warm-up calls; "
                 f"first call {extra_ms[0]:.2f} ms), once per image")
    if kernels:
        kt = {n: ti_probe.kernel_times(eng, x) for n, (eng, x, _) in engines.items()}
        a, b = kt["text"], kt["inpaint"]
        tot = {n: sum(v[0] for v in d.values()) for n, d in kt.items()}
        lines += [f"# per-kernel device time of one eager forward, fuser on (torch.profiler; sum of kernels: text {tot['text'] / 1e3:.3f} ms, "
                  f"inpaint {tot['inpaint'] / 1e3:.3f} ms, difference {(tot['inpaint'] - tot['text']) / 1e3:+.3f} ms)",
                  "# us text (launches) | us inpaint (launches) | difference us | kernel"]
        names = sorted(set(a) | set(b), key=lambda k: -abs(b.get(k, (0, 0))[0] - a.get(k, (0, 0))[0]))
        for k in names[:10]:
            ta, ca = a.get(k, (0.0, 0))
            tb, cb = b.get(k, (0.0, 0))
            lines.append(f"{ta:10.1f} ({ca:5.1f}) | {tb:10.1f} ({cb:5.1f}) | {tb - ta:+9.1f} | {k[:110]}")
        for k in sorted(set(a) | set(b)):
            if "pack_latent" in k:
                lines.append(f"# {k[:80]}: text {a.get(k, (0.0, 0))[0]:.1f} us, inpaint {b.get(k, (0.0, 0))[0]:.1f} us")
    return lines


def parity_of(name):
    import inpaint9_ref
    from oracle import unet_ref
    cfg = dataclasses.replace(UNetConfig(), inpaint_mode=name == "inpaint", split_weights=True)
    eng, sd = ti_probe.build(cfg, seed=3)
    inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, 1, 64, n_boxes=8, n_rel=3, seed=4321).items()}
    g = dict(boxes=inp["boxes"], masks=inp["masks"], positive_embeddings=inp["positive_embeddings"])
    eng.set_conditioning(inp["context"], inp["relations"], g["boxes"], g["masks"], g["positive_embeddings"], 64)
    extra = extra_of(inp, 1)
    if cfg.inpaint_mode:
        eng.set_inpaint_extra(extra)
    x = inp["x"].to(DEV)
    out_d = eng.forward(x, 481.0, 1.0, False, 1).clone().cpu()
    eng.set_option(50, 1)
    out_s = eng.forward(x, 481.0, 1.0, False, 1).clone().cpu()
    eng.set_option(50, 0)
    osd = {k: v.detach().float().cpu() for k, v in sd.items()}
    osd = {k: (v.reshape(()) if k.endswith(("alpha_attn", "alpha_dense")) else v) for k, v in osd.items()}
    del eng, sd
    torch.cuda.empty_cache()
    torch.set_num_threads(min(32, max(1, int(os.environ.get("OMP_NUM_THREADS", "16")))))
    t0 = time.perf_counter()
    with torch.no_grad():
        if cfg.inpaint_mode:
            ref = inpaint9_ref.unet_forward(osd, cfg, inp["x"], extra, torch.tensor([481]), inp["context"], inp["relations"], g)
        else:
            ref = unet_ref.unet_forward(osd, cfg, inp["x"], torch.tensor([481]), inp["context"], inp["relations"], g["boxes"], g["masks"],
                                        g["positive_embeddings"])
    rel = lambda a: float((a - ref).norm() / ref.norm())
    outside = lambda a: float(((a - ref).abs() > 1e-4 + 1e-3 * ref.abs()).float().mean())
    return [f"{name:8s} default mode: rel_l2 = {rel(out_d):.3e}, outside rtol 1e-3 / atol 1e-4: {outside(out_d) * 100:.2f} %",
            f"{name:8s} strict mode : rel_l2 = {rel(out_s):.3e}, outside rtol 1e-3 / atol 1e-4: {outside(out_s) * 100:.2f} %",
            f"({name}: reference forward on the CPU: {time.perf_counter() - t0:.1f} s)"]


def parity_report(with_text):
    lines = ["# tools/inpaint9_probe.py parity: full configuration (split weight layout), one 64 x 64 sample, 8 boxes, fuser scale 1, t = 481, against the",
             "# fp32 mirror on the CPU (tests/inpaint9_ref.py; the text handle: oracle/unet_ref.py) with the same unrounded random weights"]
    for name in (NAMES if with_text else NAMES[1:]):
        lines += parity_of(name)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--text-parity", action="store_true", help="also the text handle's parity on the same inputs and weights seed")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel table (torch.profiler) behind the forward times")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/inpaint9_probe.py measures on the GPU; none found")
    os.makedirs(a.out, exist_ok=True)
    jobs = []
    if not a.no_forward:
        jobs.append(("inpaint9_forward.txt", lambda: forward_report(a.rounds, a.iters, kernels=not a.no_kernels)))
    if not a.no_parity:
        jobs.append(("inpaint9_parity.txt", lambda: parity_report(a.text_parity)))
    for name, fn in jobs:
        lines = fn()
        with open(os.path.join(a.out, name), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
