#!/usr/bin/env python3
"""What the text_image grounding family costs (GPU box): a text handle and a text_image handle of the full configuration in ONE process.

    python tools/ti_probe.py [--out DIR] [--rounds R] [--iters K] [--no-parity]

forward : ms per UNet forward at 2B = 8 (4 latents of 64 x 64, [cond ; uncond]), fuser on (scale 1) and off (scale 0), graph replay, device
          events around K forwards, the two handles alternating within every round, median over the rounds (and the spread);
          set_conditioning ms (host clock around the call and a synchronise, median); kernel launches per forward; then, from eager
          forwards under torch.profiler, the kernels whose device time differs most between the two handles.
          -> DIR/ti_forward.txt
parity  : one sample, default and strict mode of a text_image handle, rel-L2 against tests/ti_ref.py (fp32, CPU) on the same random
          weights. -> DIR/ti_parity.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes and magnitudes matter here.
The text_image forward attends over N + 60 instead of N + 30 keys in the gated self-attention and normalises 32 more [x ; objs] rows per
sample; at 64 x 64 both key counts round to the same number of 64-key tiles on every level (65, 17, 5, 2).
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
import torch

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

DEV = "cuda:0"
T = torch.from_numpy


def cond_args(cfg, inp, B):
    """[cond ; uncond] conditioning of B latents: positional and keyword arguments of UNetEngine.set_conditioning"""
    z = torch.zeros_like
    cat = lambda a, b: torch.cat([a, b], 0).to(DEV)
    pe = inp["text_embeddings"] if cfg.grounding == "text_image" else inp["positive_embeddings"]
    args = [cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
            cat(inp["masks"], z(inp["masks"])), cat(pe, z(pe)), 64]
    kw = {}
    if cfg.grounding == "text_image":
        kw = {k: cat(inp[k], z(inp[k])) for k in ("text_masks", "image_masks", "image_embeddings")}
    return args, kw


def build(cfg, seed=0):
    sd = random_state_dict(cfg, DEV, seed)
    return UNetEngine(pack_state_dict(sd, cfg, DEV)), sd


def timed(eng, x, scale, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        eng.forward(x, 481.0, scale, False, 2)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def forward_report(rounds, iters, B=4, kernels=True):
    lines = [f"# tools/ti_probe.py forward: full configuration, 2B = {2 * B}, 64 x 64 latents, graph replay, {rounds} rounds x {iters} forwards, "
             "handles alternating per round"]
    engines = {}
    for name in ("text", "text_image"):
        cfg = dataclasses.replace(UNetConfig(), grounding=name)
        eng, _ = build(cfg)
        inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, B, 64, n_boxes=8, n_rel=3, seed=4321).items()}
        args, kw = cond_args(cfg, inp, B)
        sc = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.set_conditioning(*args, **kw)
            torch.cuda.synchronize()
            sc.append((time.perf_counter() - t0) * 1e3)
        engines[name] = (eng, inp["x"].to(DEV), sc)
    res = {(n, s): [] for n in engines for s in (1.0, 0.0)}
    for n, (eng, x, _) in engines.items():          # warm-up: capture both graphs of both handles
        for s in (1.0, 0.0):
            timed(eng, x, s, 3)
    launches = {}
    for r in range(rounds):
        for s in (1.0, 0.0):
            for n in (("text", "text_image") if r % 2 == 0 else ("text_image", "text")):
                eng, x, _ = engines[n]
                res[(n, s)].append(timed(eng, x, s, iters))
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
            lines.append(f"forward {tag} {n:10s}: {med[(n, s)]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f}), {launches[(n, s)]} launches")
        lines.append(f"forward {tag} text_image / text = {med[('text_image', s)] / med[('text', s)]:.4f}")
    for n, (_, _, sc) in engines.items():
        lines.append(f"set_conditioning {n:10s}: {statistics.median(sc[2:]):8.3f} ms (median of {len(sc) - 2} after 2 warm-up calls; first call {sc[0]:.1f} ms)")
    if kernels:
        lines += kernel_report(engines)
    return lines


def kernel_times(eng, x, reps=3):
    """{kernel name: (us per forward, launches per forward)} of eager forwards with the fuser on, from torch.profiler's device events"""
    from torch.profiler import ProfilerActivity, profile
    eng.use_graphs = False
    try:
        eng.forward(x, 481.0, 1.0, False, 2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                eng.forward(x, 481.0, 1.0, False, 2)
            torch.cuda.synchronize()
    finally:
        eng.use_graphs = True
    out = {}
    for ev in prof.key_averages():
        dt = getattr(ev, "device_time_total", None)
        if dt is None:
            dt = getattr(ev, "cuda_time_total", 0.0)
        if dt > 0 and str(getattr(ev, "device_type", "")).endswith("CUDA"):
            out[ev.key] = (dt / reps, ev.count / reps)
    return out


def kernel_report(engines, top=12):
    """where a difference between the two forwards goes: per-kernel device time (eager launches, profiler on: the sums are not the
    graph-replay forward times above), kernels ordered by |text_image - text|"""
    kt = {n: kernel_times(eng, x) for n, (eng, x, _) in engines.items()}
    a, b = kt["text"], kt["text_image"]
    tot = {n: sum(v[0] for v in d.values()) for n, d in kt.items()}
    lines = [f"# per-kernel device time of one eager forward, fuser on (torch.profiler; sum of kernels: text {tot['text'] / 1e3:.3f} ms, "
             f"text_image {tot['text_image'] / 1e3:.3f} ms, difference {(tot['text_image'] - tot['text']) / 1e3:+.3f} ms)",
             "# us text (launches) | us text_image (launches) | difference us | kernel"]
    names = sorted(set(a) | set(b), key=lambda k: -abs(b.get(k, (0, 0))[0] - a.get(k, (0, 0))[0]))
    for k in names[:top]:
        ta, ca = a.get(k, (0.0, 0))
        tb, cb = b.get(k, (0.0, 0))
        lines.append(f"{ta:10.1f} ({ca:5.1f}) | {tb:10.1f} ({cb:5.1f}) | {tb - ta:+9.1f} | {k[:110]}")
    return lines


def parity_report():
    import ti_ref
    cfg = dataclasses.replace(UNetConfig(), grounding="text_image", split_weights=True)
    eng, sd = build(cfg, seed=3)
    inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, 1, 64, n_boxes=8, n_rel=3, seed=4321).items()}
    g = {k: inp[k] for k in ti_ref.KEYS}
    eng.set_conditioning(inp["context"], inp["relations"], g["boxes"], g["masks"], g["text_embeddings"], 64, text_masks=g["text_masks"],
                         image_masks=g["image_masks"], image_embeddings=g["image_embeddings"])
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
        ref = ti_ref.unet_forward(osd, cfg, inp["x"], torch.tensor([481]), inp["context"], inp["relations"], g)
    rel = lambda a: float((a - ref).norm() / ref.norm())
    outside = lambda a: float(((a - ref).abs() > 1e-4 + 1e-3 * ref.abs()).float().mean())
    return ["# tools/ti_probe.py parity: full configuration, text_image handle (split weight layout), one 64 x 64 sample, 8 boxes grounded on a phrase,",
            "# an image or both, fuser scale 1, t = 481, against tests/ti_ref.py (fp32, CPU) with the same unrounded random weights",
            f"default mode: rel_l2 = {rel(out_d):.3e}, outside rtol 1e-3 / atol 1e-4: {outside(out_d) * 100:.2f} %",
            f"strict mode : rel_l2 = {rel(out_s):.3e}, outside rtol 1e-3 / atol 1e-4: {outside(out_s) * 100:.2f} %",
            f"(reference forward on the CPU: {time.perf_counter() - t0:.1f} s)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel table (torch.profiler) behind the forward times")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ti_probe.py measures on the GPU; none found")
    os.makedirs(a.out, exist_ok=True)
    jobs = [("ti_forward.txt", lambda: forward_report(a.rounds, a.iters, kernels=not a.no_kernels))]
    if not a.no_parity:
        jobs.append(("ti_parity.txt", parity_report))
    for name, fn in jobs:
        lines = fn()
        with open(os.path.join(a.out, name), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
