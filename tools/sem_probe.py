#!/usr/bin/env python3
"""What semantic-map grounding costs (GPU box): a full-size sem handle next to a canny handle (same engine path: 12-channel first conv, 64
tokens), and the once-per-image front end from a class map and from the reference's float one-hot, in ONE process.

    python tools/sem_probe.py [--out DIR] [--rounds R] [--iters K]

Forward: ms per UNet forward at 2B = 8 (4 latents of 64 x 64, [cond ; null]), fuser on (scale 1, the GLIGEN 12-channel first conv reading
cat([x, extra])), default mode, graph replay, device events around K forwards, the two handles alternating within every round, median over
the rounds.  Front end (tokenizer + downsampler of one 512 x 512 image, B = 1, convnext_tiny, resize 256, 152 classes): host clock around the
calls and a synchronise, median after two warm-up calls, (a) from the uint8 class map on the host (262 144 bytes cross to the device), (b)
from the float one-hot on the host (159 383 552 bytes cross, then gl_sem_onehot_index), (c) the two gather convs and the conversion alone on
device-resident inputs.  -> DIR/sem_forward.txt

Weights are weights.random_state_dict (magnitudes of the recipe, generated on the device): only shapes matter here.  No threshold is applied:
the file reports the numbers.
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

from layoutllm_t2i_amd import ops, recipe
from layoutllm_t2i_amd.arch import UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.semantic import ClassMapInput, SemDownsampler, SemTokenizer
from layoutllm_t2i_amd.spatial import SpatialDownsampler, SpatialTokenizer
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

DEV = "cuda:0"
T = torch.from_numpy
NAMES = ("canny", "sem")
CLASSES = 152


def configs():
    sp = dataclasses.replace(UNetConfig(), relation=False, grounding="spatial", max_objs=64, ds_out=8, ds_resize_input=256, sp_resize_input=256)
    return {"canny": dataclasses.replace(sp, ds_kind="conv", ds_in=1), "sem": dataclasses.replace(sp, ds_kind="sem", ds_in=CLASSES)}


def host_ms(fn, n=7):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[2:]), ts[0]


def timed(eng, x, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        eng.forward(x, 481.0, 1.0, False, 2)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def report(rounds, iters, B=4):
    cfgs = configs()
    sds = {n: random_state_dict(cfgs[n], DEV, 0) for n in NAMES}
    own = ("position_net.", "downsample_net.")
    sds["sem"].update({k: v for k, v in sds["canny"].items() if not k.startswith(own)})       # one set of UNet tensors for both handles
    cmi = ClassMapInput(CLASSES, DEV)
    tok, ds = SemTokenizer(sds["sem"], cfgs["sem"], DEV, cmi), SemDownsampler(sds["sem"], cfgs["sem"], DEV, cmi)
    ctok, cds = SpatialTokenizer(sds["canny"], cfgs["canny"], DEV), SpatialDownsampler(sds["canny"], cfgs["canny"], DEV)
    g = torch.Generator().manual_seed(0)
    # 32 x 32 blocks of one class each, like a segmentation
    cm1 = torch.randint(0, CLASSES, (1, 16, 16), generator=g, dtype=torch.uint8).repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
    one = torch.ones(1)
    lines = ["## once-per-image front end, B = 1, one 512 x 512 map (tokenizer + downsampler)"]

    def front(src):
        cmi._last = None                                      # every call converts / uploads anew
        return tok.tokens(src, one), ds(src)
    med, first = host_ms(lambda: front(cm1))
    lines.append(f"from the class map (host uint8, {cm1.numel():>11,d} B in): {med:9.3f} ms (median of 5 after 2 warm-up calls; first call {first:.1f} ms)")
    oh = torch.nn.functional.one_hot(cm1.long(), CLASSES).permute(0, 3, 1, 2).float().contiguous()
    med_oh, first = host_ms(lambda: front(oh))
    lines.append(f"from the float one-hot (host fp32, {oh.numel() * 4:>11,d} B in): {med_oh:9.3f} ms (first call {first:.1f} ms), conversion included")
    lines.append(f"input bytes one-hot / class map = {oh.numel() * 4 / cm1.numel():.0f}; time one-hot / class map = {med_oh / med:.1f}")
    cmd, ohd = cm1.to(DEV), oh.to(DEV)
    with torch.cuda.device(DEV):
        e = lambda *s: torch.empty(*s, device=DEV)
        o3, o16, o8 = e(1, 3, 256, 256), e(1, 16, 128, 128), e(1, 8, 64, 64)
        u8, bad = torch.empty(1, 512, 512, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        for name, fn in (("gl_sem_gather_conv 3x3, 152 -> 3, 256 x 256 ", lambda: ops.sem_gather_conv(cmd, 256, tok.P["in_conv.table"], tok.P["in_conv.b"], 3, 1, 1, False, o3)),
                         ("gl_sem_gather_conv 4x4 s2, 152 -> 16, 128 x 128", lambda: ops.sem_gather_conv(cmd, 256, ds.table, ds.b0, 4, 2, 1, True, o16)),
                         ("gl_sem_conv4x4s2 16 -> 8, 64 x 64             ", lambda: ops.sem_conv4x4s2(o16, ds.w2, ds.b2, o8)),
                         ("gl_sem_onehot_index 152 x 512 x 512           ", lambda: ops.sem_onehot_index(ohd, u8, bad))):
            med, _ = host_ms(fn)
            lines.append(f"{name}: {med:9.3f} ms (device-resident input, host clock around launch + synchronise)")
    del oh, ohd
    lines.append("## default mode forward, 2B = 8, fuser on, GLIGEN conv")
    engines = {}
    fc = {k: T(v).to(DEV) for k, v in recipe.sd_first_conv(cfgs["canny"], 0).items()}
    inp = {k: T(v) for k, v in recipe.synth_inputs(dataclasses.replace(UNetConfig(), relation=False), B, 64, n_boxes=8, n_rel=3, seed=4321).items()}
    ctx = torch.cat([inp["context"], inp["uc"]], 0).to(DEV)
    for name in NAMES:
        eng = UNetEngine(pack_state_dict(sds[name], cfgs[name], DEV, fc))
        if name == "sem":
            m = cm1.repeat(B, 1, 1)
            objs, extra = torch.cat([tok.tokens(m, torch.ones(B)), tok.null_tokens().expand(B, -1, -1)], 0), ds(m)
        else:
            m = (torch.rand(B, 3, 512, 512, device=DEV) * 2 - 1).contiguous()
            objs, extra = torch.cat([ctok.tokens(m, torch.ones(B)), ctok.null_tokens().expand(B, -1, -1)], 0), cds(m)
        eng.set_conditioning_tokens(ctx, objs, 64)
        eng.set_grounding_extra(extra)
        engines[name] = (eng, inp["x"].to(DEV))
    del sds
    torch.cuda.empty_cache()
    res = {n: [] for n in NAMES}
    for n, (eng, x) in engines.items():          # warm-up: capture the graph of both handles
        timed(eng, x, 3)
    for r in range(rounds):
        for n in (NAMES if r % 2 == 0 else NAMES[::-1]):
            res[n].append(timed(*engines[n], iters))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in res.items()}
    for n in NAMES:
        lines.append(f"forward {n:5s}: {med[n]:8.3f} ms (min {min(res[n]):.3f}, max {max(res[n]):.3f})")
    lines.append(f"forward sem / canny = {med['sem'] / med['canny']:.4f} ({med['sem'] - med['canny']:+.3f} ms)")
    for n, (eng, _) in engines.items():
        lines.append(f"bytes {n:5s}: packed weights {eng.P.nbytes() / 2**20:9.1f} MiB, pool {eng.pool_bytes() / 2**20:9.1f} MiB")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sem_probe.py measures on the GPU; none found")
    os.makedirs(a.out, exist_ok=True)
    lines = [f"# tools/sem_probe.py: full configuration on the upstream block, convnext_tiny tokenizer (resize 256, 64 tokens), 152 classes, "
             f"2B = 8, 64 x 64 latents, graph replay, {a.rounds} rounds x {a.iters} forwards, handles alternating per round"]
    lines += report(a.rounds, a.iters)
    with open(os.path.join(a.out, "sem_forward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
