#!/usr/bin/env python3
"""What the layout terms of the reward cost on the GPU (GPU box): gl_layout_reward at B = 16 for three layout shapes,
(boxes per layout, labels) = (8, 3), (30, 5), (30, 1), ground truth and prediction of the same size.

    python tools/layout_probe.py [--out DIR] [--rounds R] [--iters K]

Per shape, after a warm-up of the shape:
  * kernel: device events around K launches of gl_layout_reward on resident inputs, per launch, median over R rounds (and the spread);
  * call:   reward.layout_terms end to end (packing on the host, two host-to-device copies, the launch), host clock around K calls that
            end in a synchronise, per call, median over R rounds;
  * where scipy imports: a numpy / scipy restatement of compute_maximum_iou + compute_docsim for the same 16 pairs (tests/layout_ref.py's
    entries and fill order, scipy.optimize.linear_sum_assignment), host clock, median of R runs; and the largest difference between
    the two results.
-> DIR/layout_reward.txt.  No threshold is applied: the file is the record.  The kernel is 2 B = 32 waves on a 256-CU device, a chain
of dependent wave reductions: a latency figure, not a share of any peak.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import layout_ref as lr
from layoutllm_t2i_amd import _lib
from layoutllm_t2i_amd.reward import layout_terms, pack_layouts

DEV = "cuda:0"
SHAPES = ((8, 3), (30, 5), (30, 1))
B = 16


def layouts(n, k, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        lt, rb = rng.uniform(0.0, 0.35, (n, 2)), rng.uniform(0.55, 1.0, (n, 2))
        out.append((np.concatenate([lt, rb], 1), rng.integers(0, k, n).astype(np.int64)))
    return out


def resident_args(gt, pred):
    bg, lg, ng = pack_layouts(gt)
    bp, lp, npd = pack_layouts(pred)
    keep = [torch.from_numpy(x).to(DEV) for x in (bg, bp, lg, lp, ng, npd)] + [torch.empty(2, B, dtype=torch.float64, device=DEV), ng, npd]
    a = _lib.LayoutRewardArgs()
    a.boxes_gt, a.boxes_pred, a.labels_gt, a.labels_pred, a.n_gt, a.n_pred = (t.data_ptr() for t in keep[:6])
    a.n_gt_host, a.n_pred_host, a.B = ng.ctypes.data, npd.ctypes.data, B
    a.miou, a.docsim = keep[6][0].data_ptr(), keep[6][1].data_ptr()
    return a, keep


def kernel_ms(a, iters):
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _lib.check(l.gl_layout_reward(ctypes.byref(a), st), "gl_layout_reward")
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def call_ms(gt, pred, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = layout_terms(gt, pred, DEV)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, out


def scipy_terms(gt, pred, lsa):
    def best(mat):
        if min(mat.shape) == 0:
            return 0.0
        i, j = lsa(mat, maximize=True)
        return float(mat[i, j].sum())
    miou, docsim = [], []
    for (bi, li), (bj, lj) in zip(gt, pred):
        s = 0.0
        for l in set(li.tolist()):
            _bi, _bj = bi[li == l], bj[lj == l]
            if len(_bj):
                s += best(lr.flat_matrix(lambda p, q: lr.iou(_bi[p], _bj[q]), len(_bi), len(_bj)))
        miou.append(s / len(bi))
        N, M = len(bi), len(bj)
        docsim.append(0.0 if (N >= M + 3 or N <= M - 3 or min(N, M) == 0) else
                      best(lr.flat_matrix(lambda p, q: lr.bbox_sim(bi[p], li[p], bj[q], lj[q]), N, M)) / min(N, M))
    return np.array(miou), np.array(docsim)


def med(v):
    return f"{statistics.median(v):9.4f} (min {min(v):.4f}, max {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layout_probe needs a GPU: times are not measured on a CPU")
    try:
        from scipy.optimize import linear_sum_assignment as lsa
    except ImportError:
        lsa = None
    lines = [f"gl_layout_reward, B = {B}, {torch.cuda.get_device_name(0)}; ms, median over {o.rounds} rounds of {o.iters} (min, max)",
             "scipy restatement: " + ("numpy float64 + scipy.optimize.linear_sum_assignment on this box's CPU, one Python call per box pair" if lsa else "scipy does not import here: not measured")]
    for n, k in SHAPES:
        gt, pred = layouts(n, k, 10 * n + k), layouts(n, k, 10 * n + k + 1)
        a, keep = resident_args(gt, pred)
        kernel_ms(a, 20)                                   # warm-up of this shape: code object, clocks
        call_ms(gt, pred, 5)
        kern = [kernel_ms(a, o.iters) for _ in range(o.rounds)]
        call = []
        for _ in range(o.rounds):
            ms, out = call_ms(gt, pred, max(o.iters // 4, 1))
            call.append(ms)
        lines.append(f"boxes {n:2d} labels {k}:  kernel {med(kern)}   layout_terms call {med(call)}")
        if lsa:
            cpu = []
            for _ in range(max(o.rounds // 2, 1)):
                t0 = time.perf_counter()
                wm, wd = scipy_terms(gt, pred, lsa)
                cpu.append((time.perf_counter() - t0) * 1e3)
            dm = float(np.abs(out["miou"].cpu().numpy() - wm).max())
            dd = float(np.abs(out["laysim"].cpu().numpy() - wd).max())
            lines.append(f"                     scipy restatement {med(cpu)}   max |miou diff| {dm:.2e}  max |docsim diff| {dd:.2e}")
    os.makedirs(o.out, exist_ok=True)
    dst = os.path.join(o.out, "layout_reward.txt")
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", dst)


if __name__ == "__main__":
    main()
