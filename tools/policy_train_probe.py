#!/usr/bin/env python3
"""Parity and time of the policy update on the GPU (GPU box).

    python tools/policy_train_probe.py [--out DIR] [--rounds R] [--iters K] [--skip-parity]

-> DIR/policy_train_parity.txt: per case of tests/policy_train_cases.py, the error of PolicyTrainer against the fp64 run of the torch
   restatement over e_ref (the fp32 run's own error, tests/golden/policy_train_ref.npz): loss, log_prob, grad_W, grad_b of one
   loss_and_grad, and W, bias, exp_avg, exp_avg_sq after the 5 chained steps.  The tests allow 4.
-> DIR/policy_train.txt: one PolicyTrainer.step (gl_policy_grad's four launches, gl_policy_adam_step's one, and the Python around them:
   the conversions of sel / reward and six torch.empty) at P = 8 and P = 64 prompts, N = 32, D = 768, E = 128, k = 2, next to torch's
   nn.Linear + autograd + optim.Adam for the same update on the same device; after a warm-up, device events around K calls on resident
   inputs, per call, median over R rounds (min, max).  Both are launch-bound at this size.  No threshold is applied: the files are the record.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import policy_cases as pc
import policy_train_cases as tc
from layoutllm_t2i_amd.policy import PolicyNetwork
from layoutllm_t2i_amd.policy_train import PolicyTrainer

DEV = "cuda:0"
GOT = {"loss": "loss", "log_prob": "log_prob", "grad_W": "grad_weight", "grad_b": "grad_bias"}


def trainer_for(config, lr=tc.LR):
    D, E = tc.CONFIGS[config]
    W, b = tc.layer(config)
    net = PolicyNetwork(D, E, device=DEV).load_state_dict({"weight": torch.from_numpy(W), "bias": torch.from_numpy(b)})
    return PolicyTrainer(net, lr=lr)


def err(got, want) -> float:
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - np.asarray(want, np.float64)).max())


def parity(out):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "policy_train_ref.npz"))
    names = gold["names"].tolist()
    keys = list(tc.OUTPUTS) + list(tc.CHAINED)
    lines = [f"PolicyTrainer against the fp64 run of the torch restatement, {torch.cuda.get_device_name(0)}: max abs error over e_ref (the fp32 run's "
             f"own error against fp64; the tests allow {pc.BOUND_FACTOR:.0f}); the last six after {tc.STEPS} chained steps at lr = {tc.LR:g}",
             f"{'case':34s}" + "".join(f" {k:>12s}" for k in keys)]
    worst = dict.fromkeys(keys, 0.0)
    for i, name in enumerate(names):
        case, seed = tc.CASES[i], int(gold["seeds"][i])
        prompt, cand = (torch.from_numpy(a).to(DEV) for a in tc.inputs(case, seed))
        sel, reward = gold[name + ".sel"], gold[name + ".reward"]
        r64 = tc.ref64(case, seed, sel)
        tr = trainer_for(case[0])
        got = tr.loss_and_grad(prompt, cand, sel[0], reward[0], case[4])
        ratios = [err(got[GOT[k]], r64[k][0]) / gold["e_ref"][i, j] for j, k in enumerate(tc.OUTPUTS)]
        for s in range(tc.STEPS):
            tr.step(prompt, cand, sel[s], reward[s], case[4])
        state = [tr.policy.weight, tr.policy.bias, tr.exp_avg[0], tr.exp_avg[1], tr.exp_avg_sq[0], tr.exp_avg_sq[1]]
        ratios += [err(t, r64[k]) / gold["e_ref"][i, len(tc.OUTPUTS) + j] for j, (k, t) in enumerate(zip(tc.CHAINED, state))]
        for k, r in zip(keys, ratios):
            worst[k] = max(worst[k], r)
        lines.append(f"{name:34s}" + "".join(f" {r:12.2e}" for r in ratios))
    lines.append(f"{'largest over ' + str(len(names)) + ' cases':34s}" + "".join(f" {worst[k]:12.2e}" for k in keys))
    dst = os.path.join(out, "policy_train_parity.txt")
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[1] + "\n" + lines[-1])
    print("wrote", dst)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def med(v):
    return f"{statistics.median(v):9.4f} (min {min(v):.4f}, max {max(v):.4f})"


def step_times(out, rounds, iters):
    D, E, N, k, T, lr = 768, 128, 32, 2, 1.0, 1e-7          # a small lr: hundreds of timed steps must not drive the softmax into underflow
    W, b = tc.layer("d768_e128")
    lines = [f"PolicyTrainer.step and torch's nn.Linear + autograd + optim.Adam for the same update, N = {N}, D = {D}, E = {E}, k = {k}, "
             f"{torch.cuda.get_device_name(0)}; ms per step, device events, median over {rounds} rounds of {iters} steps (min, max)"]
    g = torch.Generator(device=DEV).manual_seed(0)
    cand = 0.3 * torch.randn(N, D, device=DEV, generator=g)
    for P in (8, 64):
        prompt = 0.3 * torch.randn(P, D, device=DEV, generator=g)
        sel = torch.stack([torch.randperm(N, device=DEV, generator=g)[:k] for _ in range(P)])
        sel32 = sel.to(torch.int32)
        reward = torch.randn(P, device=DEV, generator=g, dtype=torch.float64)
        tr = trainer_for("d768_e128", lr)
        lin = torch.nn.Linear(D, E).to(DEV)
        lin.load_state_dict({"weight": torch.from_numpy(W), "bias": torch.from_numpy(b)})
        opt = torch.optim.Adam(lin.parameters(), lr=lr)

        def hip():
            tr.step(prompt, cand, sel32, reward, T)

        def ref():
            probs = torch.softmax(torch.mm(lin(prompt), lin(cand).t()) / T, dim=1)
            loss = (-torch.log(probs.gather(1, sel)).sum(1) * reward).sum()
            opt.zero_grad()
            loss.backward()
            opt.step()
        timed(hip, 5), timed(ref, 5)                                   # warm-up of this shape
        th, tt = [], []
        for _ in range(rounds):                                        # alternating, same box
            th.append(timed(hip, iters))
            tt.append(timed(ref, iters))
        dw = float((tr.policy.weight - lin.weight.detach()).abs().max())
        lines.append(f"P {P:2d}:  PolicyTrainer.step {med(th)}   torch {med(tt)}   torch / hip {statistics.median(tt) / statistics.median(th):6.2f}"
                     f"   max |W here - W torch| after {5 + rounds * iters} steps {dw:.2e}")
    dst = os.path.join(out, "policy_train.txt")
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--skip-parity", action="store_true")
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_train_probe needs a GPU: times are not measured on a CPU")
    os.makedirs(o.out, exist_ok=True)
    if not o.skip_parity:
        parity(o.out)
    step_times(o.out, o.rounds, o.iters)


if __name__ == "__main__":
    main()
