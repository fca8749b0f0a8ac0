"""The cases of the policy-training tests (tests/test_gpu_policy_train.py, tests/test_policy_train_host.py) and of
tools/make_policy_train_goldens.py: inputs regenerated from seeds with recipe.normal, and the project's own torch restatement of the
reference's update (train_rl.py:167-172, :85-95, :119, :182-184): nn.Linear, torch.mm, F.softmax, torch.log, backward, torch.optim.Adam.

A case is (config, N, P, k, T): a pool ``cand`` [N, D], prompts [P, D], the layer of its config, and STEPS chained updates, each with its own
selection ``sel`` [P, k] and reward [P].  Step 0 alone is the loss / gradient case.  tests/golden/policy_train_ref.npz records, per case, the
seed that passed the generation-time checks, the selections (drawn by policy.sample_examples from the fp32 run's probabilities) and
rewards of every step, checksums that tie the regenerated inputs to the recorded ones, and ``e_ref``: the max abs error of the fp32 run
against the fp64 run, for loss / log_prob / grad_W / grad_b of step 0 and for W / bias / exp_avg / exp_avg_sq after the STEPS steps.

Drawn: features ~ 0.3 N(0, 1) (the scores stay O(1), so that at every temperature more than k candidates keep a probability above 1e-6),
W ~ N(0, 1) / sqrt(D), bias ~ 0.1 N(0, 1), rewards ~ N(0, 1) as doubles with reward[0] > 0, reward[1] = 0 exactly and reward[2] < 0 (P >= 3).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutllm_t2i_amd import recipe

CONFIGS = {"d768_e128": (768, 128), "d512_e100": (512, 100), "d4_e1": (4, 1)}
NS = ("k", 32, 63, 65, 257)
PS = (1, 3, 8, 64)
KS = (1, 2, 8, 32)
TS = (0.5, 1.0, 2.0)
STEPS = 5
LR = 1e-5          # of the chained steps: Adam moves every weight by about lr per step, all of them coherently, and at the trainer's 1e-3 one
                   # step shifts the scores by tens, so that after two the fp32 probabilities of the next selection underflow
FEATURE_SCALE = 0.3
MIN_PROB = 1e-6
HALF_ULP = 2.0 ** -25      # of an fp32 number in [1, 2), relative: the least e_ref a chained tensor's draw is accepted with
OUTPUTS = ("loss", "log_prob", "grad_W", "grad_b")
CHAINED = ("W", "bias", "exp_avg_W", "exp_avg_b", "exp_avg_sq_W", "exp_avg_sq_b")
HARD_CASE = ("d768_e128", 32, 8, 2, 0.05)     # features ~ N(0, 1): the fp32 softmax underflows, log gives -inf


def _cases():
    out = []
    for ci, config in enumerate(CONFIGS):                     # every config at every N
        for ni, n in enumerate(NS):
            j = ci * len(NS) + ni
            k = KS[1 + ci] if n == "k" else KS[(j + ci) % 4]          # (N = k = 1 has one probability, 1, and no gradient)
            out.append((config, k if n == "k" else n, PS[j % 4], k, TS[j % 3]))
    for pi, P in enumerate(PS):                               # every (P, k) at the trainer's shape
        for ki, k in enumerate(KS):
            out.append(("d768_e128", 32, P, k, TS[(pi + ki) % 3]))
    out += [("d512_e100", 257, 64, 32, 0.5), ("d4_e1", 65, 64, 8, 2.0), ("d4_e1", 257, 8, 32, 1.0), ("d512_e100", 63, 64, 2, 1.0),
            ("d768_e128", 257, 64, 8, 2.0), ("d512_e100", 32, 1, 32, 2.0), ("d4_e1", 32, 3, 2, 0.5), ("d768_e128", 65, 3, 32, 0.5)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


def case_name(case) -> str:
    return f"{case[0]}_n{case[1]}_p{case[2]}_k{case[3]}_t{case[4]:g}"


def layer(config: str):
    """(W [E, D], bias [E]) fp32"""
    D, E = CONFIGS[config]
    return (recipe.normal(f"policy_train.{config}.W", (E, D), 0) / np.float32(np.sqrt(D)),
            np.float32(0.1) * recipe.normal(f"policy_train.{config}.b", (E,), 0))


def inputs(case, seed: int, scale: float = FEATURE_SCALE):
    """(prompt [P, D], cand [N, D]) fp32"""
    config, N, P = case[:3]
    D = CONFIGS[config][0]
    name = case_name(case)
    return (np.float32(scale) * recipe.normal(f"policy_train.{name}.prompt", (P, D), seed),
            np.float32(scale) * recipe.normal(f"policy_train.{name}.cand", (N, D), seed))


def rewards(case, seed: int) -> np.ndarray:
    """[STEPS, P] doubles; for P >= 3 every step has reward[0] > 0, reward[1] == 0 and reward[2] < 0"""
    P = case[2]
    r = recipe.normal(f"policy_train.{case_name(case)}.reward", (STEPS, P), seed).astype(np.float64)
    r[r == 0] = 0.5
    if P >= 3:
        r[:, 0], r[:, 1], r[:, 2] = np.abs(r[:, 0]), 0.0, -np.abs(r[:, 2])
    return r


def run_torch(W, b, prompt, cand, reward, T, dtype, sels=None, draw=None, stable=False, lr=LR, linear=None, optimizer=None):
    """The restatement: len(reward) chained updates of an nn.Linear in ``dtype`` on the CPU.  ``sels`` [steps, P, k]: the selections (an
    entry outside [0, N) is skipped); None: ``draw(probs)`` makes each step's from that step's probabilities.  ``stable``: log_softmax
    in place of log(softmax) (the hard-range case's fp64 values).  ``linear`` / ``optimizer``: continue with these (the resume tests).
    Returns dict(loss, log_prob, grad_W, grad_b: per step; sel; min_sel_prob; W, bias and Adam's state after the last step; linear, optimizer)."""
    W, b = np.asarray(W), np.asarray(b)
    if linear is None:
        linear = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
        linear.load_state_dict({"weight": torch.from_numpy(W).to(dtype), "bias": torch.from_numpy(b).to(dtype)})
    if optimizer is None:
        optimizer = torch.optim.Adam(linear.parameters(), lr=lr)
    x, y = torch.from_numpy(np.asarray(prompt)).to(dtype), torch.from_numpy(np.asarray(cand)).to(dtype)
    N = y.shape[0]
    out = dict(loss=[], log_prob=[], grad_W=[], grad_b=[], sel=[], min_sel_prob=np.inf)
    for s in range(len(reward)):
        scores = torch.mm(linear(x), linear(y).t())
        if stable:
            logpi = torch.log_softmax(scores / T, dim=1)
            probs = logpi.exp()
        else:
            probs = torch.softmax(scores / T, dim=1)
            logpi = torch.log(probs)
        sel = torch.as_tensor(np.asarray(sels[s] if sels is not None else draw(probs.detach())), dtype=torch.int64)
        ok = (sel >= 0) & (sel < N)
        idx = sel.clamp(0, N - 1)
        log_prob = torch.where(ok, logpi.gather(1, idx), torch.zeros((), dtype=dtype)).sum(1)
        loss = (-log_prob * torch.from_numpy(np.asarray(reward[s], np.float64))).sum()      # the reward is a double tensor (its mIoU term is numpy's)
        optimizer.zero_grad()
        loss.backward()
        out["loss"].append(float(loss.detach()))
        out["log_prob"].append(log_prob.detach().double().numpy())
        out["grad_W"].append(linear.weight.grad.detach().double().numpy().copy())
        out["grad_b"].append(linear.bias.grad.detach().double().numpy().copy())
        out["sel"].append(sel.numpy())
        if ok.any():
            out["min_sel_prob"] = min(out["min_sel_prob"], float(probs.detach().gather(1, idx)[ok].min()))
        optimizer.step()
    st = optimizer.state
    out.update(W=linear.weight.detach().double().numpy(), bias=linear.bias.detach().double().numpy(),
               exp_avg_W=st[linear.weight]["exp_avg"].double().numpy(), exp_avg_b=st[linear.bias]["exp_avg"].double().numpy(),
               exp_avg_sq_W=st[linear.weight]["exp_avg_sq"].double().numpy(), exp_avg_sq_b=st[linear.bias]["exp_avg_sq"].double().numpy(),
               linear=linear, optimizer=optimizer)
    return out


def hard_selection() -> np.ndarray:
    """the fixed selection of HARD_CASE: row p takes candidates p and p + 11 (its fp32 probabilities are no distribution to draw from)"""
    N, P, k = HARD_CASE[1:4]
    return np.stack([(np.arange(k) * 11 + p) % N for p in range(P)]).astype(np.int32)


def checksum(prompt, cand) -> float:
    return float(prompt.astype(np.float64).sum() + 3.0 * cand.astype(np.float64).sum())


_REF64 = {}


def ref64(case, seed: int, sels, stable: bool = False, scale: float = FEATURE_SCALE):
    """the fp64 run of a case with the recorded selections, computed once and shared by the tests (which leave it unchanged)"""
    key = (case, seed, stable, scale, np.asarray(sels).tobytes())
    if key not in _REF64:
        W, b = layer(case[0])
        prompt, cand = inputs(case, seed, scale)
        _REF64[key] = run_torch(W, b, prompt, cand, rewards(case, seed)[:len(sels)], case[4], torch.float64, sels=sels, stable=stable)
    return _REF64[key]
