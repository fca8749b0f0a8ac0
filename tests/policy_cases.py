"""The cases of the policy-selection tests (tests/test_gpu_policy.py) and of tools/make_policy_goldens.py: inputs regenerated from seeds
(a 4099 x 768 pool does not fit a committed file), the fp64 evaluation of the reference formula, and the fp64 ranking.

A case is (config, N, P): its pool ``cand`` [N, D], its prompts [P, D], the layer of its config.  tests/golden/policy_ref.npz records, per
case, the seed that passed the generation-time checks, whether the case is planted, ``e_ref`` (the error of the reference's own fp32
evaluation) and check values that tie the regenerated inputs to the recorded ones.

Drawn cases: features ~ N(0, 1), W ~ N(0, 1) / sqrt(D), bias ~ 0.1 N(0, 1).  The golden tool redraws (next seed) until, for every prompt,
neighbouring scores among the first 33 ranks differ by more than 100 e_ref.  With 64 prompts and 33 ranks to keep apart (N >= 63) no
draw passes, so those cases are PLANTED: 40 rows at scattered places get a multiple of the prompts' common direction added (factors
100 * 1.1 ** j), which puts them on top for every prompt, well separated.
Tie cases copy rows: the copies' scores are bit-equal in any evaluation that treats rows alike, the expected order is the lower index first.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutllm_t2i_amd import recipe

CONFIGS = {"d768_e128": (768, 128), "d512_e128": (512, 128), "d768_identity": (768, None)}
NS = (1, 32, 63, 64, 65, 4099)
PS = (1, 3, 8, 64)
KS = (0, 1, 2, 8, 32)
RANKS = 33                      # the first max(KS) + 1 ranks are kept apart
GAP_FACTOR = 100.0              # ... by more than GAP_FACTOR * e_ref
BOUND_FACTOR = 4.0              # the kernel may deviate from fp64 by BOUND_FACTOR * e_ref
CASES = [(c, n, p) for c in CONFIGS for n in NS for p in PS]
# (case, [(source rank of prompt 0, destination index)]): the row at that fp64 rank is copied over the row at the index
TIE_CASES = {
    "ties_n65_k2": (("d768_e128", 65, 3), [(0, 64), (1, 2)]),               # rank 0 copied into the second block, rank 1 across k = 2
    "ties_n4099_k8": (("d768_e128", 4099, 3), [(0, 4098), (7, 70), (3, 1000)]),   # inside the top 8, and across the k = 8 boundary
    "ties_n32_identity": (("d768_identity", 32, 8), [(0, 31), (1, 0)]),
}


def case_name(case) -> str:
    return f"{case[0]}_n{case[1]}_p{case[2]}"


def planted(case) -> bool:
    return case[1] > 32 and case[2] > 8


def layer(config: str):
    """(W [E, D], bias [E]) fp32, or (None, None) for the identity"""
    D, E = CONFIGS[config]
    if E is None:
        return None, None
    return recipe.normal(f"policy.{config}.W", (E, D), 0) / np.float32(np.sqrt(D)), np.float32(0.1) * recipe.normal(f"policy.{config}.b", (E,), 0)


def folded(config: str, prompt: np.ndarray):
    """fp64 (v [P, D], c [P]) with scores = cand @ v.T + c"""
    W, b = layer(config)
    p = prompt.astype(np.float64)
    if W is None:
        return p, np.zeros(len(p))
    q = p @ W.astype(np.float64).T + b.astype(np.float64)
    return q @ W.astype(np.float64), q @ b.astype(np.float64)


@functools.lru_cache(maxsize=4)
def _drawn(config: str, N: int, P: int, seed: int):
    D = CONFIGS[config][0]
    shared = recipe.normal(f"policy.{config}.shared", (D,), seed)
    prompt = recipe.normal(f"policy.{config}.prompt.{P}", (P, D), seed) + shared
    cand = recipe.normal(f"policy.{config}.cand.{N}", (N, D), seed)
    return prompt, cand


def inputs(case, seed: int):
    """(prompt [P, D], cand [N, D]) fp32 of a case; planted cases get their 40 separated rows"""
    config, N, P = case
    prompt, cand = _drawn(config, N, P, seed)
    if planted(case):
        v, _ = folded(config, prompt)
        m = v.mean(0)
        m /= np.linalg.norm(m)
        cand = cand.copy()
        rows = (np.arange(40) * 101 + 7) % N
        cand[rows] += (100.0 * 1.1 ** np.arange(40))[:, None].astype(np.float32) * m.astype(np.float32)
    return prompt, cand


def tie_inputs(name: str, seed: int):
    case, copies = TIE_CASES[name]
    prompt, cand = inputs(case, seed)
    order = ranking(scores64(case[0], prompt, cand))[0]
    cand = cand.copy()
    for rank, dst in copies:
        cand[dst] = cand[order[rank]]
    return case, prompt, cand


def scores64(config: str, prompt: np.ndarray, cand: np.ndarray) -> np.ndarray:
    """(W p + b) . (W c + b) in fp64, the reference's formula and operation order"""
    W, b = layer(config)
    p, c = prompt.astype(np.float64), cand.astype(np.float64)
    if W is not None:
        W, b = W.astype(np.float64), b.astype(np.float64)
        p, c = p @ W.T + b, c @ W.T + b
    return p @ c.T


def ranking(s: np.ndarray) -> np.ndarray:
    """[P, N] indices by score descending, equal scores by the lower index (the stable sorted(..., reverse=True) of txt2img.py:429)"""
    return np.stack([np.lexsort((np.arange(s.shape[1]), -row)) for row in s])


def softmax64(s: np.ndarray, temperature: float) -> np.ndarray:
    x = s / temperature
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def min_gap(s: np.ndarray, order: np.ndarray, same_rows=None) -> float:
    """the smallest difference of neighbouring scores among the first RANKS ranks over all prompts (pairs of copied rows excepted)"""
    worst = np.inf
    for p in range(s.shape[0]):
        top = order[p, :min(RANKS, s.shape[1])]
        for a, b in zip(top[:-1], top[1:]):
            if same_rows is not None and same_rows(a, b):
                continue
            worst = min(worst, s[p, a] - s[p, b])
    return float(worst)


def expected_topk(order: np.ndarray, k: int) -> np.ndarray:
    """[P, k] int32 as gl_policy_select fills it: the first min(k, N) ranks, then -1"""
    P, N = order.shape
    out = np.full((P, k), -1, np.int32)
    out[:, :min(k, N)] = order[:, :k]
    return out
