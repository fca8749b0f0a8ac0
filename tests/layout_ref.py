"""numpy restatement of the layout terms of the reward (tools/metrics.py:29-42,58-75,93-144 as models/policy.py:126-135 calls
them), without scipy: the check of tests/golden/layout_ref.npz on the CPU and the model the HIP kernel (csrc/layout_reward.hip) is
read against.  Layouts are (boxes float64 [n, 4], label ids [n]).

The reference fills its matrices through np.meshgrid(range(n), range(m)) ('xy' indexing) and reshape(n, m): flat entry k holds
f(box1[k % n], box2[k // n]).  ``flat_matrix`` builds exactly that; ``true_matrix`` is the matrix a reader would expect
(entry (p, q) = f(box1[p], box2[q])), kept to show where the two differ.

The assignment maximises; it is solved by brute force over permutations when min(n, m) <= 6 and by an O(n^3) Hungarian
(shortest augmenting paths with potentials) otherwise.
"""
from __future__ import annotations

import itertools

import numpy as np

BRUTE_MAX = 6


def iou(b1, b2):
    """compute_iou of two boxes read as (l, t, r, b); 0/0 = NaN for two zero-area boxes"""
    l1, t1, r1, bb1 = (np.float64(v) for v in b1)
    l2, t2, r2, bb2 = (np.float64(v) for v in b2)
    a1, a2 = (r1 - l1) * (bb1 - t1), (r2 - l2) * (bb2 - t2)
    l_max, r_min, t_max, b_min = max(l1, l2), min(r1, r2), max(t1, t2), min(bb1, bb2)
    ai = (r_min - l_max) * (b_min - t_max) if (l_max < r_min and t_max < b_min) else np.float64(0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ai / (a1 + a2 - ai)


def bbox_sim(b1, c1, b2, c2):
    """__compute_bbox_sim of two boxes read as (cx, cy, w, h)"""
    if c1 != c2:
        return np.float64(0.0)
    cx1, cy1, w1, h1 = (np.float64(v) for v in b1)
    cx2, cy2, w2, h2 = (np.float64(v) for v in b2)
    delta_c = np.sqrt((cx1 - cx2) ** 2 + (cy1 - cy2) ** 2)
    delta_s = abs(w1 - w2) + abs(h1 - h2)
    area = min(w1 * h1, w2 * h2)
    return np.sqrt(max(area, np.float64(0.0))) * np.exp2(-1.0 * delta_c - 2.0 * delta_s)


def flat_matrix(f, n, m):
    """the reference's matrix: flat entry k = f(k % n, k // n), reshaped to (n, m)"""
    return np.array([f(k % n, k // n) for k in range(n * m)], dtype=np.float64).reshape(n, m)


def true_matrix(f, n, m):
    return np.array([[f(p, q) for q in range(m)] for p in range(n)], dtype=np.float64).reshape(n, m)


def brute_force_max(mat):
    """(best, runner-up) sums over all assignments of min(n, m) pairs; the runner-up is -inf when there is one assignment"""
    n, m = mat.shape
    if n > m:
        mat, n, m = mat.T, m, n
    sums = sorted((sum(mat[i, p[i]] for i in range(n)) for p in itertools.permutations(range(m), n)), reverse=True)
    return sums[0], (sums[1] if len(sums) > 1 else -np.inf)


def hungarian_max(mat):
    """sum of the best assignment of min(n, m) pairs, O(n^2 m): potentials + shortest augmenting paths on the negated matrix"""
    n, m = mat.shape
    if n > m:
        mat, n, m = mat.T, m, n
    if n == 0:
        return 0.0
    cost = -np.asarray(mat, dtype=np.float64)
    INF = float("inf")
    u, v = [0.0] * (n + 1), [0.0] * (m + 1)
    p, way = [0] * (m + 1), [0] * (m + 1)           # p[j]: row (1-based) assigned to column j, column 0 is the virtual start
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv, used = [INF] * (m + 1), [False] * (m + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, -1
            for j in range(1, m + 1):
                if not used[j]:
                    cur = cost[i0 - 1, j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            if j1 < 0:
                raise ValueError("no finite augmenting path")
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return float(sum(mat[p[j] - 1, j - 1] for j in range(1, m + 1) if p[j]))


def assignment_max(mat):
    n, m = mat.shape
    if min(n, m) == 0:
        return 0.0
    if np.isnan(mat).any():
        return float("nan")                          # the reference: scipy raises ValueError
    return float(brute_force_max(mat)[0]) if min(n, m) <= BRUTE_MAX else hungarian_max(mat)


def maximum_iou(layout_gt, layout_pred, matrix=flat_matrix):
    (bi, li), (bj, lj) = layout_gt, layout_pred
    bi, bj, li, lj = np.asarray(bi, np.float64).reshape(-1, 4), np.asarray(bj, np.float64).reshape(-1, 4), np.asarray(li), np.asarray(lj)
    score = 0.0
    for l in sorted(set(li.tolist())):
        _bi, _bj = bi[li == l], bj[lj == l]
        n, m = len(_bi), len(_bj)
        if m > 0:
            score += assignment_max(matrix(lambda a, b: iou(_bi[a], _bj[b]), n, m))
    return score / len(bi)


def docsim(layout_gt, layout_pred, matrix=flat_matrix):
    (b1, c1), (b2, c2) = layout_gt, layout_pred
    b1, b2, c1, c2 = np.asarray(b1, np.float64).reshape(-1, 4), np.asarray(b2, np.float64).reshape(-1, 4), np.asarray(c1), np.asarray(c2)
    N, M = len(b1), len(b2)
    if N >= M + 3 or N <= M - 3 or min(N, M) == 0:
        return 0.0
    return assignment_max(matrix(lambda a, b: bbox_sim(b1[a], c1[a], b2[b], c2[b]), N, M)) / min(N, M)


def unpack(z):
    """layout_ref.npz -> (cases, layouts_gt, layouts_pred, miou, docsim): padded arrays back to lists of (boxes, labels)"""
    names = [str(s) for s in z["names"]]
    gt = [(z["boxes_gt"][i, :n].copy(), z["labels_gt"][i, :n].copy()) for i, n in enumerate(z["n_gt"])]
    pred = [(z["boxes_pred"][i, :n].copy(), z["labels_pred"][i, :n].copy()) for i, n in enumerate(z["n_pred"])]
    return names, gt, pred, z["miou"], z["docsim"]
