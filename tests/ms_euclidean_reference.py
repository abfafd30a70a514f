"""The reference's metric='euclidean' mean shift (lib/utils/mean_shift.py) restated in float64 numpy — the four steps
the HIP kernels implement, plus the margins the GPU tests use to tell real differences from fp32 near-ties."""
from __future__ import annotations

import numpy as np


def _dist(X, s):
    return np.sqrt(((X - s[None, :]) ** 2).sum(axis=1))


def select_seeds(X, m, first):
    """select_smart_seeds :128-187: d = ||x - s||_2, farthest point = argmax of the min over the chosen seeds (first index
    on ties).  Returns (indices [m], gaps [m]): gaps[i] = the top-two gap of the argmax that chose seed i (inf for i=0)."""
    X = np.asarray(X, np.float64)
    idx = [int(first)]
    gaps = [np.inf]
    dmin = _dist(X, X[first])
    for _ in range(1, m):
        i = int(np.argmax(dmin))
        top = dmin[i]
        rest = np.delete(dmin, i)
        gaps.append(float(top - rest.max()) if rest.size else np.inf)
        idx.append(i)
        dmin = np.minimum(dmin, _dist(X, X[i]))
    return np.array(idx), np.array(gaps)


def hill_climb(X, Z, kappa, iters):
    """seed_hill_climbing_ball :79-109: W = exp(-kappa ||z - x||^2), Z <- W X / max(rowsum(W), 1)."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64).copy()
    xx = (X * X).sum(axis=1)
    for _ in range(iters):
        d2 = np.maximum((Z * Z).sum(axis=1)[:, None] + xx[None, :] - 2.0 * Z @ X.T, 0.0)
        W = np.exp(-kappa * d2)
        Z = (W @ X) / np.maximum(W.sum(axis=1, keepdims=True), 1.0)
    return Z


def seed_components(Z, eps):
    """connected_components :41-76 with ||z_j - z_i||_2 <= eps; the label-mode rule of the reference."""
    Z = np.asarray(Z, np.float64)
    m = Z.shape[0]
    lab = -np.ones(m, np.int64)
    K = 0
    for i in range(m):
        if lab[i] != -1:
            continue
        member = _dist(Z, Z[i]) <= eps
        if np.unique(lab[member]).shape[0] > 1:
            t = lab[member]
            t = t[t != -1]
            vals, counts = np.unique(t, return_counts=True)
            label = int(vals[np.argmax(counts)])
        else:
            label = K
            K += 1
        lab[member] = label
    return lab


def cc_margin(Z, eps):
    """Smallest | ||z_j - z_i|| - eps | over the seed pairs: how far the components are from a threshold decision."""
    Z = np.asarray(Z, np.float64)
    D = np.sqrt(((Z[:, None, :] - Z[None, :, :]) ** 2).sum(axis=2))
    return float(np.abs(D - eps).min())


def assign(X, Z, seed_labels):
    """mean_shift_smart_init :206-227: argmin ||x - z||_2 (first index on ties), then the largest cluster becomes 0.
    Returns (labels [n], gap [n]): how much farther the nearest seed of ANOTHER label is than the nearest seed (a pixel
    whose gap is within fp32 noise may go either way; seeds of one label may tie freely)."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64)
    sl = np.asarray(seed_labels)
    D = np.sqrt(np.maximum((X * X).sum(1)[:, None] + (Z * Z).sum(1)[None, :] - 2.0 * X @ Z.T, 0.0))
    closest = np.argmin(D, axis=1)
    near = D[np.arange(D.shape[0]), closest]
    other = np.where(sl[None, :] != sl[closest][:, None], D, np.inf).min(axis=1)
    gap = other - near
    labels = sl[closest].copy()
    num = len(np.unique(seed_labels))
    count = np.array([(labels == i).sum() for i in range(num)])
    big = int(np.argmax(count))
    if big != 0:
        a, b = labels == 0, labels == big
        labels[a] = big
        labels[b] = 0
    return labels, gap


def cluster(X, kappa, m, iters, eps, first):
    """mean_shift_smart_init end to end -> (labels, indices, Z, seed_labels)."""
    idx, _ = select_seeds(X, m, first)
    Z = hill_climb(X, np.asarray(X, np.float64)[idx], kappa, iters)
    sl = seed_components(Z, eps)
    labels, _ = assign(X, Z, sl)
    return labels, idx, Z, sl


def labels_equal_up_to_permutation(a, b) -> bool:
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    if a.shape != b.shape:
        return False
    fwd, bwd = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or bwd.setdefault(y, x) != x:
            return False
    return True
