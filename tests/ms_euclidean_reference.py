"""The reference's metric='euclidean' mean shift (lib/utils/mean_shift.py) restated in float64 numpy — the four steps
the HIP kernels implement, plus the margins the GPU tests use to tell real differences from fp32 near-ties, the records of
the decisions each step took (ties, branches) that tests/test_ms_euclidean_cases_host.py reads, and two fp32 evaluations of
the hill climbing in other orders (hill_climb_fp32_direct, hill_climb_fp32_tiles) whose distance to float64 is the yardstick
for the kernel's.  The exact input generators (line, lattice, widen, planes) are tests/ms_cosine_reference.py's."""
from __future__ import annotations

import numpy as np


def _dist(X, s):
    return np.sqrt(((X - s[None, :]) ** 2).sum(axis=1))


def select_seeds(X, m, first, init=None, num_init=0, candidates=None):
    """select_smart_seeds :128-187: d = ||x - s||_2, farthest point = argmax of the min over the chosen seeds (first index
    on ties).  With init [m, d] and num_init > 0 the first num_init rows count as chosen (:142-170): their distances enter
    the minimum, their indices stay -1, `first` is unused.
    Returns (indices [m], gaps [m]): gaps[i] = the top-two gap of the argmax that chose seed i (inf where nothing was chosen
    by an argmax); an exact tie is gap 0.  A list given as `candidates` receives, per seed, the pixels tied for that argmax
    (ascending; empty where nothing was chosen by an argmax)."""
    X = np.asarray(X, np.float64)
    idx = -np.ones(m, np.int64)
    gaps = np.full(m, np.inf)
    if init is None or num_init == 0:
        idx[0] = int(first)
        dmin = _dist(X, X[int(first)])
        start = 1
    else:
        init = np.asarray(init, np.float64)
        dmin = _dist(X, init[0])
        for i in range(1, num_init):
            dmin = np.minimum(dmin, _dist(X, init[i]))
        start = num_init
    if candidates is not None:
        candidates.extend(np.zeros(0, np.int64) for _ in range(start))
    for s in range(start, m):
        i = int(np.argmax(dmin))
        if candidates is not None:
            candidates.append(np.nonzero(dmin == dmin[i])[0])
        rest = np.delete(dmin, i)
        if rest.size:
            gaps[s] = float(dmin[i] - rest.max())
        idx[s] = i
        dmin = np.minimum(dmin, _dist(X, X[i]))
    return idx, gaps


def seed_rows(X, idx, init=None):
    """The seed matrix of a selection: X[idx], the given rows of `init` where idx is -1.  Same dtype as X (bit-exact rows)."""
    X = np.asarray(X)
    out = X[np.maximum(idx, 0)].copy()
    if init is not None:
        out[idx < 0] = np.asarray(init)[idx < 0]
    return out


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


def weight_sums(X, Z, kappa):
    """rowsum(W) of one iteration from the seeds Z, float64: what the update divides by where it exceeds 1."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64)
    d2 = np.maximum((Z * Z).sum(axis=1)[:, None] + (X * X).sum(axis=1)[None, :] - 2.0 * Z @ X.T, 0.0)
    return np.exp(-kappa * d2).sum(axis=1)


def hill_climb_fp32_direct(X, Z, kappa, iters):
    """The reference's euclidean branch (ball_kernel :21-24, :95-105) in torch float32 as it is written there: the distance
    from direct differences, torch.norm, pow 2, exp, torch.mm, clamp(min=1).  In chunks of seeds to bound the [m, n, d]
    difference tensor."""
    import torch
    X = torch.from_numpy(np.ascontiguousarray(X, np.float32))
    Z = torch.from_numpy(np.ascontiguousarray(Z, np.float32)).clone()
    step = max(1, (1 << 22) // max(1, X.shape[0] * X.shape[1]))
    for _ in range(iters):
        W = torch.cat([torch.exp(-kappa * torch.pow(torch.norm(Z[i:i + step].unsqueeze(1) - X.unsqueeze(0), dim=2), 2))
                       for i in range(0, Z.shape[0], step)])
        Z = torch.mm(W, X) / torch.clamp(W.sum(dim=1).unsqueeze(1), min=1.0)
    return Z.numpy()


def hill_climb_fp32_tiles(X, Z, kappa, iters, tile=16):
    """The same iteration in float32 in the order of a tiled kernel: ||x||^2 and ||z||^2 once, per tile of 16 pixels S = Z X_t^T,
    d2 = max(zz + xx - 2 S, 0), W = exp(-kappa d2), partial numerators W X_t and partial weight sums added tile after tile,
    then / max(sum, 1).  Not the kernel's exact order: a second, independent fp32 evaluation."""
    X = np.asarray(X, np.float32)
    Z = np.asarray(Z, np.float32).copy()
    n, d = X.shape
    T = -(-n // tile)
    Xp = np.zeros((T * tile, d), np.float32)
    Xp[:n] = X
    valid = (np.arange(T * tile) < n).reshape(T, 1, tile)
    Xt = Xp.reshape(T, tile, d)
    xx = (Xt * Xt).sum(axis=2, dtype=np.float32)[:, None, :]                # [T, 1, tile]
    k32 = np.float32(kappa)
    for _ in range(iters):
        zz = (Z * Z).sum(axis=1, dtype=np.float32)[None, :, None]          # [1, m, 1]
        S = np.matmul(Z[None], Xt.transpose(0, 2, 1))                       # [T, m, tile] fp32
        d2 = np.maximum((zz + xx) - np.float32(2) * S, np.float32(0))
        W = np.where(valid, np.exp(-k32 * d2), np.float32(0)).astype(np.float32)
        part = np.matmul(W, Xt)                                             # [T, m, d] fp32
        wpart = W.sum(axis=2, dtype=np.float32)                             # [T, m]
        acc = np.zeros_like(Z)
        wsum = np.zeros(Z.shape[0], np.float32)
        for t in range(T):
            acc = acc + part[t]
            wsum = wsum + wpart[t]
        Z = (acc / np.maximum(wsum, np.float32(1))[:, None]).astype(np.float32)
    return Z


def hill_climb_ulp(X, Z, kappa, iters, sign):
    """The float64 iteration with every squared distance moved by sign x one fp32 ulp of ||z||^2 + ||x||^2 before the clamp at
    0: the grain of the norm expansion, whose three terms cancel.  What it decides: a pixel that coincides with the seed is
    seen at distance 0 or at one ulp of 2 (weight 1 or 1 - 4.8e-6 at kappa = 20 while every other weight keeps its ratio),
    and a weight sum next to 1 falls on one side of the clamp or the other."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64).copy()
    xx = (X * X).sum(axis=1)
    for _ in range(iters):
        nn = (Z * Z).sum(axis=1)[:, None] + xx[None, :]
        d2 = np.maximum(nn - 2.0 * Z @ X.T + sign * np.spacing(nn.astype(np.float32)).astype(np.float64), 0.0)
        W = np.exp(-kappa * d2)
        Z = (W @ X) / np.maximum(W.sum(axis=1, keepdims=True), 1.0)
    return Z


def seed_components(Z, eps, record=False):
    """connected_components :41-76 with ||z_j - z_i||_2 <= eps; the label-mode rule of the reference (the mode of the labels
    present, ties -> the smallest; every member is overwritten).  With record=True returns (labels, record): the pairs
    (i < j) exactly at eps, the balls that held labelled seeds, the balls whose mode was tied, the seeds whose label was
    replaced by a different one."""
    Z = np.asarray(Z, np.float64)
    m = Z.shape[0]
    lab = -np.ones(m, np.int64)
    D = np.stack([_dist(Z, Z[i]) for i in range(m)], axis=1)
    rec = dict(pairs_at_eps=int((np.triu(D == eps, 1)).sum()), balls_with_labelled=0, tied_modes=0, overwritten=0)
    K = 0
    for i in range(m):
        if lab[i] != -1:
            continue
        member = D[:, i] <= eps
        if np.unique(lab[member]).shape[0] > 1:
            t = lab[member]
            t = t[t != -1]
            vals, counts = np.unique(t, return_counts=True)
            label = int(vals[np.argmax(counts)])
            rec["balls_with_labelled"] += 1
            rec["tied_modes"] += int((counts == counts.max()).sum() > 1)
        else:
            label = K
            K += 1
        rec["overwritten"] += int(((lab[member] != -1) & (lab[member] != label)).sum())
        lab[member] = label
    return (lab, rec) if record else lab


def cc_margin(Z, eps):
    """Smallest | ||z_j - z_i|| - eps | over the seed pairs: how far the components are from a threshold decision."""
    Z = np.asarray(Z, np.float64)
    D = np.sqrt(((Z[:, None, :] - Z[None, :, :]) ** 2).sum(axis=2))
    return float(np.abs(D - eps).min())


def _swap_largest(labels, seed_labels, num_unique=None):
    """:217-227: only labels in range(num) are counted, num = len(unique(seed_labels)) unless given; the first maximum wins;
    0 and that label change places."""
    num = len(np.unique(seed_labels)) if num_unique is None else int(num_unique)
    count = np.array([(labels == i).sum() for i in range(num)])
    big = int(np.argmax(count)) if num > 0 else 0
    if big != 0:
        a, b = labels == 0, labels == big
        labels[a] = big
        labels[b] = 0
    return labels


def assign(X, Z, seed_labels, num_unique=None):
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
    return _swap_largest(sl[closest].copy(), sl, num_unique), gap


def assign_exact(X, Z, seed_labels, num_unique=None):
    """The same step from direct differences (torch.norm(X - Z), :207-209) with its record, for inputs whose arithmetic is
    exact.  Returns (labels [n], closest [n], nties [n]): nties = how many seeds sit exactly at the pixel's smallest distance.
    A non-finite row has no smallest distance: argmin gives it seed 0 (the first NaN, numpy's and torch's rule), nties 0."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64)
    sl = np.asarray(seed_labels, np.int64)
    with np.errstate(invalid="ignore"):
        D = np.sqrt(np.stack([((X - z[None, :]) ** 2).sum(axis=1) for z in Z], axis=1))
        closest = np.argmin(D, axis=1)
        nties = (D == D.min(axis=1, keepdims=True)).sum(axis=1)
    return _swap_largest(sl[closest].copy(), sl, num_unique), closest, nties


def cluster(X, kappa, m, iters, eps, first):
    """mean_shift_smart_init end to end -> (labels, indices, Z, seed_labels)."""
    idx, _ = select_seeds(X, m, first)
    Z = hill_climb(X, np.asarray(X, np.float64)[idx], kappa, iters)
    sl = seed_components(Z, eps)
    labels, _ = assign(X, Z, sl)
    return labels, idx, Z, sl


def cluster_exact(X, m, eps, first):
    """The whole call without an iteration, every distance from direct differences -> (labels, indices, Z, seed_labels).
    The seeds stay rows of X, so on exact inputs every output is exact."""
    X = np.asarray(X, np.float64)
    idx, _ = select_seeds(X, m, first)
    Z = X[idx]
    sl = seed_components(Z, eps)
    labels, _, _ = assign_exact(X, Z, sl)
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
