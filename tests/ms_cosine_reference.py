"""The reference's metric='cosine' mean shift (lib/utils/mean_shift.py) restated in float64 numpy — the four steps the HIP
kernels implement, each with a record of the decisions it took (top-two gaps, ties, branches), plus

  * input generators whose fp32 arithmetic is EXACT in every summation order (line, lattice, widen): every coordinate is
    0 or +-2^-k, every product and every partial sum of a dot product is a small dyadic number, so an fma chain, a 16-lane
    shuffle tree and an MFMA all give the same bits as float64 and the expected integers are unconditional;
  * two fp32 evaluations of the hill climbing in other summation orders (hill_climb_fp32_tiles here, the torch oracle in
    oracle/mean_shift_oracle.py), whose distance to float64 is the yardstick for the kernel's.

Embeddings are [n, d] rows, d = 64 or 128; planes() gives the [2, n, 64] layout of the 128-d kernels."""
from __future__ import annotations

import numpy as np

C = 64


def _d(X, v):
    """0.5 (1 - X v) (mean_shift.py:162, :184)."""
    return 0.5 * (1.0 - X @ v)


# ---- the four steps --------------------------------------------------------------------------------------------------
def select_seeds(X, m, first, init=None, num_init=0, candidates=None):
    """select_smart_seeds :128-189: the first seed is X[first] (:155), every next one the argmax of the running minimum of
    the cosine distances to the chosen seeds (:174-175, first index on ties).  With init [m, d] and num_init > 0 the first
    num_init rows count as chosen (:142-170): their distances enter the minimum, their indices stay -1, `first` is unused.
    Returns (indices [m], gaps [m]): gaps[i] = top-two gap of the argmax that chose seed i (inf where nothing was chosen
    by an argmax); an exact tie is gap 0.  A list given as `candidates` receives, per seed, the pixels tied for that argmax
    (ascending; empty where nothing was chosen by an argmax)."""
    X = np.asarray(X, np.float64)
    idx = -np.ones(m, np.int64)
    gaps = np.full(m, np.inf)
    if init is None or num_init == 0:
        idx[0] = int(first)
        dmin = _d(X, X[int(first)])
        start = 1
    else:
        init = np.asarray(init, np.float64)
        dmin = _d(X, init[0])
        for i in range(1, num_init):
            dmin = np.minimum(dmin, _d(X, init[i]))
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
        dmin = np.minimum(dmin, _d(X, X[i]))
    return idx, gaps


def seed_rows(X, idx, init=None):
    """The seed matrix of a selection: X[idx], the given rows of `init` where idx is -1.  Same dtype as X (bit-exact rows)."""
    X = np.asarray(X)
    out = X[np.maximum(idx, 0)].copy()
    if init is not None:
        out[idx < 0] = np.asarray(init)[idx < 0]
    return out


def hill_climb(X, Z, kappa, iters):
    """seed_hill_climbing_ball :79-109 with ball_kernel :26: W = exp(kappa Z X^T), Z <- W X / max(||W X||_2, 1e-12)."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64).copy()
    for _ in range(iters):
        W = np.exp(kappa * (Z @ X.T))
        Z = W @ X
        Z = Z / np.maximum(np.sqrt((Z * Z).sum(axis=1, keepdims=True)), 1e-12)
    return Z


def hill_climb_fp32_tiles(X, Z, kappa, iters, tile=16):
    """The same iteration evaluated in float32 in the order of a tiled kernel: per tile of 16 pixels S = Z X_t^T, W = exp(kappa
    S), partial = W X_t, the partials added tile after tile; then the fp32 normalisation.  Not the kernel's exact order (it
    sums per wave and per block, in a tree): a second, independent fp32 evaluation next to the torch oracle's."""
    X = np.asarray(X, np.float32)
    Z = np.asarray(Z, np.float32).copy()
    n, d = X.shape
    T = -(-n // tile)
    Xp = np.zeros((T * tile, d), np.float32)
    Xp[:n] = X
    valid = (np.arange(T * tile) < n).reshape(T, 1, tile)
    Xt = Xp.reshape(T, tile, d)
    k32 = np.float32(kappa)
    for _ in range(iters):
        S = np.matmul(Z[None], Xt.transpose(0, 2, 1))                    # [T, m, tile] fp32
        W = np.where(valid, np.exp(k32 * S), np.float32(0)).astype(np.float32)
        part = np.matmul(W, Xt)                                          # [T, m, d] fp32
        acc = np.zeros_like(Z)
        for t in range(T):
            acc = acc + part[t]
        nrm = np.maximum(np.sqrt((acc * acc).sum(axis=1, keepdims=True, dtype=np.float32)), np.float32(1e-12))
        Z = (acc / nrm).astype(np.float32)
    return Z


def seed_components(Z, eps):
    """connected_components :41-76: seeds in index order; an unlabelled seed i gathers every seed within eps (<=, :58-60)
    of it; if that ball holds more than one distinct label value, -1 counting as one (:66), it takes the MODE of the labels
    present (ties -> the smallest, :30-38), else a new label; EVERY member is overwritten (:74).
    Returns (labels [m], record): record counts the pairs (i < j) exactly at eps, the balls that held labelled seeds, the
    balls whose mode was tied, and the seeds whose existing label was replaced by a different one."""
    Z = np.asarray(Z, np.float64)
    m = Z.shape[0]
    D = 0.5 * (1.0 - Z @ Z.T)
    rec = dict(pairs_at_eps=int((np.triu(D == eps, 1)).sum()), balls_with_labelled=0, tied_modes=0, overwritten=0)
    lab = -np.ones(m, np.int64)
    nxt = 0
    for i in range(m):
        if lab[i] != -1:
            continue
        member = D[:, i] <= eps
        present = lab[member]
        if np.unique(present).shape[0] > 1:
            known = present[present != -1]
            vals, counts = np.unique(known, return_counts=True)
            label = int(vals[np.argmax(counts)])                         # vals ascend: the first maximum is the smallest label
            rec["balls_with_labelled"] += 1
            rec["tied_modes"] += int((counts == counts.max()).sum() > 1)
        else:
            label = nxt
            nxt += 1
        rec["overwritten"] += int(((lab[member] != -1) & (lab[member] != label)).sum())
        lab[member] = label
    return lab, rec


def assign(X, Z, seed_labels, num_unique=None):
    """mean_shift_smart_init :206-227: closest = argmin of the cosine distance (first index on ties); labels =
    seed_labels[closest]; then the largest cluster becomes 0 (:217-227): only labels in range(num) are counted, num =
    len(unique(seed_labels)) unless given, the first maximum wins, 0 and that label change places.
    Returns (labels [n], closest [n], nties [n]): nties = how many seeds sit exactly at the pixel's smallest distance."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64)
    sl = np.asarray(seed_labels, np.int64)
    D = 0.5 * (1.0 - X @ Z.T)
    closest = np.argmin(D, axis=1)
    nties = (D == D.min(axis=1, keepdims=True)).sum(axis=1)
    labels = sl[closest].copy()
    num = len(np.unique(sl)) if num_unique is None else int(num_unique)
    count = np.array([(labels == i).sum() for i in range(num)])
    big = int(np.argmax(count)) if num > 0 else 0
    if big != 0:
        a, b = labels == 0, labels == big
        labels[a] = big
        labels[b] = 0
    return labels, closest, nties


def cluster(X, kappa, m, iters, eps, first):
    """mean_shift_smart_init :192-229 end to end -> (labels, indices, Z, seed_labels).  With iters = 0 the seeds stay rows of
    X, so on exact inputs every output is exact."""
    X = np.asarray(X, np.float64)
    idx, _ = select_seeds(X, m, first)
    Z = hill_climb(X, X[idx], kappa, iters)
    sl, _ = seed_components(Z, eps)
    labels, _, _ = assign(X, Z, sl)
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


# ---- inputs whose fp32 arithmetic is exact ---------------------------------------------------------------------------
def line_base(rng):
    """A random vertex of {+-1/8}^64: exactly unit (64 / 64)."""
    return (rng.integers(0, 2, C) * 2 - 1).astype(np.float32) / np.float32(8)


def line(base, k):
    """p(k) = base with its first k signs flipped, k = 0..64 (an int or an array of ints -> rows).  p(j).p(k) = 1 - 2|j-k|/64,
    d(p(j), p(k)) = |j-k|/64; p(64) = -base.  Every product is +-1/64 and every partial sum a multiple of 1/64 below 2^24 of
    them, hence exact in fp32 in any order."""
    scalar = np.ndim(k) == 0
    k = np.atleast_1d(np.asarray(k, np.int64))
    assert ((k >= 0) & (k <= C)).all()
    sign = np.where(np.arange(C)[None, :] < k[:, None], -1.0, 1.0).astype(np.float32)
    out = sign * np.asarray(base, np.float32)[None, :]
    return out[0] if scalar else out


def lattice(rng, n, nnz):
    """n rows with nnz in {4, 16, 64} entries of +-1/sqrt(nnz) at random channels: exactly unit, every dot product a
    multiple of 1/nnz."""
    assert nnz in (4, 16, 64)
    out = np.zeros((n, C), np.float32)
    val = np.float32(1.0 / np.sqrt(nnz))
    for i in range(n):
        pos = rng.choice(C, nnz, replace=False)
        out[i, pos] = val * (rng.integers(0, 2, nnz) * 2 - 1)
    return out


def wide_positions(rng):
    """Where widen() puts the 64 channels among 128: channels 0..31 at 32 random places of the first 64-channel half,
    channels 32..63 at 32 random places of the second half.  Two line points with more than 32 flips each then differ in the
    second half ONLY, so a decision between them can be taken only by the second plane."""
    return np.concatenate([np.sort(rng.choice(C, 32, replace=False)), C + np.sort(rng.choice(C, 32, replace=False))])


def widen(P, pos):
    """[n, 64] -> [n, 128] with column j moved to pos[j], zeros elsewhere: all dot products (and so all decisions) kept."""
    P = np.asarray(P, np.float32)
    out = np.zeros((P.shape[0], 2 * C), np.float32)
    out[:, pos] = P
    return out


def planes(X):
    """[n, 128] rows -> the [2, n, 64] plane layout of the 128-d kernels (what mean_shift.to_planes does on the device)."""
    X = np.asarray(X)
    return np.ascontiguousarray(X.reshape(X.shape[0], 2, C).transpose(1, 0, 2))
