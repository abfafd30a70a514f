"""The inputs of the cosine clustering tests, built once and shared by the CPU proof (test_ms_cosine_host.py: every
decision case is order-independent and hits the branch it was built for; every climb case is sensitive to one pixel) and
the GPU tests (test_ms_cosine_gpu.py).  Decision cases use tests/ms_cosine_reference.py's exact inputs only."""
from __future__ import annotations

import functools

import numpy as np

from tests import ms_cosine_reference as R
from unseenobjectclustering_amd import synth

KAPPA = 20.0
EPS_EXACT = 2.0 / 64.0          # exactly a distance of the line points
EPS_PRODUCT = 0.04              # the product's epsilon: between 2/64 and 3/64


def _base(seed=0):
    return R.line_base(np.random.default_rng(900 + seed))


# ---- 3a. hill climbing ------------------------------------------------------------------------------------------------
HC_TILE_M = [1] + [16 * k + 2 for k in range(1, 8)] + [16 * k + 9 for k in range(8)] + [16 * k for k in range(1, 9)]
HC_TILE_ITERS = [1, 10]
HC_EDGE_M = [100, 96]
HC_EDGE_N = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]
HC_WIDE = [(1961, 100), (1025, 96), (65, 25)]
WIDE_FIRST = 3                  # the first seed of the 128-d cases
HC_OVERREAD_N = [17, 65, 1025]
HC_STRIDED = (300, 144, 100)                    # batch, n, m: more items than the grid
HC_AFFINE = (256, 2048, 100, (0, 1, 127, 128, 255))   # batch, n, m, the fields compared


@functools.lru_cache(maxsize=None)
def _pool(seed, channels=64):
    """A clustered 60 x 80 field (4 objects, noise 0.05): the pool the climb cases draw their pixels from."""
    return synth.embedding_field(seed, 60, 80, channels, 4, 0.05)[0]


@functools.lru_cache(maxsize=None)
def hc_field(n, seed=1, channels=64):
    """n pixels of a clustered field in random order -> [n, channels] float32 unit rows (n = 1961: the 37 x 53 field itself)."""
    if n == 1961 and channels == 64:
        return synth.embedding_field(12 + seed, 37, 53, 64, 4, 0.05)[0]
    pool = _pool(30 + seed % 8, channels)
    rng = np.random.default_rng(1000 * seed + n)
    if n <= pool.shape[0]:
        return np.ascontiguousarray(pool[rng.choice(pool.shape[0], n, replace=False)])
    raise ValueError(n)


def hc_seeds(X, m, seed=0):
    """Z0 = m rows of X, without replacement where n >= m.  Returns (Z0, the row indices).  Seed 0 is the row nearest to the
    last pixel (the rest are drawn at random): a seed of another cluster gives the last pixel a weight of e^-18 and could
    not see it dropped, whatever the tolerance."""
    rng = np.random.default_rng(77 + 131 * seed + m)
    n = X.shape[0]
    idx = rng.choice(n, m, replace=n < m)
    if n >= 2:
        near = int(np.argmax(X[:-1].astype(np.float64) @ X[-1].astype(np.float64)))
        if near in idx:
            idx[idx == near] = idx[0]
        idx[0] = near
    return np.ascontiguousarray(X[idx]), idx


K_CLIMB = 4     # the kernel may be K times as far from float64 as the farther of two other fp32 evaluations (profiles/ms_cosine_error.md)


def climb_yardstick(X, Z0, kappa, iters):
    """(float64 result, deviation of the torch oracle from it, deviation of the 16-pixel-tile fp32 evaluation from it)."""
    import torch
    from oracle import mean_shift_oracle as O
    ref = R.hill_climb(X, Z0, kappa, iters)
    ora = O.hill_climb(torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(np.ascontiguousarray(Z0)), kappa, iters).numpy()
    til = R.hill_climb_fp32_tiles(X, Z0, kappa, iters)
    return ref, float(np.abs(ora - ref).max()), float(np.abs(til - ref).max())


def climb_tolerance(dev_oracle, dev_tiles):
    return K_CLIMB * max(dev_oracle, dev_tiles)


def hc_affine_field(b):
    """Field b of the 256 x 2048 batch: its own clustered field, every odd one negated, so that a seed fragment or a pixel
    tile taken from a neighbour is an O(1) error (exp(kappa z.x) collapses)."""
    X = synth.embedding_field(500 + b, 32, 64, 64, 4, 0.05)[0]
    return X if b % 2 == 0 else -X


def hc_mutations(X):
    """The single-pixel errors a tail mask, a clamp or a tile bound can make: the last pixel lost, the last pixel counted
    twice, the last full 16-pixel tile counted twice.  Only those that exist at this n and can change the result: with one
    pixel the new seed is that pixel whatever its weight, so counting it twice is invisible to any test."""
    n = X.shape[0]
    out = {}
    if n >= 2:
        out["last pixel dropped"] = X[:-1]
        out["last pixel twice"] = np.concatenate([X, X[-1:]])
    if n >= 17:
        full = (n // 16) * 16
        out["last full tile twice"] = np.concatenate([X, X[full - 16:full]])
    return out


# ---- 3b. farthest-point sampling -----------------------------------------------------------------------------------------
def _fps_line_ties():
    """n = 4100 line points, first = 7 (p0).  Fillers are p(k), k <= 7; the picks before them are engineered exact ties:
      step 1: p64 twice, pixels 100 | 2148          different blocks of both kernels (2048 pixels / 256 pixels per block)
      step 2: p32 twice, pixels 5 | 13              one 16-lane row group of both kernels
      step 3: p16 | p48 (distinct points), 70 | 130 different waves of one block
      step 5..: p8, p24, p40, p56 at 300 | 812 | 1500 | 3000: two pixel slots of one lane of the on-chip kernel (812 = 300 +
                512), different blocks of the streaming kernel
    then the fillers (hundreds of duplicates per value: every pick a many-way tie), then, all 16 distinct points chosen,
    every running minimum is exactly 0 and the picks are index 0."""
    rng = np.random.default_rng(41)
    ks = rng.integers(0, 8, 4100)
    ks[7] = 0
    for i, k in {100: 64, 2148: 64, 5: 32, 13: 32, 70: 16, 130: 48, 300: 8, 812: 24, 1500: 40, 3000: 56}.items():
        ks[i] = k
    return dict(X=R.line(_base(1), ks), m=24, first=7, ties={1: (100, 2148), 2: (5, 13), 3: (70, 130), 5: (300, 812, 1500, 3000)},
                zero_tail=8)


def _fps_distinct_40():
    """40 distinct line points, m = 100: from pick 40 on every running minimum is exactly 0 and the pick is index 0."""
    ks = np.random.default_rng(42).permutation(65)[:40]
    return dict(X=R.line(_base(2), ks), m=100, first=11, zero_tail=60)


def _fps_lattice(seed, n, m, nnz, distinct):
    """Lattice rows drawn (with repeats) from `distinct` points: most pairs are orthogonal (d = 1/2 exactly), so nearly
    every argmax is a many-way exact tie spread over all lanes, waves and blocks."""
    rng = np.random.default_rng(seed)
    pts = R.lattice(rng, distinct, nnz)
    return dict(X=np.ascontiguousarray(pts[rng.integers(0, distinct, n)]), m=m, first=int(rng.integers(0, n)))


@functools.lru_cache(maxsize=None)
def fps_cases():
    return {
        "line_ties_4100": _fps_line_ties(),
        "line_distinct_40": _fps_distinct_40(),
        "lattice4_515": _fps_lattice(43, 515, 100, 4, 300),
        "lattice16_300": _fps_lattice(44, 300, 34, 16, 200),
        "lattice64_2049": _fps_lattice(45, 2049, 128, 64, 500),
        "lattice4_77": _fps_lattice(46, 77, 68, 4, 60),
    }


@functools.lru_cache(maxsize=None)
def fps_continuation_cases():
    """num_init in {1, 5, m}: the given rows are lattice points that are not rows of X."""
    out = {}
    for k in (1, 5, 20):
        rng = np.random.default_rng(50 + k)
        pts = R.lattice(rng, 260, 16)
        X = np.ascontiguousarray(pts[rng.integers(0, 200, 700)])          # rows among the first 200 points
        init = np.ascontiguousarray(pts[200 + rng.permutation(60)[:20]])  # given rows among the other 60
        out["given_%d_of_20" % k] = dict(X=X, m=20, init=init, num_init=k)
    return out


@functools.lru_cache(maxsize=None)
def fps_batch_case():
    rng = np.random.default_rng(60)
    pts = R.lattice(rng, 150, 4)
    X = np.stack([pts[rng.integers(0, 150, 515)] for _ in range(3)])
    X[1] = R.line(_base(3), rng.integers(0, 65, 515))
    return dict(X=np.ascontiguousarray(X), m=100, first=[3, 514, 200])


# ---- 3c. seed components ---------------------------------------------------------------------------------------------------
CC_M = [5, 63, 64, 65, 127, 128]


def cc_chain(m, trigger, kind):
    """The worked chain [p0, p2, p7, p5, p3] at eps = 2/64 spread over m seeds: p0 (index 0) and p7 (index 1) found components
    0 and 1 with p2 and p5; p3, the trigger, is within eps of p2 (label 0) and p5 (label 1): kind 'tied' has as many p2 as p5
    (tied mode: the smallest label wins, every p5 is overwritten), 'majority' more p5 (label 1 wins, every p2 is
    overwritten).  p2 sits at the last index, p5 at 63 | 64 where they exist, the trigger at index 2 ('low') or m - 2
    ('high'), so a ball spans both lane halves of the wave with the trigger on either side.  Everything else is far away
    (p20, p30, ... with duplicates)."""
    if m == 5:
        ks = {"low": [0, 7, 3, 5, 2], "high": [0, 7, 5, 3, 2]}[trigger]
        if kind == "majority":
            raise ValueError("five seeds hold one p2 and one p5")
        return R.line(_base(4), np.array(ks))
    ks = np.array([20, 30, 40, 50, 60])[np.arange(m) % 5]
    taken = {0: 0, 1: 7, m - 1: 2, (2 if trigger == "low" else m - 2): 3}
    p5 = [i for i in (63, 64) if i < m and i not in taken] or [m // 2]
    for i in p5:
        taken[i] = 5
    free = (i for i in range(3, m) if i not in taken)
    if kind == "tied":
        for _ in range(len(p5) - 1):
            taken[next(free)] = 2
    else:
        for _ in range(2):
            taken[next(free)] = 5
    for i, k in taken.items():
        ks[i] = k
    return R.line(_base(4), ks)


@functools.lru_cache(maxsize=None)
def cc_cases():
    """name -> (Z [m, 64], kind).  kind: 'worked' (the issue's literal case), 'tied', 'majority', 'same', 'apart'."""
    out = {"worked": (R.line(_base(4), np.array([0, 2, 7, 5, 3])), "worked")}
    for m in CC_M:
        for trigger in ("low", "high"):
            for kind in ("tied", "majority"):
                if m == 5 and kind == "majority":
                    continue
                out["chain_m%d_%s_%s" % (m, trigger, kind)] = (cc_chain(m, trigger, kind), kind)
    for m in (1, 64, 128):
        out["same_m%d" % m] = (np.repeat(R.line(_base(5), 9)[None], m, axis=0), "same")
    rng = np.random.default_rng(70)
    far = np.zeros((128, 64), np.float32)           # 16 disjoint supports x 8 sign patterns: every pair at d >= 1/4
    for i in range(128):
        s, pat = i % 16, i // 16
        far[i, 4 * s:4 * s + 4] = 0.5 * np.array([1, 1 - 2 * (pat & 1), 1 - 2 * ((pat >> 1) & 1), 1 - 2 * ((pat >> 2) & 1)])
    far = far[rng.permutation(128)]
    for m in (17, 128):
        out["apart_m%d" % m] = (np.ascontiguousarray(far[:m]), "apart")
    return out


# ---- 3d. assignment and the swap -----------------------------------------------------------------------------------------------
ASSIGN_M = [1, 9, 17, 20, 81, 89, 96, 100, 128] + [33, 57, 80]      # the second list: seed-tile counts 3, 4 and 5
ASSIGN_N = [1, 15, 17, 1025]
PAD_M = [1, 17, 20, 100]
# (seed index, line position): the seeds that take part in a tie; a pixel p(k) between two of them two flips apart is
# equidistant (1/64) from both.  3 | 4 and 0 | 15: one 16-seed tile (the DPP steps); 3 | 19 and 5 | 101: two tiles, one lane (the
# strict '<' over s); 15 | 16 and 2 | 127: two tiles, two lanes.
TIE_SEEDS = {19: 2, 3: 4, 4: 6, 0: 10, 15: 12, 16: 14, 5: 18, 101: 20, 2: 24, 127: 26}
TIE_PIXELS = {3: (3, 19), 5: (3, 4), 11: (0, 15), 13: (15, 16), 19: (5, 101), 25: (2, 127)}     # line position -> the tied seeds
LAST_SEED_PIXEL = 31            # between seed 7 (p30) and the LAST seed (p32), where that index is free
PLAIN_PIXELS = (40, 64, 30)     # far from every tie; exactly a filler's antipode; exactly seed 7


def assign_seeds(m):
    """Z [m, 64]: the tie seeds whose index exists, seed 7 = p30 and (where free) seed m - 1 = p32, fillers p(44..64)."""
    rng = np.random.default_rng(80 + m)
    ks = rng.integers(44, 65, m)
    for i, k in TIE_SEEDS.items():
        if i < m:
            ks[i] = k
    if m > 7:
        ks[7] = 30
        if m - 1 not in TIE_SEEDS and m - 1 != 7:
            ks[m - 1] = 32
    return R.line(_base(6), ks)


def assign_pixels(n):
    """Pixel p cycles through the 9 pixel kinds (9 is odd: every kind meets every slot p % 4 within 36 pixels)."""
    kinds = list(TIE_PIXELS) + [LAST_SEED_PIXEL] + list(PLAIN_PIXELS[:2])
    assert len(kinds) % 2 == 1
    return R.line(_base(6), np.array([kinds[p % len(kinds)] for p in range(n)]))


def assign_labels(m):
    """Seed labels over min(m, 5) ids, every id present, the ids in range(num_unique)."""
    k = min(m, 5)
    return ((np.arange(m) * 7 + 3) % k).astype(np.int32), k


def padding_case(m):
    """Pixels p(53..64) (p64 = -base), every seed within 20 flips of base: every real distance is above 1/2, the distance an
    unmasked zero padding row would have."""
    rng = np.random.default_rng(90 + m)
    Z = R.line(_base(7), rng.integers(0, 21, m))
    X = R.line(_base(7), np.concatenate([[64], rng.integers(53, 65, 40)]))
    return X, Z


@functools.lru_cache(maxsize=None)
def swap_cases():
    """name -> (X, Z, seed_labels, num_unique).  Four seeds p0, p16, p32, p48; `counts` pixels sit exactly on each."""
    def build(counts, sl, nu):
        ks = np.concatenate([np.full(c, 16 * i) for i, c in enumerate(counts)])
        ks = ks[np.random.default_rng(5).permutation(ks.size)]
        return R.line(_base(8), ks), R.line(_base(8), np.array([0, 16, 32, 48])), np.array(sl, np.int32), nu
    return {
        "equal_counts_first_wins": build([5, 5, 3, 1], [0, 1, 2, 3], 4),          # 0 and 1 tie: 0 wins, no swap
        "largest_is_2": build([2, 3, 9, 1], [0, 1, 2, 3], 4),                     # swap 0 <-> 2
        "tie_between_1_and_3": build([2, 6, 1, 6], [0, 1, 2, 3], 4),              # the first maximum, 1, wins
        "gap_largest_not_counted": build([3, 9, 0, 0], [0, 2, 0, 2], 2),          # labels {0, 2}: 2 is largest, not in range(2)
        "gap_counted_label_absent": build([1, 9, 0, 0], [2, 1, 2, 1], 2),         # labels {1, 2}: 1 counted, swaps with absent 0
        "shared_labels": build([4, 4, 4, 5], [1, 0, 0, 1], 2),                    # 9 : 8 for label 1
    }


# ---- 3e. the whole call ----------------------------------------------------------------------------------------------------
WHOLE = [(n, m, wide, batch) for n in (515, 4100) for m in (96, 100) for wide in (False, True) for batch in (1, 5)]


@functools.lru_cache(maxsize=None)
def whole_field(n, k, wide):
    """Field k of a whole-call case: line points, lattice points, or both mixed (all products stay dyadic), as [n, 64] or
    widened to [n, 128] (two planes)."""
    rng = np.random.default_rng(7000 + 10 * n + k)
    line_pts = R.line(_base(10 + k), rng.integers(0, 65, n))
    if k % 3 == 0:
        X = line_pts
    else:
        pts = R.lattice(rng, 90, 16 if k % 3 == 1 else 4)
        X = pts[rng.integers(0, 90, n)]
        if k % 3 == 2:
            X = np.where((np.arange(n) % 2 == 0)[:, None], X, line_pts)
    X = np.ascontiguousarray(X, np.float32)
    return R.widen(X, R.wide_positions(np.random.default_rng(3))) if wide else X


# ---- 3f. the pixel no seed wins ------------------------------------------------------------------------------------------------
NOSEED = [(33, 17, False), (17, 17, True)]      # n, m, 128-d: two seed tiles; one full pixel tile and (n = 33) a partial one


def noseed_rows(n):
    """The two non-finite rows: one in a full 16-pixel tile, the last one (n = 33: in the partial tile)."""
    return (5, n - 1)


@functools.lru_cache(maxsize=None)
def noseed_case(n, m, wide):
    """-> (X [n, 64 | 128] with rows noseed_rows(n) NaN, Z [m, 64 | 128], seed labels, num_unique = 2).  Seed s is the line
    point p(4 s), every finite pixel a p(k) with k odd: its two neighbouring seeds are 1/64 and 3/64 away, never a tie.  Every
    seed carries label 0 but the last, p(4 (m - 1)), which carries 1 and wins the pixels at k = 4 (m - 1) - 1 only (rows 0 and
    9): component 0 holds the majority and the swap does nothing."""
    assert 4 * (m - 1) <= 64 and n > 9
    rng = np.random.default_rng(95 + n)
    ks = 4 * rng.integers(0, m - 1, n) + rng.choice([1, 3], n)
    ks[[0, 9]] = 4 * (m - 1) - 1
    X = R.line(_base(9), ks)
    Z = R.line(_base(9), 4 * np.arange(m))
    if wide:
        pos = R.wide_positions(np.random.default_rng(3))
        X, Z = R.widen(X, pos), R.widen(Z, pos)
    X[list(noseed_rows(n))] = np.nan
    sl = np.zeros(m, np.int32)
    sl[m - 1] = 1
    return X, Z, sl, 2
