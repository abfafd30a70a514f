"""The inputs of the euclidean clustering stage tests, built once and shared by the CPU proof
(test_ms_euclidean_cases_host.py: every decision case is exact in fp32 in any order and hits the branch it was built for;
every climb case is sensitive to one pixel) and the GPU tests (test_ms_euclidean_stages_gpu.py).

Decision cases are made of tests/ms_cosine_reference.py's line and lattice points, whole or scaled row by row by 1, 1/2, 3/4
or 1/4: every coordinate is a multiple of 2^-5 below 1, so every product, square of a difference and partial sum is a short
dyadic number and ||x||^2 + ||z||^2 - 2 x.z and sum (x - z)^2 give the bits of float64 in any order.  What the scales are for:
with unit rows every norm is 1 and a norm taken from the wrong pixel slot, seed row, seed tile or 128-d half changes nothing.

The identities the engineered ties rest on (p(k) the line points, a and b scales):
    ||a p(j) - b p(k)||^2 = (a - b)^2 + a b |j - k| / 16
    so  ||p(j) - p(k)||^2 = |j - k| / 16,   ||p(k) - 0.75 p(k)||^2 = 1/16 = ||p(k) - p(k +- 1)||^2,
        ||p(k) - 0.5 p(k)|| = 1/2 = ||p(k) - p(k +- 4)|| = ||p(k) - 0.75 p(k +- 4)|| = ||0.5 p(k) - 0.5 p(k +- 16)||."""
from __future__ import annotations

import functools

import numpy as np

from tests import ms_cosine_cases as CS
from tests import ms_cosine_reference as G          # the generators
from tests import ms_euclidean_reference as R

KAPPA = CS.KAPPA
SCALES = np.array([1.0, 0.5, 0.75, 0.25], np.float32)
EPS_EXACT = 0.5                 # exactly a distance: ||p(j) - p(j + 4)||
EPS_BETWEEN = 0.53              # between ||p(j) - p(j + 4)|| = 0.5 and ||p(j) - p(j + 5)|| = 0.559
K_CLIMB = CS.K_CLIMB            # the project's K (tests/test_conv_tiles_gpu.py, profiles/ms_cosine_error.md)


def point_scale(P):
    """A scale of SCALES per row, a function of the row's content (its count of negative entries): equal rows keep equal
    scales, so duplicates stay exact ties."""
    return SCALES[(np.asarray(P) < 0).sum(axis=1) % 4]


def scaled(P, s=None):
    P = np.asarray(P, np.float32)
    s = point_scale(P) if s is None else np.asarray(s, np.float32)
    return np.ascontiguousarray(P * s[:, None])


# ---- 2. hill climbing ------------------------------------------------------------------------------------------------------
# m -> hc_iter_flat_kernel<ST, QUAD, EUC>: ST = ceil(m / 16), QUAD where ST >= 2 and the last tile holds 1..4 seeds
HC_TILE_M = CS.HC_TILE_M        # 1 | 16k + 2 (QUAD, ST 2..8) | 16k + 9 (not QUAD, ST 1..8) | 16k (full tiles, ST 1..8)
HC_TILE_ITERS = CS.HC_TILE_ITERS
HC_EDGE_M = CS.HC_EDGE_M
HC_EDGE_N = CS.HC_EDGE_N
HC_WIDE = CS.HC_WIDE
WIDE_FIRST = CS.WIDE_FIRST
WIDE_EPS = 0.2                  # the components of the 128-d whole calls; not compared (the climb is)
HC_OVERREAD_N = CS.HC_OVERREAD_N
HC_STRIDED = CS.HC_STRIDED
HC_AFFINE = CS.HC_AFFINE
HC_SCALED_M = [100, 89]         # QUAD | not QUAD (ST = 7 | 6)
HC_ROW_FACTORS = np.array([1.0, 0.5, 0.75, 1.25], np.float32)
HC_CLAMP = (1961, 20, 3, 11)    # n, m, the seed at the antipode of the field's mean, the seed at half a field row


def instantiation(m):
    """(ST, QUAD) as launch_hc picks them."""
    st = (m + 15) // 16
    return st, st >= 2 and 1 <= m - 16 * (st - 1) <= 4


hc_field = CS.hc_field
hc_seeds = CS.hc_seeds
hc_affine_field = CS.hc_affine_field
hc_mutations = CS.hc_mutations


def hc_affine_seeds(b):
    """Z0 of field b of the 256 x 2048 batch: draw 600 + b of hc_seeds.  Draws b and 300 + b put one of the 100 seeds of fields 1
    and 255 between two clusters, where ten iterations amplify every rounding error: that one seed lies 4 to 10 times farther
    from float64 than the other 99 in the tile-order fp32 evaluation (1.4e-6 against 1.5e-7), and the tolerance it sets is a
    ninth of what one pixel moves.  With this draw every seed of the five fields compared sits at 1e-7 ... 2e-7."""
    return hc_seeds(hc_affine_field(b), HC_AFFINE[2], 600 + b)[0]


@functools.lru_cache(maxsize=None)
def hc_scaled_case(m):
    """The n = 1961 field with every row scaled by a factor of HC_ROW_FACTORS, m of its rows as Z0 (rows of all four scales);
    seed 0 is the row nearest (euclidean) to the last pixel, so that pixel carries weight in it.  The last pixel is a row at
    1/2: there cluster mates are d^2 = 0.08 apart and weigh e^-1.6 each; at 1.25 they are 0.5 apart, weigh e^-10, and a seed
    would not see one of them dropped under any tolerance."""
    X = hc_field(1961)
    rng = np.random.default_rng(4000 + m)
    f = rng.integers(0, 4, X.shape[0])
    f[-1] = 1
    X = np.ascontiguousarray(X * HC_ROW_FACTORS[f][:, None])
    idx = rng.choice(X.shape[0] - 1, m, replace=False)
    near = int(np.argmin(((X[:-1].astype(np.float64) - X[-1].astype(np.float64)) ** 2).sum(axis=1)))
    if near in idx:
        idx[idx == near] = idx[0]
    idx[0] = near
    return X, np.ascontiguousarray(X[idx])


HC_WIDE_SCALED = (1961, 100)    # n, m of the 128-d field with rows of four norms


@functools.lru_cache(maxsize=None)
def hc_wide_scaled_field():
    """The 128-d n = 1961 field, every row scaled by a factor of HC_ROW_FACTORS (the last pixel by 1/2, as in hc_scaled_case).
    Its reason: an unmasked zero padding row of the last pixel tile (1961 = 122 x 16 + 9: seven of them) weighs e^(-20 ||z||^2),
    e^-20 against unit seeds, which moves the unit 128-d case by 5e-7, a fortieth of its tolerance, but e^-5 against a
    seed at 1/2 (||z||^2 = 1/4), which moves this one by 3.7e-3, 340 times its tolerance."""
    X = hc_field(HC_WIDE_SCALED[0], seed=7, channels=128)
    f = np.random.default_rng(4128).integers(0, 4, X.shape[0])
    f[-1] = 1
    return np.ascontiguousarray(X * HC_ROW_FACTORS[f][:, None])


@functools.lru_cache(maxsize=None)
def hc_clamp_case():
    """n = 1961, m = 20: seed HC_CLAMP[2] is the antipode of the field's mean direction (every weight below e^-60), seed
    HC_CLAMP[3] half a field row (every weight below e^-5): their weight sums are below 1 and the update divides by 1."""
    n, m, far, half = HC_CLAMP
    X = hc_field(n)
    Z0 = hc_seeds(X, m)[0].copy()
    mean = X.astype(np.float64).sum(axis=0)
    Z0[far] = (-mean / np.linalg.norm(mean)).astype(np.float32)
    Z0[half] = np.float32(0.5) * X[700]
    return X, Z0


TILE_ORDERS = 6                 # channel orders of the tile evaluation: the given one and five permutations


def climb_yardstick(X, Z0, kappa, iters):
    """(float64 result, three deviations from it):
      direct  the reference's code in torch float32, direct differences;
      tiles   the fp32 norm expansion summed in 16-pixel tiles, in TILE_ORDERS channel orders, the farthest of them;
      ulp     the float64 iteration with every squared distance one fp32 ulp of ||z||^2 + ||x||^2 up, and down.
    The last two model one property (profiles/ms_euclidean_error.md): the error of the norm expansion is no smooth function
    of the summation order.  Whether a pixel at the seed is seen at 0 or at one ulp of 2, and a weight sum next to 1 clamped
    or not, hangs on the last bit of three 64-term sums; where a few pixels carry a seed's whole weight (n <= 144) two orders
    differ by a factor of 10 to 20, and the kernel's order is one more draw."""
    ref = R.hill_climb(X, Z0, kappa, iters)
    X, Z0 = np.asarray(X, np.float32), np.asarray(Z0, np.float32)
    dev_d = float(np.abs(R.hill_climb_fp32_direct(X, Z0, kappa, iters) - ref).max())
    dev_t = 0.0
    for k in range(TILE_ORDERS):
        perm = np.arange(X.shape[1]) if k == 0 else np.random.default_rng(k).permutation(X.shape[1])
        til = R.hill_climb_fp32_tiles(X[:, perm], Z0[:, perm], kappa, iters)
        dev_t = max(dev_t, float(np.abs(til - ref[:, perm]).max()))
    dev_u = max(float(np.abs(R.hill_climb_ulp(X, Z0, kappa, iters, s) - ref).max()) for s in (-1.0, 1.0))
    return ref, (dev_d, dev_t, dev_u)


def climb_tolerance(devs):
    return K_CLIMB * max(devs)


STRIDED_SAMPLE = 13             # every 13th of the 300 fields (24 of them) sets the batch's yardstick


def strided_field(b):
    """(X, Z0) of field b of the 300 x 144 batch."""
    X = hc_field(HC_STRIDED[1], seed=100 + b)
    return X, hc_seeds(X, HC_STRIDED[2], b)[0]


@functools.lru_cache(maxsize=None)
def strided_yardstick():
    """The three deviations of the 300 x 144 batch: per yardstick the largest over the sampled fields.  Every field is a draw
    of one ensemble (same n, m and generator), and at n = 144 the deviation of one fp32 evaluation from float64 ranges over a
    factor of 30 from field to field and order to order (1e-7 ... 5e-6).  Measured on the CPU alone (profiles/
    ms_euclidean_error.md): a seventh channel order of the tile evaluation lies above K_CLIMB x the field's own yardstick in 2
    of 2100 (field, order) pairs, the worst at 4.4 x, so over 300 fields the reference's own arithmetic misses a per-field
    bound once in four runs.  Each field is still compared with its own float64 run."""
    devs = [climb_yardstick(*strided_field(b), KAPPA, 10)[1] for b in range(0, HC_STRIDED[0], STRIDED_SAMPLE)]
    return tuple(max(d[i] for d in devs) for i in range(3))


# ---- 3a. farthest-point sampling ------------------------------------------------------------------------------------------
def _base(seed=0):
    return G.line_base(np.random.default_rng(1900 + seed))


def _fps_line_ties_scaled():
    """n = 4100, first = 7 (p0).  Unit rows p0, p64, p32, p16, p48, p8, p24, p40, p56 at the engineered pixels, every other row
    a filler a p(k), k <= 7, a in {1/2, 3/4, 1/4} (hundreds of duplicates per point).  The fillers at 1/2 and 3/4 lie within
    d^2 < 1/2 of p0, those at 1/4 between 9/16 and 11/16 of p0 and at least 9/16 from every unit row, so the unit rows are
    picked as on the unit line: p64 (100 | 2148: two blocks of both kernels), p32 (5 | 13: one 16-lane row group), p16 | p48 (70 |
    130: two waves), then, after fillers at 1/4, the four-way tie p8, p24, p40, p56 at d^2 = 1/2 (300 | 812 | 1500 | 3000: two pixel
    slots of one lane of the on-chip kernel, four blocks of the streaming one).  All 33 distinct points chosen, every running
    minimum is 0 and the pick is index 0."""
    rng = np.random.default_rng(141)
    ks = rng.integers(0, 8, 4100)
    sc = np.array([0.5, 0.75, 0.25], np.float32)[rng.integers(0, 3, 4100)]
    for i, k in {7: 0, 100: 64, 2148: 64, 5: 32, 13: 32, 70: 16, 130: 48, 300: 8, 812: 24, 1500: 40, 3000: 56}.items():
        ks[i], sc[i] = k, 1.0
    return dict(X=scaled(G.line(_base(1), ks), sc), m=40, first=7, groups=[(100, 2148), (5, 13), (70, 130), (300, 812, 1500, 3000)],
                zero_tail=7, scaled=True)


def _fps_lattice_scaled(seed, n, m, nnz, distinct):
    rng = np.random.default_rng(seed)
    pts = scaled(G.lattice(rng, distinct, nnz), SCALES[np.arange(distinct) % 4])
    return dict(X=np.ascontiguousarray(pts[rng.integers(0, distinct, n)]), m=m, first=int(rng.integers(0, n)), scaled=True, groups=[])


@functools.lru_cache(maxsize=None)
def fps_cases():
    """The cosine cases as they are (unit rows: d = 2 sqrt(cosine distance), the same picks, the engineered tie placements
    kept), and scaled ones."""
    out = {}
    for name, c in CS.fps_cases().items():
        out["unit_" + name] = dict(c, scaled=False, groups=list(c.get("ties", {}).values()))
    out["scaled_line_ties_4100"] = _fps_line_ties_scaled()
    out["scaled_lattice4_515"] = _fps_lattice_scaled(143, 515, 100, 4, 300)
    out["scaled_lattice16_300"] = _fps_lattice_scaled(144, 300, 34, 16, 200)
    out["scaled_lattice64_2049"] = _fps_lattice_scaled(145, 2049, 128, 64, 500)
    return out


@functools.lru_cache(maxsize=None)
def fps_continuation_cases():
    """num_init in {1, 5, m}: the given rows are scaled lattice points that are not rows of X."""
    out = {}
    for k in (1, 5, 20):
        rng = np.random.default_rng(150 + k)
        pts = scaled(G.lattice(rng, 260, 16), SCALES[np.arange(260) % 4])
        X = np.ascontiguousarray(pts[rng.integers(0, 200, 700)])
        init = np.ascontiguousarray(pts[200 + rng.permutation(60)[:20]])
        out["given_%d_of_20" % k] = dict(X=X, m=20, init=init, num_init=k)
    return out


@functools.lru_cache(maxsize=None)
def fps_batch_case():
    rng = np.random.default_rng(160)
    pts = scaled(G.lattice(rng, 150, 4), SCALES[np.arange(150) % 4])
    X = np.stack([pts[rng.integers(0, 150, 515)] for _ in range(3)])
    ks = rng.integers(0, 65, 515)
    X[1] = scaled(G.line(_base(3), ks), SCALES[ks % 4])
    return dict(X=np.ascontiguousarray(X), m=100, first=[3, 514, 200])


# ---- 3b. seed components ---------------------------------------------------------------------------------------------------------
CC_M = CS.CC_M
# the cosine chain's line positions -> positions twice as far apart: two flips (the cosine eps) become four (||.|| = 1/2)
_CC_MAP = {0: 0, 2: 4, 7: 14, 5: 10, 3: 6, 20: 28, 30: 36, 40: 44, 50: 52, 60: 60}


def cc_chain(m, trigger, kind):
    """The cosine chain (tests/ms_cosine_cases.py: cc_chain) at eps = 1/2: [p0, p4, p14, p10, p6] spread over m seeds.  p0 and
    p14 found components 0 and 1 with p4 and p10 (each exactly at eps); p6, the trigger, is within eps of p4 and exactly at eps
    of p10.  Everything else is at least sqrt(1/2) away."""
    Z = CS.cc_chain(m, trigger, kind)
    ks = (Z * CS._base(4)[None, :] < 0).sum(axis=1)
    return G.line(_base(4), np.array([_CC_MAP[int(k)] for k in ks]))


def cc_chain_scaled(m, trigger, kind):
    """A chain whose members have different norms.  Seed 0 = p0 founds component 0 with 0.5 p0 (exactly at eps; the last
    index); seed 1 = p20 founds component 1 with 0.75 p24 (exactly at eps; indices 63 | 64 where they exist, else m // 2); the
    trigger 0.5 p16 (index 2 'low' | m - 2 'high') is exactly at eps of 0.5 p0 and of 0.75 p24 and farther from p0 and p20.
    'tied': as many 0.5 p0 as 0.75 p24 (the smallest label wins, every 0.75 p24 is overwritten); 'majority': two more 0.75 p24
    (label 1 wins, every 0.5 p0 is overwritten).  The rest: unit p36, p44, p52, p60 with duplicates, far from everything."""
    P0, P20, TRIG, L0, L1 = (0, 1.0), (20, 1.0), (16, 0.5), (0, 0.5), (24, 0.75)
    if m == 5:
        if kind == "majority":
            raise ValueError("five seeds hold one of each")
        pts = {"low": [P0, P20, TRIG, L1, L0], "high": [P0, P20, L1, TRIG, L0]}[trigger]
    else:
        pts = [((36, 44, 52, 60)[i % 4], 1.0) for i in range(m)]
        taken = {0: P0, 1: P20, m - 1: L0, (2 if trigger == "low" else m - 2): TRIG}
        l1 = [i for i in (63, 64) if i < m and i not in taken] or [m // 2]
        for i in l1:
            taken[i] = L1
        free = (i for i in range(3, m) if i not in taken)
        for _ in range(len(l1) - 1 if kind == "tied" else 2):
            taken[next(free)] = L0 if kind == "tied" else L1
        for i, p in taken.items():
            pts[i] = p
    return scaled(G.line(_base(4), np.array([k for k, _ in pts])), [a for _, a in pts])


@functools.lru_cache(maxsize=None)
def cc_cases():
    """name -> (Z [m, 64], kind).  kind: 'tied', 'majority' (unit chains), 'scaled_tied', 'scaled_majority', 'same', 'apart'."""
    out = {}
    for m in CC_M:
        for trigger in ("low", "high"):
            for kind in ("tied", "majority"):
                if m == 5 and kind == "majority":
                    continue
                out["chain_m%d_%s_%s" % (m, trigger, kind)] = (cc_chain(m, trigger, kind), kind)
                out["scaled_chain_m%d_%s_%s" % (m, trigger, kind)] = (cc_chain_scaled(m, trigger, kind), "scaled_" + kind)
    for m in (1, 64, 128):
        out["same_m%d" % m] = (np.repeat((np.float32(0.75) * G.line(_base(5), 9))[None], m, axis=0), "same")
    for m in (17, 128):
        out["apart_m%d" % m] = (CS.cc_cases()["apart_m%d" % m][0], "apart")       # every pair at least 1 apart
    return out


# ---- 3c. assignment and the swap ---------------------------------------------------------------------------------------------
ASSIGN_M = CS.ASSIGN_M          # every seed-tile count 1..8: assign_kernel<ST, 1, EUC>
ASSIGN_N = CS.ASSIGN_N
PAD_M = CS.PAD_M
TIE_PIXELS = CS.TIE_PIXELS
LAST_SEED_PIXEL = CS.LAST_SEED_PIXEL
assign_pixels = CS.assign_pixels
assign_labels = CS.assign_labels
swap_cases = CS.swap_cases
SCALED_TIE_SEED = {3: 19, 5: 4, 11: 0, 13: 16, 19: 101, 25: 127}     # pixel position -> the seed of its pair that is scaled


def assign_seeds(m, scale):
    """Z [m, 64].  Unit: the cosine case's seeds (a pixel p(k) between the seeds p(k - 1) and p(k + 1) is 1/4 from both).
    Scaled: one seed of every tie pair (SCALED_TIE_SEED: one that belongs to no other pair) becomes 0.75 p(k), k the pixel's
    position: still exactly 1/4 from the pixel, with another norm than its rival p(k -+ 1); the fillers take scales of SCALES."""
    Z = CS.assign_seeds(m).copy()
    if not scale:
        return Z
    rng = np.random.default_rng(180 + m)
    fill = np.ones(m, bool)
    fill[[i for i in list(CS.TIE_SEEDS) + [7, m - 1] if i < m]] = False
    Z[fill] *= SCALES[rng.integers(0, 4, int(fill.sum()))][:, None]
    for k, (a, b) in tie_pairs(m).items():
        Z[SCALED_TIE_SEED.get(k, m - 1)] = np.float32(0.75) * G.line(CS._base(6), k)
    return np.ascontiguousarray(Z)


def last_seed_is_free(m):
    return m > 7 and m - 1 not in CS.TIE_SEEDS and m - 1 != 7


def tie_pairs(m):
    """line position of the pixel -> the two seeds it is equidistant from, for the pairs that exist with m seeds."""
    pairs = {k: v for k, v in TIE_PIXELS.items() if max(v) < m}
    if last_seed_is_free(m):
        pairs[LAST_SEED_PIXEL] = (7, m - 1)
    return pairs


def padding_case(m):
    """The cosine case's seeds (within 20 flips of base) and pixels (p(53) .. p(64)), the pixels scaled by SCALES: every real
    squared distance is (1 - a)^2 + a |j - k| / 16 with |j - k| >= 33, above a^2 = the squared distance ||x||^2 of an unmasked
    zero padding row of the last seed tile."""
    X, Z = CS.padding_case(m)
    return scaled(X, SCALES[np.arange(X.shape[0]) % 4]), Z


# ---- 3d. the whole call ----------------------------------------------------------------------------------------------------
WHOLE = CS.WHOLE
WHOLE_EPS = EPS_EXACT


@functools.lru_cache(maxsize=None)
def whole_field(n, k, wide):
    """Field k of a whole-call case: the cosine case's field, every row scaled by point_scale (equal rows stay equal), as
    [n, 64] or widened to [n, 128]: the two halves then carry different parts of every norm."""
    X = scaled(CS.whole_field(n, k, False))
    return G.widen(X, G.wide_positions(np.random.default_rng(3))) if wide else X


# ---- 3e. the pixel no seed wins ------------------------------------------------------------------------------------------------
NOSEED_N = [33, 17]             # 17 seeds (two seed tiles); n = 33: a NaN row in a full pixel tile and one in the partial tile
noseed_rows = CS.noseed_rows


@functools.lru_cache(maxsize=None)
def noseed_case(n):
    """-> (X [n, 64] with rows noseed_rows(n) NaN, Z [17, 64], seed labels, num_unique = 2).  Seed s is p(4 s) with label s % 2;
    every finite pixel is p(4 s - 1) (p(1) for s = 0): 1/4 from seed s and sqrt(3)/4 from the next, never a tie.  Of the n - 2
    finite pixels (n - 2) // 2 + 1 go to seeds of label 1 and (n - 2) // 2 to seeds of label 0: label 0 is the largest only with
    the two NaN rows counted under it, and then the swap does nothing."""
    m = 17
    rng = np.random.default_rng(195 + n)
    bad = list(noseed_rows(n))
    fin = np.setdiff1d(np.arange(n), bad)
    want = np.zeros(n, np.int64)
    want[fin[:(n - 2) // 2 + 1]] = 1
    want[fin] = want[fin][rng.permutation(fin.size)]
    s = 2 * rng.integers(0, 8, n) + want                 # a seed of the wanted label (parity), 0..16
    ks = np.where(s == 0, 1, 4 * s - 1)
    X = G.line(_base(9), ks)
    Z = G.line(_base(9), 4 * np.arange(m))
    X[bad] = np.nan
    return X, Z, (np.arange(m) % 2).astype(np.int32), 2
