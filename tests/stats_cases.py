"""Engineered inputs, exact expectations and a gap-independent checker for the kernels that share csrc/fixed_order.h:
uoc_objects (objects.hip) and steps C and D of uoc_support_plane / uoc_support_planes (plane.hip).

Tier 1 (exact in every summation order).  Points lie on a dyadic lattice (multiples of 2^-10 m, |x| <= 32, at most 2^14
points; the two `fine_pair` cases use the float32 grid itself, 2^-19 m at 16 m) and are symmetric about a dyadic centre.
Every sum, the mean, every centred difference and every product is then exact in fp64 whatever the order; the one
rounding is M / n, followed by the cast to float32.  `expected_object` evaluates that with Python integers and
fractions.Fraction, rounds once to float64 and then to float32, as the kernel does, so every float field is compared with
np.array_equal and nothing is exempt.

Tier 2 (separated from a rounding boundary).  Where 1/sqrt 2 enters (the axes and the extents of the 45-degree cases,
the tilted plane), the expected float32 is the value to 60 decimal digits rounded once, and a case is admitted only when
that value lies at least 2^-40 (relative) from a float32 rounding boundary (TIER2_SEPARATION, asserted by
tests/test_stats_cases_host.py): any fp64 evaluation, whose error is a few 2^-53, lands on the same float.  The
eigenvalues of the 45-degree cases are chosen exactly representable in float32, which is the same argument with the
widest possible separation.

The checker (`object_metrics`, `plane_metrics`, `plane_object_metrics`, `height_metrics`, and `plane_reference_metrics`
for the sums of steps C and D against the reference itself) judges a record by properties that hold whatever the
eigen-gaps are; every bound is derived in the docstring of the function that computes it, from n, the magnitudes and
the float32 / fp64 roundings.  A metric is (name, value, bound); a record passes when every value <= bound.

`model_object` and `model_plane_object` restate the kernels' arithmetic on the CPU (fp64 sums, the cyclic Jacobi of
fixed_order.h, the stable 3-sort, the sign rule, the closed-form 2x2) with switches for the mutants
tests/test_stats_cases_host.py must see rejected."""
import functools
import itertools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

LATTICE_EXP = 10                                   # tier-1 coordinates are multiples of 2^-10 m
BASE_CENTRE = (0, 0, 1 << LATTICE_EXP)             # (0, 0, 1) m in lattice units
OFFSET = (-8 * 1024 + 3, 2 * 1024, 16 * 1024)      # (-8 + 3/1024, 2, 16) m: the large dyadic translation
TIER2_SEPARATION = 2.0 ** -40
U24, U25, U53 = 2.0 ** -24, 2.0 ** -25, 2.0 ** -53
SQ3 = math.sqrt(3.0)
FP64_SLACK = 2.0 ** -40        # relative room for the fp64 solver and sums: at most 48 rotations, each a few 2^-53


# ---- the cases ----------------------------------------------------------------------------------------------------------
def grid(counts, half_steps):
    """Integer points of a box grid symmetric about 0: coordinate hs * (2 i - (n - 1)), i < n, per axis."""
    ax = [hs * (2 * np.arange(n) - (n - 1)) for n, hs in zip(counts, half_steps)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)


def diag45(pair, p, q, h):
    """Eight points symmetric under the swap of the two axes of `pair`: +-(p, p) and +-(q, -q) in the pair's plane, each
    at +-h along the third axis.  var = (p^2 + q^2) / 2 on both axes, cov = (p^2 - q^2) / 2: eigenvalues p^2, q^2, h^2."""
    a, b = pair
    t = 3 - a - b
    out = []
    for sa, sb in ((p, p), (-p, -p), (q, -q), (-q, q)):
        for st in (h, -h):
            v = [0, 0, 0]
            v[a], v[b], v[t] = sa, sb, st
            out.append(v)
    return np.array(out, np.int64)


def object_cases():
    """name -> dict(rel [n,3] int64 offsets from the centre, centre (3 ints), exp: coordinates are integers * 2^-exp m,
    translate: whether the case is also run at OFFSET)."""
    C = {}

    def add(name, rel, centre=BASE_CENTRE, exp=LATTICE_EXP, translate=True):
        C[name] = dict(rel=np.asarray(rel, np.int64).reshape(-1, 3), centre=tuple(centre), exp=exp, translate=translate)

    # diagonal covariance, three distinct variances, all six axis orders
    for perm in itertools.permutations(range(3)):
        counts = [0, 0, 0]
        for rank, ax in enumerate(perm):
            counts[ax] = (9, 5, 3)[rank]
        add("brick_%d%d%d" % perm, grid(counts, (4, 4, 4)))
    # ties
    add("cube", grid((3, 3, 3), (4, 4, 4)))
    add("plate_xy", grid((4, 4, 2), (4, 4, 4)))        # variances (2, 2, 1): order [0, 1, 2]
    add("plate_yz", grid((2, 4, 4), (4, 4, 4)))        # (1, 2, 2): [1, 2, 0]
    add("plate_xz", grid((4, 2, 4), (4, 4, 4)))        # (2, 1, 2): [0, 2, 1], e2 = -y
    add("rod_x", grid((4, 2, 2), (4, 4, 4)))           # (2, 1, 1): [0, 1, 2]
    add("rod_y", grid((2, 4, 2), (4, 4, 4)))           # (1, 2, 1): [1, 0, 2], e2 = -z
    add("rod_z", grid((2, 2, 4), (4, 4, 4)))           # (1, 1, 2): [2, 0, 1]
    # rank-deficient sets
    for k, ax in enumerate("xyz"):
        counts2, counts5 = [1, 1, 1], [1, 1, 1]
        counts2[k], counts5[k] = 2, 5
        add("two_" + ax, grid(counts2, (8, 8, 8)))
        add("line5_" + ax, grid(counts5, (4, 4, 4)))
    add("patch_xy", grid((7, 4, 1), (4, 4, 4)))
    add("patch_yz", grid((1, 7, 4), (4, 4, 4)))
    add("patch_xz", grid((4, 1, 7), (4, 4, 4)))
    add("coincident", np.zeros((5, 3)))
    add("single", np.zeros((1, 3)))
    # the 45-degree tie: theta == 0, c == s in bits
    add("d45_xy_pos_tall", diag45((0, 1), 24, 8, 16))  # third axis second: e1 = z, e2 = (f, -f, 0)
    for pair, nm in (((0, 1), "xy"), ((0, 2), "xz"), ((1, 2), "yz")):
        add("d45_%s_pos" % nm, diag45(pair, 24, 16, 8))
        add("d45_%s_neg" % nm, diag45(pair, 16, 24, 8))
    # rank-deficient 45-degree sets.  The variance is a power of two and every coordinate a power of two (or 0), so that
    # c * a, s * a and c * dx are exact and the null eigenvalue and the null extent are exact zeros with or without fused
    # multiply-adds.
    add("diagline2_xy", [[16, 16, 0], [-16, -16, 0]])
    add("diagline5_xy", [[8 * i, 8 * i, 0] for i in range(-2, 3)])
    add("tilted_patch_pos", [[8 * i, j, 8 * i] for i in range(-2, 3) for j in (-6, 0, 6)])
    add("tilted_patch_neg", [[8 * i, j, -8 * i] for i in range(-2, 3) for j in (-6, 0, 6)])
    # the float32 grid itself: the centroid 16 + 2^-20 is no float32, so a float32 centroid doubles the variance
    add("fine_pair_x", [[1, 0, 0], [-1, 0, 0]], centre=((16 << 20) + 1, 2 << 20, 1 << 20), exp=20, translate=False)
    add("fine_pair_z", [[0, 0, 1], [0, 0, -1]], centre=(1 << 20, 2 << 20, (16 << 20) + 1), exp=20, translate=False)
    # large enough that a float32 accumulator loses bits (4096 points at 17 m: 27 bits).  The centre is odd in no coordinate
    # pattern: about an odd x every addend is a tie of the running sum's spacing, and round-to-even cancels the errors.
    add("big_brick", grid((32, 16, 8), (1, 1, 1)), centre=(5, -3, (1 << LATTICE_EXP) + 1))
    return C


def case_points(case, translated=False):
    """[n,3] float32 coordinates in metres (exact) and the centre as integers in the case's unit."""
    centre = np.array(case["centre"], np.int64)
    if translated:
        assert case["translate"] and case["exp"] == LATTICE_EXP
        centre = centre + np.array(OFFSET, np.int64)
    q = case["rel"] + centre
    p = (q.astype(np.float64) * 2.0 ** -case["exp"]).astype(np.float32)
    assert np.array_equal(p.astype(np.float64) * 2.0 ** case["exp"], q), "coordinates are not exact float32"
    return p, centre


# ---- tier 2: one rounding of a high-precision value -------------------------------------------------------------------------
def f32_round_checked(num, over_sqrt2):
    """(float32 nearest to num [/ sqrt 2], relative distance of that value from the nearest float32 rounding boundary;
    inf where the value is exactly representable).  num is a Fraction."""
    getcontext().prec = 60
    val = Decimal(num.numerator) / Decimal(num.denominator)
    if over_sqrt2:
        val = val / Decimal(2).sqrt()
    f = np.float32(float(val))
    if val == 0 or Decimal(float(f)) == val:
        return f, math.inf
    up = Decimal(float(np.nextafter(f, np.float32(np.inf))))
    dn = Decimal(float(np.nextafter(f, np.float32(-np.inf))))
    fd = Decimal(float(f))
    sep = min(abs(val - (fd + up) / 2), abs(val - (fd + dn) / 2)) / abs(val)
    return f, float(sep)


def f32_exact(num):
    """float32 of a Fraction rounded once to float64 and then to float32, as `(float)double` does."""
    return np.float32(float(num))


# ---- the exact reference ------------------------------------------------------------------------------------------------------
def eigen_structure(rel):
    """The diagonalised form the kernel's Jacobi reaches, in its index order: three (eigenvalue as a Fraction in unit^2,
    integer vector w; the eigenvector is w / |w|), and the rotated pair (p, q) or None.  Admits a diagonal moment matrix,
    or one non-zero off-diagonal (p, q) with equal diagonal entries p, q: the 45-degree tie."""
    n = len(rel)
    M = [[int(v) for v in row] for row in (rel.T @ rel)]
    off = [(i, j) for i in range(3) for j in range(i + 1, 3) if M[i][j] != 0]
    unit = [tuple(int(i == k) for i in range(3)) for k in range(3)]
    if not off:
        return [(Fraction(M[k][k], n), unit[k]) for k in range(3)], None
    assert len(off) == 1, "more than one correlated pair"
    p, q = off[0]
    assert M[p][p] == M[q][q], "not symmetric under the swap of the pair"
    out = [None, None, None]
    t = 3 - p - q
    out[p] = (Fraction(M[p][p] - M[p][q], n), tuple(unit[p][i] - unit[q][i] for i in range(3)))    # column (c, -s)
    out[q] = (Fraction(M[p][p] + M[p][q], n), tuple(unit[p][i] + unit[q][i] for i in range(3)))    # column (s, c)
    out[t] = (Fraction(M[t][t], n), unit[t])
    return out, (p, q)


def expected_object(case, translated=False):
    """Every float field of uoc_object for one case as float32, with `order` (the axis order after the stable
    descending sort), `tier2` (name -> separation of every value that is the rounding of an irrational) and `count`."""
    rel, exp = case["rel"], case["exp"]
    p32, centre = case_points(case, translated)
    n = len(rel)
    assert n <= 1 << 14 and np.abs(rel + centre).max() <= 32 << exp
    assert not np.any(rel.sum(axis=0)), "not symmetric about its centre"
    ulen = Fraction(1, 1 << exp)
    M = rel.T @ rel
    cov = np.array([f32_exact(Fraction(int(M[i, j]), n) * ulen * ulen) for i, j in
                    ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], np.float32)
    eig3, pair = eigen_structure(rel)
    order = sorted(range(3), key=lambda k: -eig3[k][0])          # stable: ties keep the lower index first
    tier2 = {}
    eig = np.zeros(3, np.float32)
    for k, o in enumerate(order):
        eig[k] = f32_exact(eig3[o][0] * ulen * ulen)
        if pair is not None:
            assert Fraction(float(eig[k])) == eig3[o][0] * ulen * ulen, "45-degree eigenvalue is no float32"
    w = [np.array(eig3[order[0]][1], np.int64), np.array(eig3[order[1]][1], np.int64)]
    w.append(np.cross(w[0], w[1]))
    norm2 = [int(w[0] @ w[0]), int(w[1] @ w[1])]
    norm2.append(norm2[0] * norm2[1])                           # |e0 x e1| = |e0| |e1|: the two are orthogonal
    axes = np.zeros((3, 3), np.float32)
    half = np.zeros(3, np.float32)
    for k in range(3):
        s2 = norm2[k]                                           # 1, 2 or 4: the axis is w / sqrt(s2)
        assert s2 in (1, 2, 4) and int(w[k] @ w[k]) == s2
        for i in range(3):
            num = Fraction(int(w[k][i]), 2 if s2 == 4 else 1)
            axes[i, k], sep = f32_round_checked(num, s2 == 2)
            tier2["axes[%d,%d]" % (i, k)] = sep
        d = rel @ w[k]
        hi, lo = int(d.max()), int(d.min())
        assert hi == -lo, "extent not symmetric about the centroid"
        half[k], sep = f32_round_checked(Fraction(hi, 2 if s2 == 4 else 1) * ulen, s2 == 2)
        tier2["obb_half[%d]" % k] = sep
    c32 = np.array([f32_exact(Fraction(int(v)) * ulen) for v in centre], np.float32)
    return dict(count=n, centroid=c32, cov=cov, aabb_min=p32.min(axis=0), aabb_max=p32.max(axis=0), eig=eig, axes=axes,
                obb_half=half, obb_center=c32.copy(), order=order, tier2=tier2, pair=pair)


FLOAT_FIELDS = ("centroid", "cov", "aabb_min", "aabb_max", "eig", "axes", "obb_half", "obb_center")
SHAPE_FIELDS = ("cov", "eig", "axes", "obb_half")          # unchanged by a translation


def cov6(c):
    """The six upper-triangle entries (xx, xy, xz, yy, yz, zz) of a covariance given as those six or as a 3x3 matrix."""
    c = np.asarray(c)
    return c.reshape(3, 3)[np.triu_indices(3)] if c.size == 9 else c.reshape(6)


def assert_object_exact(got, want, where):
    """np.array_equal on every float field and the count: no field and no case is exempt."""
    assert int(got["count"]) == want["count"], (where, "count", int(got["count"]), want["count"])
    for k in FLOAT_FIELDS:
        g = np.asarray(cov6(got[k]) if k == "cov" else got[k], np.float32).reshape(np.shape(want[k]))
        assert np.array_equal(g, want[k]), (where, k, g.tolist(), want[k].tolist())


# ---- the kernel's arithmetic on the CPU, with mutants ---------------------------------------------------------------------------
def jacobi3(a):
    """fixed_order.h's jacobi3 in Python floats (fp64, no fused multiply-add): (diagonalised a, v)."""
    a = [[float(x) for x in row] for row in a]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(16):
        off = abs(a[0][1]) + abs(a[0][2]) + abs(a[1][2])
        dia = abs(a[0][0]) + abs(a[1][1]) + abs(a[2][2])
        if off <= 1e-18 * dia or off == 0.0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = a[k][p], a[k][q]
                a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(3):
                apk, aqk = a[p][k], a[q][k]
                a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
            a[p][q] = a[q][p] = 0.0
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return a, v


def sort_eig3(a, v, ascending=False, unstable=False):
    lam = [a[i][i] for i in range(3)]
    vec = [[v[k][i] for k in range(3)] for i in range(3)]

    def swap_if(i, j):
        move = lam[j] < lam[i] if ascending else (lam[j] >= lam[i] if unstable else lam[j] > lam[i])
        if move:
            lam[i], lam[j] = lam[j], lam[i]
            vec[i], vec[j] = vec[j], vec[i]
    swap_if(1, 2)
    swap_if(0, 1)
    swap_if(1, 2)
    return lam, vec


def sign_rule(e):
    k = 0
    for i in (1, 2):
        if abs(e[i]) > abs(e[k]):
            k = i
    return [-x for x in e] if e[k] < 0.0 else list(e)


MUTANTS = ("drop_point", "point_twice", "float32_sums", "float32_centroid", "single_pass_float32", "e1_negated",
           "no_sign_rule", "e2_flipped", "ascending", "unstable_sort", "extents_about_origin", "min_max_swapped")


def model_object(p32, mutant=None, order=None):
    """uoc_object's float fields for the valid points p32 [n,3] float32, computed as objects.hip does (fp64 sums in the
    given point order, moments about the fp64 centroid, jacobi3, the stable sort, the sign rule, e2 = e0 x e1, extents
    of (p - c) . e_k in fp64, the eigenvalues clamped at 0), every field cast once to float32.  `mutant` is None or one
    of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    p32 = np.asarray(p32, np.float32)
    aabb = p32.min(axis=0), p32.max(axis=0)
    if order is not None:
        p32 = p32[order]
    if mutant == "drop_point":
        p32 = p32[:-1] if len(p32) > 1 else p32
    if mutant == "point_twice":
        p32 = np.concatenate([p32, p32[-1:]])
    n = len(p32)
    p = p32.astype(np.float64)
    if mutant == "float32_sums":
        s = np.zeros(3, np.float32)
        for row in p32:
            s = s + row
        c = s.astype(np.float64) / n
    else:
        c = p.sum(axis=0) / n
    cc = c.astype(np.float32).astype(np.float64) if mutant == "float32_centroid" else c
    d = p - cc
    if mutant == "single_pass_float32":
        s2 = np.zeros((3, 3), np.float32)
        for row in p32:
            s2 = s2 + np.outer(row, row)
        c32 = c.astype(np.float32)
        cov = ((s2 / np.float32(n)) - np.outer(c32, c32)).astype(np.float64)
    elif mutant == "float32_sums":
        s2 = np.zeros((3, 3), np.float32)
        for row in d.astype(np.float32):
            s2 = s2 + np.outer(row, row)
        cov = s2.astype(np.float64) / n
    else:
        cov = np.einsum("ni,nj->ij", d, d) / n
    a, v = jacobi3(cov)
    lam, vec = sort_eig3(a, v, ascending=mutant == "ascending", unstable=mutant == "unstable_sort")
    e0, e1 = (vec[0], vec[1]) if mutant == "no_sign_rule" else (sign_rule(vec[0]), sign_rule(vec[1]))
    if mutant == "e1_negated":
        e1 = [-x for x in e1]
    e0, e1 = np.array(e0), np.array(e1)
    e2 = np.cross(e1, e0) if mutant == "e2_flipped" else np.cross(e0, e1)
    A = np.stack([e0, e1, e2], axis=1)
    proj = (p if mutant == "extents_about_origin" else p - c) @ A
    hi, lo = proj.max(axis=0), proj.min(axis=0)
    if mutant == "min_max_swapped":
        hi, lo = lo, hi
    f = np.float32
    return dict(count=n, centroid=c.astype(f), cov=cov[np.triu_indices(3)].astype(f), aabb_min=aabb[0], aabb_max=aabb[1],
                eig=np.maximum(np.array(lam), 0.0).astype(f), axes=A.astype(f), obb_half=(0.5 * (hi - lo)).astype(f),
                obb_center=(c + A @ (0.5 * (hi + lo))).astype(f))


# ---- the gap-independent checker -------------------------------------------------------------------------------------------------
def half_ulp(x):
    """Half the spacing of float32 at x (elementwise, float64): the most a single rounding to float32 moves a value
    whose nearest float32 is x."""
    return 0.5 * np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def ortho_bound():
    """Bound on |A^T A - I| for the float32 image of an orthonormal fp64 triple.  Each component moves by at most 2^-25
    (half a float32 ulp below 1), so entry (j, k) moves by at most 2^-25 (|a_j|_1 + |a_k|_1) <= 2 sqrt 3 * 2^-25, about
    1.7 half-ulps of 1; the products of two errors (3 * 2^-50) and the fp64 triple's own defect fit in FP64_SLACK."""
    return 2.0 * SQ3 * U25 + FP64_SLACK


def residual_bound(l0):
    """Bound on |C a - lam a|_inf for a stored float32 eigenpair (a, lam) of the fp64 covariance C with largest
    eigenvalue l0.  The fp64 pair (a', lam') has a residual of the solver's own size, FP64_SLACK * l0 (the sweeps end at
    off <= 1e-18 * dia; the kernel's C differs from the reference's by the accumulation error, far below that).
    Rounding moves each component of a by at most 2^-25 and lam by at most 2^-24 lam <= 2^-24 l0, and
    |C - lam I|_inf <= |C|_inf + lam <= (sqrt 3 + 1) l0 (a row sum is at most sqrt 3 times the 2-norm), so the residual
    grows by at most (sqrt 3 + 1) l0 2^-25 + 2^-24 l0 |a|_inf <= 2.37 * 2^-24 l0.  2^-149 covers a subnormal store."""
    return ((SQ3 + 1.0) / 2.0 + 1.0) * U24 * l0 + FP64_SLACK * l0 + 2.0 ** -149


def sum_gamma(n, mean_abs):
    """fp64 accumulation bound for a mean of n terms: each of the n - 1 additions and the division round by at most
    2^-53 of the running magnitude, which the sum of |term| bounds, so the mean is within n * 2^-53 * mean|term| in any
    order.  The kernel and the reference each get one such error: callers use 2 * sum_gamma."""
    return n * U53 * mean_abs


def _metric(out, name, value, bound):
    out.append((name, float(value), float(bound)))


def _sign_rule_metric(out, name, e):
    """The component of largest magnitude is positive.  Judged on the stored float32 vector where it is decided there:
    when every component within 2^-22 (relative) of the largest has the same sign.  A closer tie of mixed signs is
    decided by fp64 bits the record does not hold, and is left to the exact cases."""
    m = float(np.abs(e).max())
    if m == 0.0:
        return
    near = e[np.abs(e) >= m * (1.0 - 2.0 ** -22)]
    if np.all(near > 0) or np.all(near < 0):
        _metric(out, name, max(0.0, -float(near[0])), 0.0)


def object_metrics(got, pts, ref):
    """Metrics of one uoc_object record with count >= 1.  got: float32 fields centroid [3], cov [6] or [3,3], eig [3], axes [3,3]
    (column k = e_k), obb_half [3], obb_center [3]; pts [n,3]: the valid points (float64 holding float32 values); ref:
    the fp64 reference's centroid [3] and cov [3,3].

    Orthonormal, right-handed: ortho_bound; det > 0.  Eigenvalues: descending, none negative (bound 0).  Sign rule on e0
    and e1 (_sign_rule_metric).  Residual of each stored pair against the reference's covariance: residual_bound.

    Fixed-order sums, |got - ref| <= half an fp32 ulp + gamma.  centroid: gamma = 2 * sum_gamma(n, mean|x_i|).  cov(i, j):
    a term d_i d_j carries three roundings (two differences, one product), so gamma = 2 * (n + 3) 2^-53 mean|d_i d_j|;
    the two centroids differ by at most g_i = gamma of the centroid, which moves the moment by g_i g_j only, because the
    centred differences sum to zero up to g: + 4 g_i g_j.

    Box, recomputed in fp64 from the stored float32 centroid c and axes A over the points: d_k = (p - c) . a_k.  With
    r = max |p - c|_2: the kernel projected with its fp64 c' and a'_k, so d_k = d'_k + (c' - c) . a_k + (p - c') . (a_k -
    a'_k).  The first term is the same for every point, the second at most sqrt 3 * 2^-25 r =: eps.
      obb_half_k against (max - min) / 2: the common shift cancels: eps + half an ulp of the stored value.
      obb_center against c + A (max + min) / 2: A A^T (c' - c) gives back c' - c, so what is left is A eps (at most
        sqrt 3 eps = 3 * 2^-25 r per component) and (A - A') mid (at most 2^-25 |mid|_1 <= 3 * 2^-25 r): 3 * 2^-24 r + half
        an ulp.
      containment, |(p - center) . a_k| - half_k <= sqrt 3 * 2^-25 * 2 r (the rounded axis on |p - center| <= 2 r) + the
        sum of the centre's half-ulps + half an ulp of half_k.
    Every box bound adds 2^-45 (r + |c|_inf) for the fp64 evaluation and the second-order terms.  All of them are below
    2^-23 (r + |c|_inf) + half an ulp: 3.6e-7 m + half an ulp at r = 1 m, |c| = 2 m, against the 1e-5 m they stand beside."""
    out = []
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    g = {k: np.asarray(got[k], np.float32).astype(np.float64) for k in ("centroid", "cov", "eig", "axes", "obb_half", "obb_center")}
    g["cov"] = cov6(g["cov"])
    A, c, eig = g["axes"].reshape(3, 3), g["centroid"], g["eig"]
    C = np.asarray(ref["cov"], np.float64)
    l0 = max(float(np.linalg.eigvalsh(C)[-1]), 0.0)
    _metric(out, "orthonormal", np.abs(A.T @ A - np.eye(3)).max(), ortho_bound())
    _metric(out, "right_handed", 0.0 if np.linalg.det(A) > 0 else 1.0, 0.0)
    _metric(out, "eig_descending", max(0.0, eig[1] - eig[0], eig[2] - eig[1]), 0.0)
    _metric(out, "eig_nonnegative", max(0.0, -eig.min()), 0.0)
    for k in range(2):
        _sign_rule_metric(out, "sign_rule_e%d" % k, A[:, k])
    for k in range(3):
        _metric(out, "residual_e%d" % k, np.abs(C @ A[:, k] - eig[k] * A[:, k]).max(), residual_bound(l0))
    # fixed-order sums
    rc = np.asarray(ref["centroid"], np.float64)
    gam_c = 2.0 * sum_gamma(n, np.abs(pts).mean(axis=0))
    for i in range(3):
        hu = max(half_ulp(c[i]), half_ulp(rc[i]))
        _metric(out, "centroid[%d]" % i, abs(c[i] - rc[i]), hu + gam_c[i])
    d = pts - rc
    for m, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        gam = 2.0 * (n + 3) * U53 * float(np.abs(d[:, i] * d[:, j]).mean()) + 4.0 * gam_c[i] * gam_c[j]
        hu = max(half_ulp(g["cov"][m]), half_ulp(C[i, j]))
        _metric(out, "cov[%d]" % m, abs(g["cov"][m] - C[i, j]), hu + gam)
    # the box
    dd = pts - c
    r = float(np.sqrt((dd * dd).sum(axis=1)).max())
    slack = 2.0 ** -45 * (r + float(np.abs(c).max()))
    eps = SQ3 * U25 * r
    proj = dd @ A
    hi, lo = proj.max(axis=0), proj.min(axis=0)
    centre = c + A @ (0.5 * (hi + lo))
    hu_center = half_ulp(g["obb_center"])
    inside = np.abs((pts - g["obb_center"]) @ A).max(axis=0) - g["obb_half"]
    for k in range(3):
        hu = half_ulp(g["obb_half"][k])
        _metric(out, "obb_half[%d]" % k, abs(g["obb_half"][k] - 0.5 * (hi[k] - lo[k])), eps + hu + slack)
        _metric(out, "obb_center[%d]" % k, abs(g["obb_center"][k] - centre[k]), 3.0 * U24 * r + hu_center[k] + slack)
        _metric(out, "contained[%d]" % k, max(0.0, inside[k]), 2.0 * eps + hu_center.sum() + hu + slack)
    return out


def plane_metrics(got, pts, ref):
    """Metrics of one found uoc_plane record.  got: float32 normal, centroid, eig, u, v [3], d, rms; pts [n,3]: the
    inliers; ref: the fp64 reference's centroid and cov [3,3] of the inliers.

    (u, v, normal) orthonormal and right-handed: ortho_bound, which also holds u . normal = 0; v against normal x u of
    the stored vectors: each component is a difference of two products of numbers off by 2^-25, at most 4 * 2^-25, plus
    v's own rounding 2^-25 and FP64_SLACK.  d >= 0 (bound 0); where d == 0 the sign rule on the normal.
    Eigenvalues descending and never negative; rms^2 against eig[2]: rms = fl32(sqrt(lam)), eig = fl32(lam), so rms^2
    is within 2 * 2^-24 (1 + 2^-24) of lam and eig[2] within 2^-24: 3.5 * 2^-24 eig[2] + 2^-126 (the smallest normal:
    below it float32 rounds absolutely).
    Residual of (normal, eig[2]) against the reference's covariance: residual_bound.
    centroid, a fixed-order sum: half an ulp + 2 * sum_gamma(n, mean|x_i|).
    d against -(normal . centroid) of the stored float32 values: the normal moved by 2^-25 per component and the
    centroid by 2^-24 |c_i|, |n_i| <= 1: 3 * 2^-25 |c|_1 + half an ulp of d.  d itself depends on the direction of the
    normal and so on the eigen-gap; its agreement with the reference stays under the gap condition of check_frame."""
    out = []
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    g = {k: np.asarray(got[k], np.float32).astype(np.float64) for k in ("normal", "centroid", "eig", "u", "v", "d", "rms")}
    nn, u, v, c, eig, d, rms = g["normal"], g["u"], g["v"], g["centroid"], g["eig"], float(g["d"]), float(g["rms"])
    T = np.stack([u, v, nn], axis=1)
    _metric(out, "orthonormal", np.abs(T.T @ T - np.eye(3)).max(), ortho_bound())
    _metric(out, "right_handed", 0.0 if np.linalg.det(T) > 0 else 1.0, 0.0)
    _metric(out, "v_is_n_cross_u", np.abs(v - np.cross(nn, u)).max(), 5.0 * U25 + FP64_SLACK)
    _metric(out, "d_nonnegative", max(0.0, -d), 0.0)
    if d == 0.0:
        _sign_rule_metric(out, "sign_rule_normal", nn)
    _metric(out, "eig_descending", max(0.0, eig[1] - eig[0], eig[2] - eig[1]), 0.0)
    _metric(out, "eig_nonnegative", max(0.0, -eig.min()), 0.0)
    _metric(out, "rms", abs(rms * rms - eig[2]), 3.5 * U24 * eig[2] + 2.0 ** -126)
    C = np.asarray(ref["cov"], np.float64)
    l0 = max(float(np.linalg.eigvalsh(C)[-1]), 0.0)
    _metric(out, "residual_normal", np.abs(C @ nn - eig[2] * nn).max(), residual_bound(l0))
    rc = np.asarray(ref["centroid"], np.float64)
    gam_c = 2.0 * sum_gamma(n, np.abs(pts).mean(axis=0))
    for i in range(3):
        _metric(out, "centroid[%d]" % i, abs(c[i] - rc[i]), max(half_ulp(c[i]), half_ulp(rc[i])) + gam_c[i])
    _metric(out, "d", abs(d + float(nn @ c)), 3.0 * U25 * np.abs(c).sum() + half_ulp(d) + FP64_SLACK * np.abs(c).sum())
    return out


def height_metrics(height, plane, pts):
    """The height map over the valid points pts [n,3] against n . p + d of the stored float32 plane: the normal moved by
    2^-25 per component against |p|_1, d by half an ulp, and the stored height by half an ulp of its own."""
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)            # noqa: E731
    pts, h = np.asarray(pts, np.float64), f64(height)
    nn, d = f64(plane["normal"]), float(f64(plane["d"]))
    P = np.abs(pts).sum(axis=1)
    bound = U25 * P + half_ulp(d) + half_ulp(h) + 2.0 ** -45 * (P + abs(d))
    k = int(np.argmax(np.abs(h - (pts @ nn + d)) / bound))
    return [("height", float(abs(h[k] - (pts[k] @ nn + d))), float(bound[k]))]


def plane_object_metrics(got, plane, pts):
    """Metrics of one uoc_plane_object record with count >= 1 against the stored float32 plane it was measured in.
    got: float32 height_min, height_max, foot [2], cov2 [3], axis [2], half [3], center [3]; plane: float32 normal, d,
    centroid, u, v; pts [n,3] the id's valid points.

    Every quantity is recomputed in fp64 from the stored plane, so the bounds hold the float32 rounding of that plane
    and nothing about how well the plane itself is determined.  With c the plane's centroid, P = max |p|_1 and
    Q = max |p - c|_1 over the points:
      a height t = n . p + d moves by e_t = 2^-25 P (the normal) + half an ulp of d.  height, height_min, height_max:
        e_t + half an ulp of the stored value (the extremes of values each off by e_t are off by e_t); the height map
        likewise (height_metrics).
      an in-plane coordinate (p - c) . u moves by e_ab = 2^-25 Q (u, v) + 2^-24 |c|_1 (the centroid).
      foot, the mean of the in-plane coordinates, a fixed-order sum: e_ab + half an ulp + 2 * sum_gamma(n, mean|coordinate|).
      a centred coordinate uses the stored foot: e_r = e_ab + half an ulp of foot.  With R the largest |centred
        coordinate|, a product of two moves by 2 e_r R + e_r^2 and so does their mean: cov2 within that + half an ulp
        + the accumulation term 2 (n + 3) 2^-53 mean|product|.
      axis: a unit vector (2 sqrt 2 * 2^-25 + FP64_SLACK on |axis|^2 - 1), the sign rule, and the residual against the
        larger eigenvalue l of the recomputed cov2: the stored axis moved by 2^-25 per component against |C2 - l I|_inf
        <= (sqrt 2 + 1) l, and the recomputed C2 is off by E = the cov2 bound above in each entry, which moves C2 a by
        2 E and l by 2 E: (sqrt 2 + 1) 2^-25 l + 4 E + FP64_SLACK l.  An isotropic cov2 (s == 0) must give (1, 0).
      half and center of the upright box, with e' = (-e1, e0): an extent along e or e' moves by e_d = 2 e_r + 2^-25 * 2 R
        (the stored axis); along the normal by e_t.  half against (max - min) / 2: e_d (or e_t) + half an ulp.  center
        against c + a u + b v + mid_t n with (a, b) = foot + mid_0 e + mid_1 e': the mids move by e_d, e_d, e_t, foot by
        half an ulp each, and the three stored vectors by 2^-25 each against |a| + |b| + |mid_t|:
        2 e_d + e_t + 2 half-ulps of foot + 2^-25 (|a| + |b| + |mid_t|) + half an ulp of the stored value.
      containment: |(p - center) . axis_k| - half_k <= the centre's error summed over its components (3 e_c + its
        half-ulps) + the half bound + the rounding of the stored directions on |p - center|, 2^-25 * 4 (R + P)."""
    out = []
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)            # noqa: E731
    nn, c, u, v, d = f64(plane["normal"]), f64(plane["centroid"]), f64(plane["u"]), f64(plane["v"]), float(f64(plane["d"]))
    g = {k: f64(got[k]) for k in ("height_min", "height_max", "foot", "cov2", "axis", "half", "center")}
    P = float(np.abs(pts).sum(axis=1).max())
    Q = float(np.abs(pts - c).sum(axis=1).max())
    c1 = float(np.abs(c).sum())
    slack = 2.0 ** -45 * (P + c1)
    e_t = U25 * P + half_ulp(d) + slack
    t = pts @ nn + d
    _metric(out, "height_min", abs(g["height_min"] - t.min()), e_t + half_ulp(g["height_min"]))
    _metric(out, "height_max", abs(g["height_max"] - t.max()), e_t + half_ulp(g["height_max"]))
    e_ab = U25 * Q + U24 * c1 + slack
    ab = np.stack([(pts - c) @ u, (pts - c) @ v], axis=1)
    gam_f = 2.0 * sum_gamma(n, np.abs(ab).mean(axis=0))
    for i in range(2):
        _metric(out, "foot[%d]" % i, abs(g["foot"][i] - ab[:, i].mean()), e_ab + half_ulp(g["foot"][i]) + gam_f[i])
    rr = ab - g["foot"]
    e_r = e_ab + float(half_ulp(g["foot"]).max())
    R = float(np.abs(rr).max())
    C2 = np.array([(rr[:, 0] * rr[:, 0]).mean(), (rr[:, 0] * rr[:, 1]).mean(), (rr[:, 1] * rr[:, 1]).mean()])
    E = []
    for m, (i, j) in enumerate(((0, 0), (0, 1), (1, 1))):
        e = 2.0 * e_r * R + e_r * e_r + 2.0 * (n + 3) * U53 * float(np.abs(rr[:, i] * rr[:, j]).mean())
        E.append(e)
        _metric(out, "cov2[%d]" % m, abs(g["cov2"][m] - C2[m]), e + half_ulp(g["cov2"][m]))
    E = max(E)
    e = g["axis"]
    _metric(out, "axis_unit", abs(float(e @ e) - 1.0), 2.0 * math.sqrt(2.0) * U25 + FP64_SLACK)
    _sign_rule_metric(out, "sign_rule_axis", e)
    hd = 0.5 * (C2[0] - C2[2])
    s = math.hypot(hd, C2[1])
    lam = 0.5 * (C2[0] + C2[2]) + s
    M2 = np.array([[C2[0], C2[1]], [C2[1], C2[2]]])
    _metric(out, "residual_axis", np.abs(M2 @ e - lam * e).max(), (math.sqrt(2.0) + 1.0) * U25 * lam + 4.0 * E + FP64_SLACK * lam)
    ep = np.array([-e[1], e[0]])
    proj = np.stack([rr @ e, rr @ ep, t], axis=1)
    hi, lo = proj.max(axis=0), proj.min(axis=0)
    mid = 0.5 * (hi + lo)
    e_d = 2.0 * e_r + U25 * 2.0 * R
    e_k = (e_d, e_d, e_t)
    a, b = g["foot"] + mid[0] * e + mid[1] * ep
    centre = c + a * u + b * v + mid[2] * nn
    e_c = 2.0 * e_d + e_t + 2.0 * float(half_ulp(g["foot"]).max()) + U25 * (abs(a) + abs(b) + abs(mid[2])) + U24 * float(np.abs(c).max())
    hu_c = half_ulp(g["center"])
    T = np.stack([e[0] * u + e[1] * v, ep[0] * u + ep[1] * v, nn], axis=1)
    inside = np.abs((pts - g["center"]) @ T).max(axis=0) - g["half"]
    for k in range(3):
        hb = e_k[k] + half_ulp(g["half"][k])
        _metric(out, "half[%d]" % k, abs(g["half"][k] - 0.5 * (hi[k] - lo[k])), hb)
        _metric(out, "center[%d]" % k, abs(g["center"][k] - centre[k]), e_c + hu_c[k])
        _metric(out, "contained[%d]" % k, max(0.0, inside[k]), 3.0 * e_c + float(hu_c.sum()) + hb + U25 * 4.0 * (R + P))
    return out


NORMAL_SOLVER = 2.0 ** -46     # relative residual of an fp64 3x3 eigen-solve: at most 48 rotations (or LAPACK's QL sweeps) of
                               # a few 2^-53 each, 128 * 2^-53 in all


def frame_uncertainty(plane):
    """(dn, du, dv, dd, gam_c): how far two correct fp64 evaluations of the plane of `plane["points"]` can lie apart in the
    normal, u, v (2-norm) and d, and in the centroid (per component).  The frame is an eigenvector, so this depends on the
    eigen-gap, and the term below is what the gap costs; nothing is exempt, a vanishing gap gives an infinite bound.

    Each evaluation's covariance is within g = (n + 3) 2^-53 max mean|d_i d_j| of the exact one per entry (object_metrics),
    so the two matrices differ by at most 2 g per entry, 6 g in the 2-norm, and each solver leaves a residual of
    NORMAL_SOLVER * l0: E = 6 g + 2 NORMAL_SOLVER l0.  By Davis-Kahan the angle between the two normals has
    sin <= E / (gap - E) with gap = eig[1] - eig[2]; for gap >= 4 E that is a distance dn <= 2 E / gap, otherwise inf.
    u = (e_a - n_a n) / L with L = sqrt(1 - n_a^2): the numerator moves by at most 2 dn and normalising it by as much
    again over L, du <= 3 dn / L (inf below L = 1e-5, where the other axis may be chosen); v = n x u moves by dn + du.
    d = -(n . c): dn |c|_2 + the centroid's accumulation error sum gam_c + four roundings 2^-53 |c|_1; where |d| is
    below that, its sign and with it the orientation of the whole frame is open: everything inf."""
    pts = np.asarray(plane["points"], np.float64)
    n = len(pts)
    c = np.asarray(plane["centroid"], np.float64)
    eig = np.asarray(plane["eig"], np.float64)
    d = pts - c
    g = (n + 3) * U53 * max(float(np.abs(d[:, i] * d[:, j]).mean()) for i in range(3) for j in range(i, 3))
    E = 6.0 * g + 2.0 * NORMAL_SOLVER * float(eig[0])
    gap = float(eig[1] - eig[2])
    gam_c = 2.0 * sum_gamma(n, np.abs(pts).mean(axis=0))
    dn = 2.0 * E / gap if gap >= 4.0 * E and gap > 0 else math.inf
    nn = np.asarray(plane["normal"], np.float64)
    axis = 0 if math.sqrt(max(1.0 - nn[0] * nn[0], 0.0)) >= 1e-6 else 1
    L = math.sqrt(max(1.0 - nn[axis] * nn[axis], 0.0))
    du = 3.0 * dn / L if L >= 1e-5 else math.inf
    dd = dn * float(np.sqrt(c @ c)) + float(gam_c.sum()) + 4.0 * U53 * float(np.abs(c).sum())
    if abs(float(plane["d"])) <= dd:
        dn = du = dd = math.inf
    return dn, du, dn + du, dd, gam_c


def plane_reference_metrics(got, want):
    """The fixed-order sums of steps C and D against the fp64 reference itself: |got - ref| <= half an fp32 ulp + gamma +
    what the normal's fp64 uncertainty moves the field by (frame_uncertainty).  got: the float32 record of a found plane
    with its [128, ...] object fields (and `height` [H,W] or None); want: the reference's dict(plane, objects[, height, xyz]).

    With (dn, du, dv, dd, gam_c) of the plane, P2 = max |p|_2, P1 = max |p|_1, Q2 = max |p - c|_2, Q1 = max |p - c|_1 over
    an id's n points:
      d: dd.
      a height n . p + d (the map, height_min, height_max): dn P2 + dd + 4 * 2^-53 (P1 + d).
      an in-plane coordinate (p - c) . u: e_a = du Q2 + sum gam_c + 4 * 2^-53 Q1 (v: dv).  foot, its mean: e_a + gamma,
        gamma = 2 * sum_gamma(n, mean|coordinate|).
      a centred coordinate: the centroid's shift is the same in the coordinate and in the foot point and cancels; what is
        left is e_r = 2 du Q2 + 8 * 2^-53 Q1 (v: dv).  With R the largest |centred coordinate| of each kind, cov2 moves by
        2 e_ra R_a + e_ra^2, e_ra R_b + e_rb R_a + e_ra e_rb, 2 e_rb R_b + e_rb^2, plus gamma = 2 (n + 3) 2^-53 mean|product|.
    On a plane with an ordinary gap every added term is some 1e-13 m and the bound is half a float32 ulp for practical
    purposes: got == float32(ref) or its neighbour."""
    out = []
    p = want["plane"]
    dn, du, dv, dd, gam_c = frame_uncertainty(p)
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)            # noqa: E731

    def hu(a, b):
        return np.maximum(half_ulp(a), half_ulp(b))
    c, nn, u, v, d = (np.asarray(p[k], np.float64) for k in ("centroid", "normal", "u", "v", "d"))
    _metric(out, "ref.d", abs(float(f64(got["d"])) - float(d)), hu(got["d"], d) + dd)
    if got.get("height") is not None and want.get("height") is not None and "xyz" in want:
        m = ~np.isnan(want["height"]).reshape(-1)
        if m.any():
            pts = np.asarray(want["xyz"], np.float64).reshape(3, -1).T[m]
            h, r = f64(got["height"]).reshape(-1)[m], want["height"].reshape(-1)[m]
            bound = hu(h, r) + dn * np.sqrt((pts * pts).sum(axis=1)) + dd + 4.0 * U53 * (np.abs(pts).sum(axis=1) + abs(d))
            k = int(np.argmax(np.where(np.isfinite(bound), np.abs(h - r) / bound, 0.0)))
            _metric(out, "ref.height", abs(h[k] - r[k]), bound[k])
    for l, o in want["objects"].items():
        pts = np.asarray(o["points"], np.float64)
        n = len(pts)
        e_t = dn * float(np.sqrt((pts * pts).sum(axis=1)).max()) + dd + 4.0 * U53 * (float(np.abs(pts).sum(axis=1).max()) + abs(d))
        for k in ("height_min", "height_max"):
            _metric(out, "ref.%d.%s" % (l, k), abs(float(f64(got[k][l])) - o[k]), hu(got[k][l], o[k]) + e_t)
        q = pts - c
        Q2, Q1 = float(np.sqrt((q * q).sum(axis=1)).max()), float(np.abs(q).sum(axis=1).max())
        ab = np.stack([q @ u, q @ v], axis=1)
        rr = ab - np.asarray(o["foot"], np.float64)
        R = np.abs(rr).max(axis=0)
        e_r = []
        for i, dw in enumerate((du, dv)):
            e_a = dw * Q2 + float(gam_c.sum()) + 4.0 * U53 * Q1
            gam = 2.0 * sum_gamma(n, float(np.abs(ab[:, i]).mean()))
            _metric(out, "ref.%d.foot[%d]" % (l, i), abs(float(f64(got["foot"][l][i])) - o["foot"][i]), hu(got["foot"][l][i], o["foot"][i]) + e_a + gam)
            e_r.append(2.0 * dw * Q2 + 8.0 * U53 * Q1)
        move = (math.inf,) * 3
        if math.isfinite(e_r[1]):                                           # inf * 0 is no bound
            move = (2.0 * e_r[0] * R[0] + e_r[0] ** 2, e_r[0] * R[1] + e_r[1] * R[0] + e_r[0] * e_r[1], 2.0 * e_r[1] * R[1] + e_r[1] ** 2)
        for m2, (i, j) in enumerate(((0, 0), (0, 1), (1, 1))):
            gam = 2.0 * (n + 3) * U53 * float(np.abs(rr[:, i] * rr[:, j]).mean())
            _metric(out, "ref.%d.cov2[%d]" % (l, m2), abs(float(f64(got["cov2"][l][m2])) - o["cov2"][m2]),
                    hu(got["cov2"][l][m2], o["cov2"][m2]) + move[m2] + gam)
    return out


def worst(metrics):
    """(ratio, name) of the metric that uses most of its bound; a violated bound of 0 counts as infinite."""
    best = (0.0, "")
    for name, value, bound in metrics:
        ratio = value / bound if bound > 0 else (math.inf if value > 0 else 0.0)
        best = max(best, (ratio, name))
    return best


def assert_metrics(metrics, where):
    for name, value, bound in metrics:
        assert value <= bound, (where, name, value, bound)


# ---- frames -----------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("contiguous", "straddle", "scattered")
INVALID_Z = (0.0, np.nan, np.inf, -0.5)
BACKGROUND_IDS = (0, 128, -1)
FRAME, TINY_FRAME = (72, 128), (5, 13)      # 9216 pixels: two 4096-pixel blocks and one 1024-pixel wave; 65: a wave and a lane


def pixel_order(n_pix, placement, seed=0):
    """The order in which a frame's pixels are handed out.  contiguous: raster order from pixel 0.  straddle: outwards
    from the block borders 4096 and 8192 and the wave border 1024 in turn (1023, 1024, 4095, 4096, 8191, 8192, 1022, ...;
    in a frame without them, from pixel 64, where the second wave starts), so that even a two-point object lies in two
    waves.  scattered: a seeded permutation."""
    if placement == "contiguous":
        return np.arange(n_pix)
    if placement == "scattered":
        return np.random.default_rng(seed).permutation(n_pix)
    assert placement == "straddle"
    borders = [b for b in (1024, 4096, 8192) if b < n_pix] or [64 if n_pix > 64 else n_pix // 2]
    out, seen, k = [], set(), 0
    while len(out) < n_pix:
        for b in borders:
            for p in (b - 1 - k, b + k):
                if 0 <= p < n_pix and p not in seen:
                    seen.add(p)
                    out.append(p)
        k += 1
    return np.array(out)


def lay_out(shape, items, placement, seed=0, plane=False):
    """(labels [H,W] int32, xyz [3,H,W] float32): the points of `items` = [(id, p32 [n,3]), ...] laid along
    pixel_order, one item after the other (id 0: background points, the plane's candidates).  Of the pixels left over
    every fourth belongs to one of the items' ids with invalid depth (0, NaN, inf, negative in turn: it counts as a pixel
    and not as a point); the others carry the background ids 0, 128, -1, with invalid depth where `plane` (no further
    candidates) or for id -1, else with a valid point that no object may pick up."""
    H, W = shape
    N = H * W
    order = pixel_order(N, placement, seed)
    lab = np.zeros(N, np.int32)
    xyz = np.zeros((3, N), np.float32)
    j = 0
    for l, p in items:
        assert j + len(p) <= N, "the frame is too small for the items"
        px = order[j:j + len(p)]
        j += len(p)
        lab[px] = l
        xyz[:, px] = np.asarray(p, np.float32).T
    ids = [l for l, _ in items if l != 0]
    rng = np.random.default_rng(seed + 1)
    for k, px in enumerate(order[j:]):
        kind, turn = k % 4, k // 4
        x, y = rng.integers(-64, 64, 2) / 32.0
        if kind == 3 and ids:
            lab[px] = ids[turn % len(ids)]
            xyz[:, px] = (x, y, INVALID_Z[turn % 4])
        else:
            lab[px] = BACKGROUND_IDS[kind % 3]
            xyz[:, px] = (x, y, INVALID_Z[turn % 4] if (plane or kind == 2) else 0.75)
    return lab.reshape(H, W), xyz.reshape(3, H, W)


CASE_IDS = [1, 63, 64, 127] + [i for i in range(2, 127) if i not in (63, 64)]
TINY_CASES = ("two_x", "coincident", "single", "cube", "d45_xy_pos", "diagline5_xy", "fine_pair_x")


def object_groups():
    """group -> (frame shape, [(id, case name, translated), ...]).  `small`: every case but the big brick, plain and
    translated, 72 ids in one 72x128 frame; `big`: the 4096-point brick, plain and translated; `tiny`: 50 points in the
    65 pixels of a 5x13 frame."""
    cases = object_cases()
    small = [(n, t) for n, c in cases.items() if n != "big_brick" for t in ((False, True) if c["translate"] else (False,))]
    return dict(small=(FRAME, [(CASE_IDS[k], n, t) for k, (n, t) in enumerate(small)]),
                big=(FRAME, [(64, "big_brick", False), (127, "big_brick", True)]),
                tiny=(TINY_FRAME, [(CASE_IDS[k], n, False) for k, n in enumerate(TINY_CASES)]))


def object_group_frames(group, seed=0):
    """(labels [3,H,W], xyz [3,3,H,W]: the group in the three placements; expected {id: expected_object})."""
    cases = object_cases()
    shape, members = object_groups()[group]
    items = [(l, case_points(cases[n], t)[0]) for l, n, t in members]
    frames = [lay_out(shape, items, pl, seed) for pl in PLACEMENTS]
    want = {l: expected_object(cases[n], t) for l, n, t in members}
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), want


# ---- support-plane scenes ------------------------------------------------------------------------------------------------------
# The background is a symmetric grid of points on an exact plane, coordinates multiples of 1/8 m: dyadic, and a whole 125 mm,
# so every candidate is an integer millimetre point on the plane and every non-degenerate hypothesis scores M.
EIGHTH = 1 << (LATTICE_EXP - 3)
PLANE_NAMES = ("frontal", "tilted", "origin45")
BIG_PLATE_ID = 7
PLANE_SEEDS = (1, 20)       # with seed 20 hypothesis 0 is degenerate in every scene and placement: the winner is h >= 1


def _m(q):
    """Lattice integers -> float32 metres (exact)."""
    p = (np.asarray(q, np.float64) * 2.0 ** -LATTICE_EXP).astype(np.float32)
    assert np.array_equal(p.astype(np.float64) * 2.0 ** LATTICE_EXP, np.asarray(q, np.float64))
    return p


def _frontal_object(q):
    """Expected uoc_plane_object float fields of lattice points q [n,3] above the frontal plane z = 1 (normal (0, 0, -1),
    d = 1, centroid (0, 0, 1), u = (1, 0, 0), v = (0, -1, 0)): a = x, b = -y, t = 1 - z, all exact; Fractions throughout."""
    n = len(q)
    ulen = Fraction(1, 1 << LATTICE_EXP)
    a = [Fraction(int(v)) for v in q[:, 0]]
    b = [Fraction(-int(v)) for v in q[:, 1]]
    t = [Fraction((1 << LATTICE_EXP) - int(v)) for v in q[:, 2]]
    fa, fb = sum(a) / n, sum(b) / n
    assert float(fa * ulen) == fa * ulen and float(fb * ulen) == fb * ulen, "the foot point is no fp64 number"
    ra, rb = [x - fa for x in a], [x - fb for x in b]
    caa, cab, cbb = sum(x * x for x in ra) / n, sum(x * y for x, y in zip(ra, rb)) / n, sum(y * y for y in rb) / n
    tier2 = {}
    hd = caa - cbb
    if hd == 0 and cab == 0:
        branch, e = "s == 0", ((1, 0), False)
    elif cab == 0:
        branch, e = ("hd > 0, cab == 0", ((1, 0), False)) if hd > 0 else ("hd < 0, cab == 0", ((0, 1), False))
    else:
        assert hd == 0, "a general 2x2 axis is not an exact case"
        branch, e = ("hd == 0, cab > 0", ((1, 1), True)) if cab > 0 else ("hd == 0, cab < 0", ((1, -1), True))
    (e0, e1), diag = e
    axis = np.zeros(2, np.float32)
    for i, w in enumerate((e0, e1)):
        axis[i], tier2["axis[%d]" % i] = f32_round_checked(Fraction(w), diag)
    d0 = [x * e0 + y * e1 for x, y in zip(ra, rb)]
    d1 = [y * e0 - x * e1 for x, y in zip(ra, rb)]
    half = np.zeros(3, np.float32)
    for k, (dk, dg) in enumerate(((d0, diag), (d1, diag), (t, False))):
        half[k], tier2["half[%d]" % k] = f32_round_checked((max(dk) - min(dk)) / 2 * ulen, dg)
    assert max(d0) == -min(d0) and max(d1) == -min(d1), "footprint not symmetric about the foot point"
    mid_t = (max(t) + min(t)) / 2
    f = f32_exact
    return dict(count=n, height_min=f(min(t) * ulen), height_max=f(max(t) * ulen), foot=np.array([f(fa * ulen), f(fb * ulen)]),
                cov2=np.array([f(caa * ulen * ulen), f(cab * ulen * ulen), f(cbb * ulen * ulen)]), axis=axis, half=half,
                center=np.array([f(fa * ulen), f(-fb * ulen), f(((1 << LATTICE_EXP) - mid_t) * ulen)]), branch=branch, tier2=tier2)


@functools.lru_cache(maxsize=None)
def plane_scene(name, tiny=False):
    """dict(background [m,3] float32, objects {id: p32}, plane: expected uoc_plane float fields, expected {id: dict of the
    uoc_plane_object fields that are exact for that object}, tier2 {name: separation}).

    frontal: z = 1, a 32x16 grid (4x4 in the tiny frame) about (0, 0, 1): placement_reference.flat_plane() exactly.  Its
      objects take every branch of the 2x2 solver, and every float field of theirs is tier 1, or tier 2 where the axis is
      (1, +-1) / sqrt 2.  Id 7 is a 32x16x8 plate of 4096 points at x = -8 m, whose in-plane sums need more than 24 bits.
    tilted: z = 1 + x, a 5x32 grid about (2, 0, 3).  The five x offsets are 0, +-1/4, +-1/2 and their variance 2^-3: powers
      of two, so that the null eigenvalue and rms are exact zeros (see object_cases).  normal = (f, 0, -f), d = fl(1/sqrt 2),
      u = (f, 0, f), v = (0, -1, 0).
    origin45: z = x through the origin, the same grid about (2, 0, 2): normal . centroid = c * 2 - s * 2 == 0 exactly, the
      d == 0 branch, and the sign rule's magnitude tie between n_x and n_z goes to index 0: normal = (f, 0, -f).
    On the two tilted planes u and v are fp64 roundings of irrational vectors, so no in-plane sum is exact; a one-point
    object and two coincident points are still tier 2 in every field (the centred coordinates are exact zeros), and a brick
    is held to tier-2 heights and, like every record, to the checker."""
    ulen = Fraction(1, 1 << LATTICE_EXP)
    f = f32_exact
    tier2, objects, expected = {}, {}, {}
    if name == "frontal":
        nx, ny = (4, 4) if tiny else (32, 16)
        bg = grid((nx, ny, 1), (EIGHTH, EIGHTH, 1)) + np.array([0, 0, 1 << LATTICE_EXP])
        var = [Fraction(EIGHTH * EIGHTH * (k * k - 1), 3) * ulen * ulen for k in (nx, ny)]
        eig = sorted(var, reverse=True) + [Fraction(0)]
        plane = dict(normal=np.array([0, 0, -1], np.float32), d=np.float32(1), centroid=np.array([0, 0, 1], np.float32),
                     eig=np.array([f(v) for v in eig]), rms=np.float32(0), u=np.array([1, 0, 0], np.float32),
                     v=np.array([0, -1, 0], np.float32))
        shapes = [(1, grid((3, 3, 2), (8, 8, 16))), (63, grid((5, 3, 2), (8, 8, 16))), (64, grid((3, 5, 2), (8, 8, 16))),
                  (127, diag45((0, 1), 24, 16, 8)), (2, diag45((0, 1), 16, 24, 8)), (3, np.zeros((1, 3), np.int64)),
                  (4, grid((2, 1, 1), (8, 8, 8))), (5, np.zeros((5, 3), np.int64)), (6, grid((1, 2, 1), (8, 8, 8)))]
        if tiny:
            shapes = [s for s in shapes if s[0] in (1, 127, 3, 4, 5)]
        else:       # 4096 points 8 m off the centroid: the in-plane sums need 26 bits, a float32 accumulator loses some
            shapes.append((BIG_PLATE_ID, grid((32, 16, 8), (7, 9, 1))))        # and the centred moments 26 bits too
        for k, (l, rel) in enumerate(shapes):
            centre = np.array([(k % 3 - 1) * 1536 + 40, (k // 3 - 1) * 768 - 24, 1024 - 256 - 32 * k])
            if l == BIG_PLATE_ID:
                centre = np.array([OFFSET[0] + 5, OFFSET[1] - 3, 512 + 1])
            objects[l] = _m(rel + centre)
            expected[l] = _frontal_object(rel + centre)
            tier2.update({"%d.%s" % (l, kk): v for kk, v in expected[l].pop("tier2").items()})
    else:
        ny = 8 if tiny else 32
        cx = 2 << LATTICE_EXP
        cz = cx + (1 << LATTICE_EXP if name == "tilted" else 0)
        g = grid((5, ny, 1), (EIGHTH, EIGHTH, 1))
        bg = np.stack([g[:, 0] + cx, g[:, 1], g[:, 0] + cz], axis=1)
        a = Fraction(EIGHTH * EIGHTH * 24, 3)                      # the variance of the five x offsets: 2^17 units^2
        assert a == 1 << 17
        var_y = Fraction(EIGHTH * EIGHTH * (ny * ny - 1), 3)
        eig = sorted([2 * a * ulen * ulen, var_y * ulen * ulen], reverse=True) + [Fraction(0)]

        def r(num, key):                                           # num / sqrt 2 rounded once, its separation recorded
            val, tier2[key] = f32_round_checked(Fraction(num), True)
            return val
        fq = r(1, "f")
        plane = dict(normal=np.array([fq, 0, -fq], np.float32), d=r((cz - cx) * ulen, "d"),
                     centroid=np.array([f(cx * ulen), 0, f(cz * ulen)], np.float32), eig=np.array([f(v) for v in eig]),
                     rms=np.float32(0), u=np.array([fq, 0, fq], np.float32), v=np.array([0, -1, 0], np.float32))

        def point_object(l, q, copies):
            objects[l] = _m(np.repeat(q[None], copies, axis=0))
            h = r((q[0] - q[2] + cz - cx) * ulen, "%d.height" % l)
            fa = r((q[0] - cx + q[2] - cz) * ulen, "%d.foot_a" % l)
            expected[l] = dict(count=copies, height_min=h, height_max=h, foot=np.array([fa, f(-q[1] * ulen)], np.float32),
                               cov2=np.zeros(3, np.float32), axis=np.array([1, 0], np.float32), half=np.zeros(3, np.float32),
                               center=_m(q))
        point_object(1, np.array([cx + 96, 128, cz - 416]), 1)
        point_object(64, np.array([cx - 160, -256, cz - 800]), 2)
        rel = grid((3, 2, 2), (8, 8, 8)) + np.array([cx + 64, 320, cz - 640])
        objects[127] = _m(rel)
        t = rel[:, 0] - rel[:, 2] + cz - cx
        expected[127] = dict(count=len(rel), height_min=r(int(t.min()) * ulen, "127.height_min"),
                             height_max=r(int(t.max()) * ulen, "127.height_max"))
    return dict(background=_m(bg), objects=objects, plane=plane, expected=expected, tier2=tier2)


def plane_scene_frame(name, tiny, placement, seed=0):
    """(labels [H,W], xyz [3,H,W]) of a plane scene in one placement."""
    sc = plane_scene(name, tiny)
    items = [(0, sc["background"])] + [(l, p) for l, p in sc["objects"].items()]
    return lay_out(TINY_FRAME if tiny else FRAME, items, placement, seed, plane=True)


PLANE_EXACT = ("normal", "d", "centroid", "eig", "rms", "u", "v")


def assert_plane_exact(got, sc, where):
    for k in PLANE_EXACT:
        g = np.asarray(got[k], np.float32).reshape(np.shape(sc["plane"][k]))
        assert np.array_equal(g, sc["plane"][k]), (where, k, g.tolist(), np.asarray(sc["plane"][k]).tolist())
    for l, want in sc["expected"].items():
        assert int(got["count"][l]) == want["count"], (where, l, "count")
        for k, v in want.items():
            if k not in ("count", "branch"):
                g = np.asarray(got[k][l], np.float32).reshape(np.shape(v))
                assert np.array_equal(g, v), (where, l, k, g.tolist(), np.asarray(v).tolist())


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
# Which cases must reject which mutant, by the exact comparison or by the checker: (case name, translated).
_BRICKS = [("brick_%d%d%d" % p, False) for p in itertools.permutations(range(3))]
MUTANT_CASES = {
    "drop_point": [("brick_012", False), ("cube", False), ("two_x", True), ("d45_xy_pos", False), ("big_brick", True)],
    "point_twice": [("brick_012", False), ("cube", False), ("two_x", True), ("d45_xy_pos", False), ("big_brick", True)],
    "float32_sums": [("big_brick", True)],                         # 4096 points at 17 m: the sum needs 27 bits
    "float32_centroid": [("fine_pair_x", False), ("fine_pair_z", False)],      # the only centroids that are no float32
    "single_pass_float32": [("brick_012", True), ("cube", True), ("d45_xy_pos", True)],   # x^2 near 64: an ulp of 4e-6 m^2
    "e1_negated": [("brick_012", False), ("cube", False), ("d45_xy_neg", False), ("two_x", False)],
    "e2_flipped": [("brick_012", False), ("brick_102", False), ("d45_xy_pos", False), ("coincident", False)],
    "ascending": _BRICKS,
    # the mutant swaps on >= : on rod_x, variances (2, 1, 1), its first and last swap undo each other, so that case is not listed
    "unstable_sort": [(n, False) for n in ("cube", "plate_xy", "plate_yz", "plate_xz", "rod_y", "rod_z", "coincident")],
    "extents_about_origin": [("brick_012", False), ("brick_012", True), ("d45_xy_pos", True), ("two_x", False)],
    "min_max_swapped": [("brick_012", False), ("two_x", False), ("d45_xy_pos", False), ("patch_xy", True)],
}       # no_sign_rule: no exact case makes the solver return a vector the rule flips; it is judged on seeded scenes
MIN_MISS = 4.0


def same_record(a, b):
    return int(a["count"]) == int(b["count"]) and all(
        np.array_equal(np.asarray(cov6(a[k]) if k == "cov" else a[k], np.float32).reshape(-1),
                       np.asarray(cov6(b[k]) if k == "cov" else b[k], np.float32).reshape(-1)) for k in FLOAT_FIELDS)


def reference_record(p64):
    """What the checker needs of the fp64 reference: centroid and covariance of the points."""
    c = p64.mean(axis=0)
    d = p64 - c
    return dict(centroid=c, cov=d.T @ d / len(p64))


def mutant_rows():
    """[(mutant, case, translated, rejected by the exact comparison, the checker's worst value / bound, its metric)].
    The points come in a seeded shuffled order, as the scattered placement hands them to the kernel: in grid order the
    rounding errors of a float32 accumulator cancel by symmetry."""
    cases, rows = object_cases(), []
    for mutant, members in MUTANT_CASES.items():
        for name, translated in members:
            p32, _ = case_points(cases[name], translated)
            got = model_object(p32, mutant, order=np.random.default_rng(7).permutation(len(p32)))
            ratio, metric = worst(object_metrics(got, p32.astype(np.float64), reference_record(p32.astype(np.float64))))
            rows.append((mutant, name, translated, not same_record(got, expected_object(cases[name], translated)), ratio, metric))
    return rows


PLANE_MUTANTS = ("float32_foot_sums", "float32_cov2_sums")
FRONTAL = dict(normal=np.array([0.0, 0.0, -1.0]), d=1.0, centroid=np.array([0.0, 0.0, 1.0]), u=np.array([1.0, 0.0, 0.0]),
               v=np.array([0.0, -1.0, 0.0]))


def model_plane_object(p32, plane, mutant=None):
    """uoc_plane_object's float fields for the valid points p32 [n,3] of one id against the fp64 frame `plane` (normal, d,
    centroid, u, v), computed as step D of plane.hip does, every field cast once to float32; the points are summed in the
    order given.  `mutant` is None or one of PLANE_MUTANTS: the in-plane sums, or the centred second moments, accumulated
    in float32."""
    assert mutant is None or mutant in PLANE_MUTANTS
    p = np.asarray(p32, np.float32).astype(np.float64)
    n = len(p)
    nn, c, u, v, d = plane["normal"], plane["centroid"], plane["u"], plane["v"], float(plane["d"])
    t = p @ nn + d
    ab = np.stack([(p - c) @ u, (p - c) @ v], axis=1)

    def total(x):
        if mutant is None or (mutant == "float32_foot_sums") != (x is ab):
            return x.sum(axis=0)
        s = np.zeros(x.shape[1], np.float32)
        for row in x.astype(np.float32):
            s = s + row
        return s.astype(np.float64)
    foot = total(ab) / n
    r = ab - foot
    caa, cab, cbb = total(np.stack([r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 1] * r[:, 1]], axis=1)) / n
    hd = 0.5 * (caa - cbb)
    s = math.sqrt(hd * hd + cab * cab)
    e = np.array([1.0, 0.0])
    if s > 0.0:
        x, y = (s + hd, cab) if hd >= 0.0 else (cab, s - hd)
        e = np.array([x, y]) / math.sqrt(x * x + y * y)
        if (e[1] if abs(e[1]) > abs(e[0]) else e[0]) < 0.0:
            e = -e
    proj = np.stack([r[:, 0] * e[0] + r[:, 1] * e[1], r[:, 1] * e[0] - r[:, 0] * e[1], t], axis=1)
    hi, lo = proj.max(axis=0), proj.min(axis=0)
    mid = 0.5 * (hi + lo)
    a, b = foot[0] + (mid[0] * e[0] - mid[1] * e[1]), foot[1] + (mid[0] * e[1] + mid[1] * e[0])
    f = np.float32
    return dict(count=n, height_min=f(t.min()), height_max=f(t.max()), foot=foot.astype(f), cov2=np.array([caa, cab, cbb]).astype(f),
                axis=e.astype(f), half=(0.5 * (hi - lo)).astype(f), center=(c + a * u + b * v + mid[2] * nn).astype(f))


PLANE_OBJECT_FIELDS = ("height_min", "height_max", "foot", "cov2", "axis", "half", "center")


def plane_mutant_rows():
    """[(mutant, rejected by the exact comparison, plane_reference_metrics' worst value / bound, its metric)] on the big
    plate of the frontal scene in the scattered placement, its points in raster order."""
    from tests import support_reference as R
    sc = plane_scene("frontal")
    lab, xyz = plane_scene_frame("frontal", False, "scattered")
    want = R.fit(lab, xyz, 16, 10, 1)
    o = want["objects"][BIG_PLATE_ID]
    want = dict(plane=want["plane"], objects={BIG_PLATE_ID: o})
    rows = []
    for mutant in (None,) + PLANE_MUTANTS:
        rec = model_plane_object(o["points"].astype(np.float32), FRONTAL, mutant)
        got = dict(sc["plane"])
        for k in PLANE_OBJECT_FIELDS:
            got[k] = np.zeros((128,) + np.shape(rec[k]), np.float32)
            got[k][BIG_PLATE_ID] = rec[k]
        exact = any(not np.array_equal(rec[k], sc["expected"][BIG_PLATE_ID][k]) for k in PLANE_OBJECT_FIELDS)
        ratio, metric = worst(plane_reference_metrics(got, want))
        rows.append((mutant, exact, ratio, metric))
    return rows


def sign_rule_rows(point_sets):
    """The no_sign_rule mutant on arbitrary objects {key: p32}: [(key, flipped, ratio, metric)] where `flipped` says that
    the mutant's axes differ from the model's, and the ratio is the checker's verdict on the mutant."""
    rows = []
    for key, p32 in point_sets.items():
        good, bad = model_object(p32), model_object(p32, "no_sign_rule")
        ratio, metric = worst(object_metrics(bad, p32.astype(np.float64), reference_record(p32.astype(np.float64))))
        rows.append((key, not np.array_equal(good["axes"], bad["axes"]), ratio, metric))
    return rows
