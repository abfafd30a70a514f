"""CPU proof behind tests/test_ms_euclidean_stages_gpu.py:
  1. the additions to the float64 restatement tests/ms_euclidean_reference.py agree with what it had (and with the golden
     vectors through it);
  2. every engineered decision case is exact: its coordinates are multiples of 2^-6 below 1 (so 128 products or squared
     differences sum without rounding in any order), the fp32 norm expansion and the fp32 direct differences, each in two
     channel orders, give the bits of float64, distinct squared distances keep distinct fp32 square roots, and the case takes
     the branch it was built for;
  3. every hill-climbing case is sensitive to one lost or repeated pixel (at least 10 x its tolerance), and the clamp case has
     exactly two weight sums below 1."""
import numpy as np
import pytest

from tests import ms_cosine_reference as G
from tests import ms_euclidean_cases as EC
from tests import ms_euclidean_reference as R
from tests.golden.cases import KAPPA

assert KAPPA == EC.KAPPA


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def d2_float64(X, Z):
    X, Z = np.asarray(X, np.float64), np.asarray(Z, np.float64)
    return np.stack([((X - z[None, :]) ** 2).sum(axis=1) for z in Z], axis=1)


def d2_expansion_fp32(X, Z, perm):
    """||x||^2 + ||z||^2 - 2 x.z, every operation in fp32, the channels visited in the order perm (sequential sums)."""
    X, Z = np.asarray(X, np.float32)[:, perm], np.asarray(Z, np.float32)[:, perm]
    xx = np.add.accumulate(X * X, axis=1, dtype=np.float32)[:, -1]
    zz = np.add.accumulate(Z * Z, axis=1, dtype=np.float32)[:, -1]
    S = np.stack([np.add.accumulate(X * z[None, :], axis=1, dtype=np.float32)[:, -1] for z in Z], axis=1)
    return (xx[:, None] + zz[None, :]) - np.float32(2) * S


def d2_direct_fp32(X, Z, perm):
    X, Z = np.asarray(X, np.float32)[:, perm], np.asarray(Z, np.float32)[:, perm]
    return np.stack([np.add.accumulate((X - z[None, :]) ** 2, axis=1, dtype=np.float32)[:, -1] for z in Z], axis=1)


def assert_exact(X, Z=None):
    """The distances between the distinct rows of X and of Z (X itself if none) are exact in fp32 in any order."""
    X = np.asarray(X, np.float32).reshape(-1, np.shape(X)[-1])
    X = np.unique(X[np.isfinite(X).all(axis=1)], axis=0)
    Z = X if Z is None else np.unique(np.asarray(Z, np.float32).reshape(-1, np.shape(Z)[-1]), axis=0)
    for A in (X, Z):
        assert np.array_equal(A * 64, np.rint(A * 64)) and np.abs(A).max() <= 1.0        # multiples of 2^-6: the proof
    if X.shape[0] > 300:
        X = X[np.random.default_rng(0).permutation(X.shape[0])[:300]]
    if Z.shape[0] > 300:
        Z = Z[np.random.default_rng(1).permutation(Z.shape[0])[:300]]
    want = d2_float64(X, Z)
    d = X.shape[1]
    for perm in (np.arange(d), np.random.default_rng(7).permutation(d)):
        assert np.array_equal(d2_expansion_fp32(X, Z, perm).astype(np.float64), want)
        assert np.array_equal(d2_direct_fp32(X, Z, perm).astype(np.float64), want)
    # distinct squared distances keep distinct fp32 square roots, at least 8 ulp apart (a square root within an ulp or two of
    # the rounded one decides as float64 does); equal ones are equal whatever the square root does
    v = np.unique(want)
    r = np.sqrt(v.astype(np.float32)).astype(np.float64)
    assert v.size == 1 or (np.diff(r) > 8 * 2.0 ** -23 * r[1:]).all()
    return want


def has_mixed_norms(*arrays):
    return all(len(np.unique((np.asarray(a, np.float64) ** 2).sum(axis=-1)[np.isfinite(a).all(axis=-1)])) >= 3 for a in arrays)


def cosine_picks(X, m, first):
    return G.select_seeds(X, m, first)[0]


def test_line_points_at_four_scales_are_exact():
    """The 65 line points at the four scales: all 260 x 260 squared distances bit-equal to float64 by both forms, and the
    identities the engineered ties use."""
    base = EC._base(0)
    P = np.concatenate([a * G.line(base, np.arange(65)) for a in EC.SCALES])
    D = assert_exact(P)
    assert len(np.unique(D)) > 300
    k, a = np.tile(np.arange(65), 4), np.repeat(EC.SCALES.astype(np.float64), 65)
    Dp = d2_float64(P, P)
    assert np.array_equal(Dp, (a[:, None] - a[None, :]) ** 2 + a[:, None] * a[None, :] * np.abs(k[:, None] - k[None, :]) / 16.0)
    p = lambda kk, aa=1.0: np.float32(aa) * G.line(base, kk)
    one = lambda x, z: float(d2_float64(x[None], z[None])[0, 0])
    assert one(p(9), p(9, 0.75)) == one(p(9), p(8)) == 1 / 16
    assert one(p(9), p(9, 0.5)) == one(p(9), p(13)) == one(p(9), p(13, 0.75)) == one(p(0, 0.5), p(16, 0.5)) == 0.25 == EC.EPS_EXACT ** 2
    assert np.float32(EC.EPS_EXACT) == EC.EPS_EXACT and np.sqrt(np.float32(0.25)) == np.float32(0.5)
    assert 0.25 < EC.EPS_BETWEEN ** 2 < 5 / 16


# ---- 1. the restatement's additions ------------------------------------------------------------------------------------------
def test_additions_agree_with_the_restatement():
    X = EC.hc_field(300, seed=3)
    idx, gaps = R.select_seeds(X, 34, 5)
    assert idx[0] == 5 and gaps[0] == np.inf and len(set(idx.tolist())) == 34
    cont, _ = R.select_seeds(X, 34, None, X[idx], 10)               # given the first ten picks, the rest follow
    assert (cont[:10] == -1).all() and np.array_equal(cont[10:], idx[10:])
    assert np.array_equal(R.seed_rows(X, cont, X[idx]), X[idx])
    Z = R.hill_climb(X, X[idx], KAPPA, 10)
    lab, rec = R.seed_components(Z, 0.2, record=True)
    assert np.array_equal(lab, R.seed_components(Z, 0.2)) and rec["pairs_at_eps"] == 0
    labels, gap = R.assign(X, Z, lab)
    exact, closest, nties = R.assign_exact(X, Z, lab)
    assert np.array_equal(labels[gap > 1e-9], exact[gap > 1e-9]) and (nties >= 1).all() and closest.max() < 34
    assert np.array_equal(R.assign(X, Z, lab, len(np.unique(lab)))[0], labels)
    for Zf in (R.hill_climb_fp32_direct(X, X[idx], KAPPA, 10), R.hill_climb_fp32_tiles(X, X[idx], KAPPA, 10)):
        assert Zf.dtype == np.float32 and 0 < np.abs(Zf - Z).max() < 1e-5
    ws = R.weight_sums(X, X[idx], KAPPA)
    one = (np.exp(-KAPPA * d2_float64(X, X[idx]))).sum(axis=0)
    assert np.allclose(ws, one, rtol=1e-9) and (ws >= 1 - 1e-9).all()          # a seed that is a row weighs itself 1


# ---- 2. the decision cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.fps_cases()))
def test_sampling_case(name):
    c = EC.fps_cases()[name]
    X, m, first = c["X"], c["m"], c["first"]
    assert_exact(X)
    cands = []
    idx, gaps = R.select_seeds(X, m, first, candidates=cands)
    assert (gaps[1:] == 0).any(), "no exact tie"
    if c["scaled"]:
        assert has_mixed_norms(X) and not np.array_equal(idx, cosine_picks(X, m, first))
    else:
        assert np.array_equal(idx, cosine_picks(X, m, first))       # unit rows: d = 2 sqrt(cosine distance), the same picks
    for tied in c["groups"]:
        # some pick's candidates are exactly the listed pixels, and the lowest wins
        steps = [s for s in range(m) if cands[s].tolist() == sorted(tied)]
        assert steps and idx[steps[0]] == min(tied), tied
    if "zero_tail" in c:
        assert (idx[-c["zero_tail"]:] == 0).all() and (gaps[-c["zero_tail"]:] == 0).all() and idx[-c["zero_tail"] - 1] != 0
    if c["groups"]:
        (a, b), (r0, r1), (w0, w1), s = c["groups"]
        assert a // 2048 != b // 2048 and a // 256 != b // 256              # blocks of the on-chip / the streaming kernel
        assert r0 // 64 == r1 // 64 and r0 % 4 == r1 % 4 and r0 // 16 == r1 // 16   # one row group in both pixel-to-lane maps
        assert w0 // 256 == w1 // 256 and w0 // 64 != w1 // 64
        assert s[1] == s[0] + 512 and len({p // 256 for p in s}) == 4
        assert not np.array_equal(X[w0], X[w1])                              # two distinct points, equally far
    else:
        assert (gaps[1:] == 0).sum() >= 5
        # some tie is between different points, not between copies of one
        assert any(len(cn) > 1 and len(np.unique(X[cn], axis=0)) > 1 for cn in cands)


@pytest.mark.parametrize("name", list(EC.fps_continuation_cases()))
def test_sampling_continuation_case(name):
    c = EC.fps_continuation_cases()[name]
    X, m, init, k = c["X"], c["m"], c["init"], c["num_init"]
    assert_exact(X, init)
    assert has_mixed_norms(X, init)
    assert (d2_float64(X, init[:k]) > 0).all()                               # no given row is a row of X
    idx, gaps = R.select_seeds(X, m, None, init, k)
    assert (idx[:k] == -1).all() and (idx[k:] >= 0).all()
    assert k == m or (gaps[k:] == 0).any()
    assert k == m or not np.array_equal(idx, G.select_seeds(X, m, None, init, k)[0])


def test_sampling_batch_case():
    c = EC.fps_batch_case()
    assert len(set(c["first"])) == 3
    picks = []
    for b in range(3):
        assert_exact(c["X"][b])
        assert has_mixed_norms(c["X"][b])
        idx, gaps = R.select_seeds(c["X"][b], c["m"], c["first"][b])
        assert (gaps[1:] == 0).any() and not np.array_equal(idx, cosine_picks(c["X"][b], c["m"], c["first"][b]))
        picks.append(idx.tolist())
    assert picks[0] != picks[1] != picks[2]


@pytest.mark.parametrize("name", list(EC.cc_cases()))
def test_component_case(name):
    Z, kind = EC.cc_cases()[name]
    m = Z.shape[0]
    assert_exact(Z)
    (lab, rec), (lab2, rec2) = (R.seed_components(Z, eps, record=True) for eps in (EC.EPS_EXACT, EC.EPS_BETWEEN))
    assert np.array_equal(lab, lab2) and rec2["pairs_at_eps"] == 0
    assert np.array_equal(lab, R.seed_components(Z, float(np.float32(EC.EPS_BETWEEN))))
    chain = kind.replace("scaled_", "")
    if chain in ("tied", "majority"):
        assert rec["pairs_at_eps"] >= 1 and rec["balls_with_labelled"] == 1 and rec["overwritten"] >= 1
        assert rec["tied_modes"] == (0 if chain == "majority" else 1)
        # stricter membership would change the answer: the threshold pairs matter
        assert not np.array_equal(R.seed_components(Z, np.nextafter(np.float32(EC.EPS_EXACT), np.float32(0))), lab)
        winner = 0 if chain == "tied" else 1
        assert lab[0] == 0 and lab[1] == 1 and lab[m - 1] == winner and sorted(set(lab.tolist())) == list(range(lab.max() + 1))
        trig = 2 if "_low_" in name else m - 2
        if m > 5:
            assert lab[trig] == winner and (m < 127 or lab[63] == lab[64] == winner)
    if kind.startswith("scaled"):
        nrm = (Z.astype(np.float64) ** 2).sum(axis=1)
        D = np.sqrt(d2_float64(Z, Z))
        i, j = np.nonzero(np.triu(D == EC.EPS_EXACT, 1))
        assert (nrm[i] != nrm[j]).sum() >= 3 and len({nrm[m - 1], nrm[0], nrm[2 if "_low_" in name else m - 2]}) == 2
        assert len(np.unique(nrm)) == 3
    if kind == "same":
        assert (lab == 0).all()
    if kind == "apart":
        assert lab.tolist() == list(range(m)) and (d2_float64(Z, Z) + 4 * np.eye(m) >= 1).all()


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("m", EC.ASSIGN_M)
def test_assignment_case(m, scale):
    Z = EC.assign_seeds(m, scale)
    sl, nu = EC.assign_labels(m)
    assert len(np.unique(sl)) == nu
    X = EC.assign_pixels(1025)
    assert_exact(X, Z)
    labels, closest, nties = R.assign_exact(X, Z, sl, nu)
    base = G.line(EC.CS._base(6), 0).astype(np.float64)
    ks = np.rint(16 * d2_float64(X, base[None])[:, 0]).astype(int)
    pairs = EC.tie_pairs(m)
    assert len(pairs) == {1: 0, 9: 2, 17: 3, 20: 4, 33: 5, 57: 5, 80: 5, 81: 5, 89: 5, 96: 5, 100: 5, 128: 6}[m]
    nrm = (Z.astype(np.float64) ** 2).sum(axis=1)
    for k, (a, b) in pairs.items():
        sel = ks == k
        assert set((np.nonzero(sel)[0] % 4).tolist()) == {0, 1, 2, 3}      # the tie is met in every pixel slot of a lane
        assert (nties[sel] == 2).all() and (closest[sel] == min(a, b)).all()
        D = d2_float64(X[sel][:1], Z)[0]
        assert D[a] == D[b] == 1.0 / 16 and (nrm[a] != nrm[b]) == scale
    if scale and m > 9:
        assert len(np.unique(nrm)) >= 3
    for n in EC.ASSIGN_N:           # the smaller pixel counts are prefixes: the same rows
        assert np.array_equal(EC.assign_pixels(n), X[:n])


def test_cases_cover_every_instantiation():
    assert {(m + 15) // 16 for m in EC.ASSIGN_M} == set(range(1, 9))
    combos = {EC.instantiation(m) for m in EC.HC_TILE_M}
    assert combos == {(st, quad) for st in range(1, 9) for quad in (False, True)} - {(1, True)}
    assert [EC.instantiation(m) for m in EC.HC_SCALED_M] == [(7, True), (6, False)]
    assert {EC.instantiation(m) for m in EC.HC_EDGE_M} == {(7, True), (6, False)}


@pytest.mark.parametrize("m", EC.PAD_M)
def test_padding_case(m):
    X, Z = EC.padding_case(m)
    D = assert_exact(X, Z)
    assert has_mixed_norms(X)
    D = d2_float64(X, Z)
    assert (D > (X.astype(np.float64) ** 2).sum(axis=1)[:, None]).all()      # a zero row (d = ||x||) would beat every real seed
    _, closest, _ = R.assign_exact(X, Z, np.arange(m) % 3)
    assert closest.max() < m


@pytest.mark.parametrize("name", list(EC.swap_cases()))
def test_swap_case(name):
    X, Z, sl, nu = EC.swap_cases()[name]
    assert_exact(X, Z)
    labels, closest, nties = R.assign_exact(X, Z, sl, nu)
    assert (nties == 1).all()
    want, wc, _ = G.assign(X, Z, sl, nu)              # unit rows on their seeds: the cosine answer
    assert np.array_equal(labels, want) and np.array_equal(closest, wc)


@pytest.mark.parametrize("n,m,wide", sorted({(n, m, w) for n, m, w, _ in EC.WHOLE}))
def test_whole_call_case(n, m, wide):
    halves_differ = 0
    for k in range(5):
        X = EC.whole_field(n, k, wide)
        assert X.shape == (n, 128 if wide else 64) and has_mixed_norms(X)
        assert_exact(X)
        first = (37 * k + 11) % n
        labels, idx, Z, sl = R.cluster_exact(X, m, EC.WHOLE_EPS, first)
        _, gaps = R.select_seeds(X, m, first)
        _, _, nties = R.assign_exact(X, Z, sl)
        assert (gaps[1:] == 0).any() and (nties > 1).any() and len(np.unique(sl)) > 1
        assert not np.array_equal(idx, cosine_picks(X, m, first))
        if wide:
            # the two planes carry different parts of the norms: neither half alone orders the rows as the whole does
            h0, h1 = (X[:, :64].astype(np.float64) ** 2).sum(axis=1), (X[:, 64:].astype(np.float64) ** 2).sum(axis=1)
            assert len(np.unique(h0)) >= 3 and len(np.unique(h1)) >= 3
            halves_differ += not np.array_equal(h0, h1)
            X64 = EC.whole_field(n, k, False)
            assert np.array_equal(R.cluster_exact(X64, m, EC.WHOLE_EPS, first)[0], labels)
    if wide:
        assert halves_differ >= 3           # (a line point has half its norm in either plane; the lattice points do not)
        assert np.array_equal(G.planes(X)[0], X[:, :64]) and np.array_equal(G.planes(X)[1], X[:, 64:])


@pytest.mark.parametrize("n", EC.NOSEED_N)
def test_no_seed_case(n):
    """As built: two NaN rows (one in a full pixel tile, the last one), two seed tiles, no finite pixel on a tie, and label 0
    the largest only because the two NaN rows count under it."""
    X, Z, sl, nu = EC.noseed_case(n)
    bad = list(EC.noseed_rows(n))
    fin = np.setdiff1d(np.arange(n), bad)
    assert bad[0] < 16 and bad[1] == n - 1 and (n - 1) // 16 == (n + 15) // 16 - 1 and (Z.shape[0] + 15) // 16 == 2
    assert np.isnan(X[bad]).all() and sl[0] == 0 and nu == 2
    assert_exact(X[fin], Z)
    labels, closest, nties = R.assign_exact(X, Z, sl, nu)
    assert (nties[fin] == 1).all() and (nties[bad] == 0).all() and (closest[bad] == 0).all() and (labels[bad] == 0).all()
    raw = sl[closest]
    assert np.array_equal(labels, raw)                                       # no swap ...
    assert (raw[fin] == 1).sum() == (raw[fin] == 0).sum() + 1                # ... though label 1 leads among the finite rows
    without, _, _ = R.assign_exact(X[fin], Z, sl, nu)
    assert np.array_equal(without, 1 - raw[fin])
    D = np.sort(d2_float64(X[fin], Z), axis=1)[:, :2]
    assert (D == np.array([1.0, 3.0]) / 16).all()


# ---- 3. the climb cases see one pixel ------------------------------------------------------------------------------------------
def sensitivity(X, Z0, iters):
    """(tolerance of the case, {mutation: distance of the mutated float64 result from the full one})."""
    ref, devs = EC.climb_yardstick(X, Z0, KAPPA, iters)
    tol = EC.climb_tolerance(devs)
    return tol, {k: float(np.abs(R.hill_climb(Xm, Z0, KAPPA, iters) - ref).max()) for k, Xm in EC.hc_mutations(X).items()}


def assert_sensitive(what, X, Z0, iters):
    tol, moved = sensitivity(X, Z0, iters)
    for k, v in moved.items():
        print("%s: %s moves the seeds by %.2e = %.0f x the tolerance %.2e" % (what, k, v, v / tol, tol))
        assert v >= 10 * tol, (what, k, v, tol)
    return tol, moved


@pytest.mark.parametrize("iters", EC.HC_TILE_ITERS)
@pytest.mark.parametrize("m", EC.HC_TILE_M)
def test_climb_tile_cases_are_sensitive(m, iters):
    X = EC.hc_field(1961)
    _, moved = assert_sensitive("n 1961 m %d iters %d" % (m, iters), X, EC.hc_seeds(X, m)[0], iters)
    assert len(moved) == 3


@pytest.mark.parametrize("m", EC.HC_EDGE_M)
@pytest.mark.parametrize("n", EC.HC_EDGE_N + [4097])
def test_climb_edge_cases_are_sensitive(n, m):
    for k in range(3 if n == 4097 else 1):
        X = EC.hc_field(n, seed=1 + k)
        _, moved = assert_sensitive("n %d m %d field %d" % (n, m, k), X, EC.hc_seeds(X, m, k)[0], 10)
        assert len(moved) == (0 if n == 1 else 2 if n < 17 else 3)


def test_climb_batch_cases_are_sensitive():
    batch, n, m = EC.HC_STRIDED
    tol = EC.climb_tolerance(EC.strided_yardstick())          # the batch's: the largest deviations over the sampled fields
    for b in range(0, batch, EC.STRIDED_SAMPLE):
        X, Z0 = EC.strided_field(b)
        ref = R.hill_climb(X, Z0, KAPPA, 10)
        assert EC.climb_tolerance(EC.climb_yardstick(X, Z0, KAPPA, 10)[1]) <= tol
        for k, Xm in EC.hc_mutations(X).items():
            v = float(np.abs(R.hill_climb(Xm, Z0, KAPPA, 10) - ref).max())
            print("strided field %d: %s moves the seeds by %.2e = %.0f x the tolerance %.2e" % (b, k, v, v / tol, tol))
            assert v >= 10 * tol, (b, k, v, tol)
    _, n, m, fields = EC.HC_AFFINE
    for b in fields:
        assert_sensitive("affine field %d" % b, EC.hc_affine_field(b), EC.hc_affine_seeds(b), 10)


@pytest.mark.parametrize("n,m", EC.HC_WIDE + [(n, 100) for n in EC.HC_OVERREAD_N])
def test_climb_wide_and_overread_cases_are_sensitive(n, m):
    wide = (n, m) in EC.HC_WIDE
    X = EC.hc_field(n, seed=7, channels=128 if wide else 64)
    # the 128-d cases climb from the seeds the whole call samples itself
    Z0 = X[R.select_seeds(X, m, EC.WIDE_FIRST)[0]] if wide else EC.hc_seeds(X, m)[0]
    assert_sensitive("n %d m %d %s" % (n, m, "128-d" if wide else "over-read"), X, Z0, 10)


@pytest.mark.parametrize("m", EC.HC_SCALED_M)
def test_climb_scaled_case_is_sensitive(m):
    X, Z0 = EC.hc_scaled_case(m)
    for A in (X, Z0):
        nrm = (A.astype(np.float64) ** 2).sum(axis=1)
        assert len(np.unique(np.round(nrm, 2))) == 4 and nrm.min() < 0.3 and nrm.max() > 1.5
    assert_sensitive("scaled rows m %d" % m, X, Z0, 10)


def test_climb_wide_scaled_case_is_sensitive():
    n, m = EC.HC_WIDE_SCALED
    X = EC.hc_wide_scaled_field()
    Z0 = X[R.select_seeds(X, m, EC.WIDE_FIRST)[0]]
    nrm = (Z0.astype(np.float64) ** 2).sum(axis=1)
    assert X.shape == (n, 128) and n % 16 == 9 and nrm.min() < 0.3 and nrm.max() > 1.5
    tol, _ = assert_sensitive("128-d scaled rows", X, Z0, 10)
    # seven zero rows that kept their weight (an unmasked last pixel tile) are seen here, and are not in the unit 128-d case
    ref = R.hill_climb(X, Z0, KAPPA, 10)
    padded = R.hill_climb(np.concatenate([X, np.zeros((7, 128), np.float32)]), Z0, KAPPA, 10)
    assert np.abs(padded - ref).max() >= 100 * tol


def test_climb_clamp_case():
    """Two weight sums below 1 (the clamp's active side), every other above 1, at the first iteration; the far seed's new
    position is the origin to fp32 resolution; and the case sees one pixel like every other."""
    n, m, far, half = EC.HC_CLAMP
    X, Z0 = EC.hc_clamp_case()
    ws = R.weight_sums(X, Z0, KAPPA)
    print("weight sums: far seed %.2e, half-row seed %.3f, the smallest other %.1f" % (ws[far], ws[half], np.delete(ws, [far, half]).min()))
    assert ws[far] < 1e-9 and 0.05 < ws[half] < 1 and (np.delete(ws, [far, half]) > 1).all()
    Z1 = R.hill_climb(X, Z0, KAPPA, 1)
    assert np.abs(Z1[far]).max() < 1e-9 and 0.01 < np.abs(Z1[half]).max() < 0.3
    # without the clamp the half-row seed would land on a mean of field rows: an O(1) difference
    unclamped = (np.exp(-KAPPA * d2_float64(X, Z0[half][None]))[:, 0] @ X.astype(np.float64)) / ws[half]
    assert np.abs(unclamped - Z1[half]).max() > 0.05
    assert_sensitive("clamp", X, Z0, 10)
