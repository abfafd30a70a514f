"""The engineered cases of tests/stats_cases.py on the CPU: each case is what it is named for, the reference passes its
own checker, and the comparisons can fail.

Mutants, and the cases that must reject each (stats_cases.MUTANT_CASES): one point dropped and one point counted twice
(bricks, the cube, two points, a 45-degree set, the big brick); sums accumulated in float32 (the big brick at 17 m, whose
sums need 27 bits); a float32 centroid used for centring (the fine pairs, whose centroid 16 + 2^-20 m is no float32: on the
2^-10 lattice every centroid is one, so no other case can show it); the single-pass E[x^2] - c^2 in float32 (the
translated cases); e1 negated, e2 = e1 x e0 (any case); eigenvalues ascending (the six bricks); an unstable sort (cube,
plates, rods, coincident points: only the exact comparison can see it); extents about the origin; min and max swapped.
The sign rule skipped: on the exact cases the solver returns identity columns or (c, -s), which the rule leaves alone, so
that mutant is judged by the checker on the seeded scene, where it must be rejected wherever it changes the axes.  Every
listed pair is rejected by the exact comparison, or by the checker with a miss of at least MIN_MISS = 4 times the bound.
Step D of the plane path with float32 in-plane sums, or float32 centred moments: the 4096-point plate of the frontal scene,
rejected by the exact comparison and by the comparison with the reference (plane_reference_metrics)."""
import math

import numpy as np
import pytest

from tests import objects_reference as OR
from tests import planes_reference as PR
from tests import stats_cases as S
from tests import support_reference as R

CASES = S.object_cases()
VARIANTS = [(n, t) for n, c in CASES.items() for t in ((False, True) if c["translate"] else (False,))]
F = np.float32(math.sqrt(0.5))


def rounded(rec, keys):
    return {k: np.asarray(rec[k], np.float64).astype(np.float32) for k in keys}


def test_object_cases_are_exact_in_every_order():
    for name, translated in VARIANTS:
        want = S.expected_object(CASES[name], translated)
        p32, _ = S.case_points(CASES[name], translated)
        rng = np.random.default_rng(len(p32))
        for trial in range(6):
            order = None if trial == 0 else rng.permutation(len(p32))
            S.assert_object_exact(S.model_object(p32, order=order), want, (name, translated, trial))


def test_object_cases_have_the_stated_structure():
    orders = {}
    for name, case in CASES.items():
        want = S.expected_object(case)
        eig3, pair = S.eigen_structure(case["rel"])
        orders[name] = want["order"]
        cov = dict(zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), want["cov"]))
        for (i, j), v in cov.items():
            if i != j and (i, j) != pair:
                assert v == 0.0, (name, i, j)
        if pair is None:                                     # a signed permutation matrix
            assert np.array_equal(np.abs(want["axes"]).sum(axis=0), [1, 1, 1]) and set(np.abs(want["axes"]).ravel()) <= {0.0, 1.0}
            assert np.array_equal(want["axes"][:, 0] >= 0, [True] * 3) and np.array_equal(want["axes"][:, 1] >= 0, [True] * 3)
            odd = want["order"] in ([0, 2, 1], [1, 0, 2], [2, 1, 0])
            assert want["axes"][:, 2].sum() == (-1.0 if odd else 1.0), name
        else:
            assert cov[pair] != 0.0 and cov[(pair[0], pair[0])] == cov[(pair[1], pair[1])], name
    values = lambda n: [v for v, _ in S.eigen_structure(CASES[n]["rel"])[0]]        # noqa: E731
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        n = "brick_%d%d%d" % perm
        assert len(set(values(n))) == 3 and orders[n] == list(perm), n
    assert len(set(values("cube"))) == 1 and orders["cube"] == [0, 1, 2] and orders["coincident"] == [0, 1, 2]
    assert orders["plate_xy"] == [0, 1, 2] and orders["plate_yz"] == [1, 2, 0] and orders["plate_xz"] == [0, 2, 1]
    assert orders["rod_x"] == [0, 1, 2] and orders["rod_y"] == [1, 0, 2] and orders["rod_z"] == [2, 0, 1]
    for n in ("plate_xy", "plate_yz", "plate_xz"):
        v = sorted(values(n))
        assert v[0] < v[1] == v[2], n                       # the tie on the two largest
    for n in ("rod_x", "rod_y", "rod_z"):
        v = sorted(values(n))
        assert v[0] == v[1] < v[2], n                       # the tie on the two smallest
    for n, zeros in (("two_x", 2), ("two_y", 2), ("two_z", 2), ("line5_x", 2), ("line5_y", 2), ("line5_z", 2), ("patch_xy", 1),
                     ("patch_yz", 1), ("patch_xz", 1), ("coincident", 3), ("single", 3), ("diagline2_xy", 2), ("diagline5_xy", 2),
                     ("tilted_patch_pos", 1), ("tilted_patch_neg", 1)):
        want = S.expected_object(CASES[n])
        assert np.count_nonzero(want["eig"] == 0) == zeros and np.array_equal(want["eig"] == 0, want["obb_half"] == 0), n
    for n in ("coincident", "single"):
        want = S.expected_object(CASES[n])
        assert np.array_equal(want["axes"], np.eye(3)) and not np.any(want["cov"]) and np.array_equal(want["obb_center"], want["centroid"])
    # the 45-degree tie: e0 = (f, f, 0) for cov_xy > 0, (f, -f, 0) for cov_xy < 0, the same in the other two planes
    for nm, (a, b) in (("xy", (0, 1)), ("xz", (0, 2)), ("yz", (1, 2))):
        for sign in ("pos", "neg"):
            want = S.expected_object(CASES["d45_%s_%s" % (nm, sign)])
            e0 = np.zeros(3, np.float32)
            e0[a], e0[b] = F, F if sign == "pos" else -F
            assert np.array_equal(want["axes"][:, 0], e0), (nm, sign, want["axes"])
            assert np.all(want["eig"] > 0) and len(set(want["eig"].tolist())) == 3
    assert np.array_equal(S.expected_object(CASES["d45_xy_pos_tall"])["axes"], np.array([[F, 0, F], [F, 0, -F], [0, 1, 0]], np.float32))
    # the rank-deficient 45-degree sets: a power-of-two variance and power-of-two coordinates in the rotated pair
    for n in ("diagline2_xy", "diagline5_xy", "tilted_patch_pos", "tilted_patch_neg"):
        rel = CASES[n]["rel"]
        _, (p, q) = S.eigen_structure(rel)
        var = int((rel[:, p] ** 2).sum())
        assert var % len(rel) == 0 and (var // len(rel)) & (var // len(rel) - 1) == 0, n
        assert all(v == 0 or v & (v - 1) == 0 for v in np.abs(rel[:, [p, q]]).ravel().tolist()), n
    # the fine pairs: the centroid is no float32
    for n, k in (("fine_pair_x", 0), ("fine_pair_z", 2)):
        c = CASES[n]["centre"][k] * 2.0 ** -20
        assert float(np.float32(c)) != c and S.expected_object(CASES[n])["cov"][(0, 5)[k // 2]] == np.float32(2.0 ** -40)


def test_tier2_values_are_separated_from_rounding_boundaries():
    seps = []
    for name, translated in VARIANTS:
        seps += [(name, k, v) for k, v in S.expected_object(CASES[name], translated)["tier2"].items()]
    for name in S.PLANE_NAMES:
        for tiny in (False, True):
            seps += [(name, k, v) for k, v in S.plane_scene(name, tiny)["tier2"].items()]
    assert any(math.isfinite(v) for _, _, v in seps)
    for name, k, v in seps:
        assert v >= S.TIER2_SEPARATION, (name, k, v)


def test_translation_moves_the_centre_and_nothing_else():
    off = np.array(S.OFFSET, np.float64) * 2.0 ** -S.LATTICE_EXP
    for name, case in CASES.items():
        if case["translate"]:
            a, t = S.expected_object(case), S.expected_object(case, True)
            for k in S.SHAPE_FIELDS:
                assert np.array_equal(a[k], t[k]), (name, k)
            for k in ("centroid", "aabb_min", "aabb_max", "obb_center"):
                assert np.array_equal(t[k].astype(np.float64), a[k].astype(np.float64) + off), (name, k)


@pytest.mark.parametrize("group", list(S.object_groups()))
def test_frames_hold_the_cases_where_the_placements_say(group):
    lab, xyz, want = S.object_group_frames(group)
    shape, members = S.object_groups()[group]
    if group == "small":
        assert {1, 63, 64, 127} <= {l for l, _, _ in members}
    n_pix = shape[0] * shape[1]
    recs, _, _, _, _ = OR.extract(lab, xyz)
    for b, placement in enumerate(S.PLACEMENTS):
        flat, X = lab[b].reshape(-1), xyz[b].reshape(3, -1)
        assert {0, 128, -1} <= set(flat.tolist())
        bad = ~(np.isfinite(X).all(axis=0) & (X[2] > 0))
        assert np.isnan(X[2]).any() and np.isinf(X[2]).any() and (X[2] == 0).any() and (X[2] < 0).any()
        for l, name, translated in members:
            p32, _ = S.case_points(CASES[name], translated)
            got = recs[b][l]["points"]
            assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, p32.astype(np.float64).tolist())), (placement, name)
            px = np.nonzero((flat == l) & ~bad)[0]
            if placement == "contiguous" and n_pix > 65:
                assert px.max() - px.min() == len(px) - 1
            if placement == "straddle" and len(px) >= 2 and n_pix > 1024:
                assert len(set((px // 1024).tolist())) >= 2, (name, px)     # a wave owns 1024 pixels: two waves at least
            if group == "small":
                assert (bad & (flat == l)).any(), (placement, name)     # pixels of the id that are no points
        if placement == "straddle" and n_pix > 8192:
            obj = (flat >= 1) & (flat < 128) & ~bad
            assert obj[[1023, 1024, 4095, 4096, 8191, 8192]].all()
        if placement == "scattered":
            ids_per_wave = [len(set(flat[w:w + 64][(flat[w:w + 64] >= 1) & (flat[w:w + 64] < 128)].tolist())) for w in range(0, n_pix, 64)]
            assert max(ids_per_wave) >= min(3, len(members))


@pytest.mark.parametrize("name", S.PLANE_NAMES)
def test_plane_scenes_have_the_stated_properties(name):
    for tiny in (False, True):
        sc = S.plane_scene(name, tiny)
        M = len(sc["background"])
        mm = sc["background"].astype(np.float64) * 8
        assert np.array_equal(mm, np.rint(mm))                                   # multiples of 1/8 m: whole 125 mm
        if name == "frontal":
            branches = {w["branch"] for w in sc["expected"].values()}
            want = {"s == 0", "hd > 0, cab == 0", "hd == 0, cab < 0"} | (set() if tiny else {"hd < 0, cab == 0", "hd == 0, cab > 0"})
            assert branches == want
            assert {len(p) for p in sc["objects"].values()} >= {1, 2, 5}
        for seed in S.PLANE_SEEDS:
            for placement in S.PLACEMENTS:
                lab, xyz = S.plane_scene_frame(name, tiny, placement)
                ref = R.fit(lab, xyz, 16, 10, seed, height_map=True)
                p, sc_ = ref["plane"], ref["scores"]
                nondeg = np.nonzero(sc_ >= 0)[0]
                assert p["found"] == 1 and p["candidates"] == p["inliers"] == M and np.all(sc_[nondeg] == M)   # every candidate an inlier
                assert p["hyp"] == nondeg[0] and (seed != 20 or p["hyp"] >= 1), (name, tiny, seed, placement, p["hyp"])
                for k in S.PLANE_EXACT:
                    assert np.abs(np.asarray(p[k]) - sc["plane"][k].astype(np.float64)).max() <= 1e-6, (name, k)
                for l, w in sc["expected"].items():
                    for k, v in w.items():
                        if k != "branch":
                            assert np.abs(np.asarray(ref["objects"][l][k], np.float64) - np.asarray(v, np.float64)).max() <= 1e-6, (name, l, k)


def _check_support_reference(ref, where):
    """The reference's own records, rounded to float32, through the plane checkers."""
    p = ref["plane"]
    got = rounded(p, S.PLANE_EXACT)
    S.assert_metrics(S.plane_metrics(got, p["points"], p), where)
    for l, o in ref["objects"].items():
        g = rounded(o, ("height_min", "height_max", "foot", "cov2", "axis", "half", "center"))
        S.assert_metrics(S.plane_object_metrics(g, got, o["points"]), (where, l))
    if ref.get("height") is not None:
        m = ~np.isnan(ref["height"]).reshape(-1)
        S.assert_metrics(S.height_metrics(ref["height"].reshape(-1)[m].astype(np.float32), got, ref["xyz"].T[m]), where)
    full = dict(got, height=None if ref.get("height") is None else ref["height"].astype(np.float32))
    for k in S.PLANE_OBJECT_FIELDS:                          # the [128, ...] layout of the GPU result
        full[k] = np.zeros((128,) + np.shape(next(iter(ref["objects"].values()))[k]) if ref["objects"] else (128, 3), np.float32)
        for l, o in ref["objects"].items():
            full[k][l] = o[k]
    S.assert_metrics(S.plane_reference_metrics(full, ref), where)


def test_the_reference_passes_its_own_checker():
    keys = ("centroid", "cov", "eig", "axes", "obb_half", "obb_center")
    # every new object case
    for name, translated in VARIANTS:
        p64 = S.case_points(CASES[name], translated)[0].astype(np.float64)
        r = OR.object_record(p64)
        got = rounded(dict(r, cov=r["cov"][np.triu_indices(3)]), keys)
        S.assert_metrics(S.object_metrics(got, p64, r), (name, translated))
    # the seeded scenes of tests/test_objects_gpu.py at their small sizes
    from tests.test_objects_gpu import synthetic
    n = 0
    for H, W, ids in ((7, 13, "all"), (24, 32, "all"), (48, 64, "gaps")):
        lab, xyz, _ = synthetic(2, H, W, seed=H * 7 + W, ids=ids)
        for b, frame in enumerate(OR.extract(lab, xyz)[0]):
            for l, r in frame.items():
                if r["count"] >= 1:
                    got = rounded(dict(r, cov=r["cov"][np.triu_indices(3)]), keys)
                    S.assert_metrics(S.object_metrics(got, r["points"], r), (H, W, b, l))
                    n += 1
    assert n > 300
    # every new plane scene, and the seeded scenes of tests/test_support_gpu.py and tests/test_planes_gpu.py
    for name in S.PLANE_NAMES:
        for tiny in (False, True):
            for placement in S.PLACEMENTS:
                lab, xyz = S.plane_scene_frame(name, tiny, placement)
                _check_support_reference(R.fit(lab, xyz, 16, 10, 1, height_map=True), (name, tiny, placement))
    for H, W, seed, tau_mm, num_hyp in ((61, 83, 1, 10, 64), (61, 83, 2, 3, 256), (24, 32, 1, 10, 64), (24, 32, 2, 3, 1024)):
        lab, xyz = R.tabletop(H, W, seed, noise=0.0015 if tau_mm == 3 else 0.0005)
        ref = R.fit(lab, xyz, num_hyp, tau_mm, seed, height_map=True)
        assert ref["plane"]["found"] == 1
        _check_support_reference(ref, (H, W, seed))
    for name in R.ENGINEERED:
        lab, xyz = R.ENGINEERED[name]()
        ref = R.fit(lab, xyz, 64, 10, 1, height_map=True)
        if ref["plane"]["found"]:
            _check_support_reference(ref, name)
    lab, xyz, _ = PR.shelves(24, 32, 1)
    ref = PR.fit(lab, xyz, 2, 64, 10, 20, PR.default_min_inliers(24, 32), 1)
    assert ref["count"] >= 1
    for r in range(ref["count"]):
        _check_support_reference(dict(plane=ref["planes"][r], objects=ref["objects"][r]), ("shelves", r))


def test_plane_path_mutants_are_rejected_with_margin():
    """Step D with its in-plane sums, or its centred moments, accumulated in float32, on the 4096-point plate of the frontal
    scene (x = -8 m: both need 26 bits): rejected by the exact comparison and, at MIN_MISS times the bound or more, by the
    comparison with the reference; the unmutated model passes both, on the plate and on every other frontal object."""
    rows = S.plane_mutant_rows()
    assert [r[0] for r in rows] == [None] + list(S.PLANE_MUTANTS)
    for mutant, exact, ratio, metric in rows:
        print("%-20s exact comparison %s, reference comparison %.3g x bound (%s)" % (mutant, "rejects" if exact else "passes", ratio, metric))
        if mutant is None:
            assert not exact and ratio <= 1.0
        else:
            assert exact and ratio >= S.MIN_MISS, (mutant, exact, ratio, metric)
    assert rows[1][3].endswith("foot[0]") and ".cov2" in rows[2][3]
    sc = S.plane_scene("frontal")
    for l, p32 in sc["objects"].items():
        rec = S.model_plane_object(p32, S.FRONTAL)
        for k in S.PLANE_OBJECT_FIELDS:
            assert np.array_equal(rec[k], sc["expected"][l][k]), (l, k)


def test_mutants_are_rejected_with_margin():
    rows = S.mutant_rows()
    assert {m for m, *_ in rows} == set(S.MUTANTS) - {"no_sign_rule"}
    for mutant, name, translated, exact, ratio, metric in rows:
        print("%-22s %-16s %-5s exact comparison %s, checker %.3g x bound (%s)" % (mutant, name, translated,
              "rejects" if exact else "passes", ratio, metric))
        assert exact or ratio >= S.MIN_MISS, (mutant, name, translated, ratio, metric)
        assert exact or mutant != "unstable_sort"
        if mutant != "unstable_sort":                       # the properties hold for any order within a tie
            assert ratio >= S.MIN_MISS, (mutant, name, translated, ratio, metric)
    # the unmutated model passes both on every one of those cases
    for name, translated in {(n, t) for _, n, t, *_ in rows}:
        p32, _ = S.case_points(CASES[name], translated)
        got = S.model_object(p32)
        assert S.same_record(got, S.expected_object(CASES[name], translated))
        assert S.worst(S.object_metrics(got, p32.astype(np.float64), S.reference_record(p32.astype(np.float64))))[0] <= 1.0
    # the sign rule skipped: rejected on every seeded object whose axes it changes
    from tests.test_objects_gpu import synthetic
    lab, xyz, _ = synthetic(2, 24, 32, seed=24 * 7 + 32)
    sets = {(b, l): r["points"].astype(np.float32) for b, frame in enumerate(OR.extract(lab, xyz)[0]) for l, r in frame.items()
            if r["count"] >= 3}
    rows = S.sign_rule_rows(sets)
    flipped = [r for r in rows if r[1]]
    assert len(flipped) >= 10
    for key, _, ratio, metric in flipped:
        assert ratio >= S.MIN_MISS and metric.startswith(("sign_rule", "right_handed")), (key, ratio, metric)
    for key, flip, ratio, metric in rows:
        assert flip or ratio <= 1.0, (key, ratio, metric)
