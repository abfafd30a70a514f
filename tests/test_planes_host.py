"""CPU checks of tests/planes_reference.py: every scene of tests/test_planes_gpu.py contains what it is used for, the
reference's round 0 is support_reference.fit, and fit_planes refuses bad arguments before it touches a device."""
import math

import numpy as np
import pytest

from tests import planes_reference as P
from tests import support_reference as R

BANDS = ((3, 6), (10, 20), (10, 10))
SIZES = ((24, 32), (48, 64), (61, 83), (120, 160))
UP = tuple(float(x) for x in R.PLANE_N)


def surface_counts(lab, xyz, surf):
    idx, _ = R.candidates(lab, xyz)
    s = surf.reshape(-1)[idx]
    return {k: int((s == v).sum()) for k, v in P.SURFACES.items()}


def margins_ok(want, like):
    """Every planes_like cosine at least 1e-3 from its threshold, every standing_on decision at least 1 mm from its."""
    thr = math.cos(math.radians(15.0))
    for c in P.like_cosines(want, like):
        assert c is not None and abs(c - thr) >= 1e-3, (like, c)
    cls = P.planes_like(want, like)
    for l in range(1, P.NUM_IDS):
        hs = [want["objects"][k][l]["height_min"] for k in range(want["count"]) if cls[k] and l in want["objects"][k]]
        for h in hs:
            assert abs(h + 0.02) >= 1e-3, (like, l, h)
        kept = sorted(h for h in hs if h >= -0.02)
        assert len(kept) < 2 or kept[1] - kept[0] >= 1e-3, (like, l, kept)


@pytest.mark.parametrize("H,W", SIZES)
def test_shelves_hold_three_planes_with_fringes(H, W):
    mi = P.default_min_inliers(H, W)
    for seed in (1, 2):
        lab, xyz, surf = P.shelves(H, W, seed)
        n = surface_counts(lab, xyz, surf)
        for name in ("table", "board", "wall"):
            assert n[name] >= 2 * mi, (name, n, mi)
        assert 2 * n["far"] <= mi, (n, mi)
        assert set(np.unique(lab).tolist()) == {0, 1, 2, 3, 11, 12, 13}
        for tau_mm, rem_mm in BANDS:
            for hash_seed in (1, 2):
                want = P.fit(lab, xyz, 8, 256, tau_mm, rem_mm, mi, hash_seed)
                assert want["count"] == 3, (H, W, seed, tau_mm, rem_mm, hash_seed, want["count"])
                fringe = sum(i["removed"] - p["inliers"] for i, p in zip(want["info"], want["planes"]))
                assert (fringe > 0) == (rem_mm > tau_mm), (H, W, seed, tau_mm, rem_mm, fringe)
                assert (want["index"] >= P.FRINGE).sum() == fringe and (want["index"][lab > 0] == -2).all()
                cos = sorted(i["cos0"] for i in want["info"][1:3])
                assert abs(cos[0]) <= 0.05 and cos[1] > 0.99, cos                  # the wall and the board
                assert want["info"][0]["cos0"] == pytest.approx(1.0, abs=1e-12) and abs(want["info"][0]["offset0"]) < 1e-9
                k_board = 1 if want["info"][1]["cos0"] > 0.99 else 2
                assert abs(want["info"][k_board]["offset0"] - P.BOARD_T) < 0.005
                e = want["info"][0]["extent"]
                assert e[0] < 0 < e[1] and e[2] < 0 < e[3]
                on = P.standing_on(want)
                assert on[1:4] == [0, 0, 0] and on[11:14] == [k_board] * 3 and set(on[4:11] + on[14:]) == {-1}
                assert P.planes_like(want, 0)[:3] == [k == 0 or k == k_board for k in range(3)]
                assert P.choose_support(want) == 0 and P.choose_support(want, up=UP) == 0
                margins_ok(want, 0)
                margins_ok(want, UP)
                one = P.fit(lab, xyz, 1, 256, tau_mm, rem_mm, mi, hash_seed)
                assert one["count"] == 1 and np.array_equal(one["index"] == 0, want["index"] == 0)


@pytest.mark.parametrize("H,W", SIZES[:3])
def test_wall_dominant_variant_needs_up(H, W):
    mi = P.default_min_inliers(H, W)
    lab, xyz, surf = P.shelves(H, W, 1, 0.7, True)
    n = surface_counts(lab, xyz, surf)
    assert n["wall"] > n["table"] >= 2 * mi and n["board"] >= 2 * mi and 2 * n["far"] <= mi, (n, mi)
    want = P.fit(lab, xyz, 4, 256, 10, 20, mi, 1)
    assert want["count"] == 3
    assert abs(float(want["planes"][0]["normal"] @ R.PLANE_N)) < 0.05            # plane 0 is the wall, not the table
    assert float(want["planes"][1]["normal"] @ R.PLANE_N) > 0.99 and abs(want["info"][1]["cos0"]) < 0.05
    assert P.choose_support(want) == 0 and P.choose_support(want, up=UP) == 1      # without `up` the wall stays chosen
    assert P.standing_on(want, UP)[1:4] == [1, 1, 1]
    margins_ok(want, UP)


def test_round_zero_is_the_single_plane_reference():
    cases = [R.tabletop(61, 83, 1), R.tabletop(24, 32, 2)] + [f() for f in R.ENGINEERED.values()]
    for lab, xyz in cases:
        for num_hyp, tau_mm, seed in ((64, 10, 1), (16, 3, 2)):
            one = R.fit(lab, xyz, num_hyp, tau_mm, seed)
            many = P.fit(lab, xyz, 3, num_hyp, tau_mm, 2 * tau_mm, 3, seed)
            assert many["count"] >= one["plane"]["found"]
            for k, v in one["plane"].items():
                assert np.array_equal(np.asarray(many["planes"][0][k]), np.asarray(v)), k
            assert set(many["objects"][0]) == set(one["objects"])
            for l, o in one["objects"].items():
                for k, v in o.items():
                    assert np.array_equal(np.asarray(many["objects"][0][l][k]), np.asarray(v)), (l, k)


def test_stairs_use_every_slot_and_the_tie_rule():
    lab, xyz = P.stairs()
    per = lab.size // 8
    want = P.fit(lab, xyz, 8, 64, 3, 6, 3, 2)
    assert want["count"] == 8 and [p["inliers"] for p in want["planes"]] == [per] * 8
    assert [i["round_candidates"] for i in want["info"]] == [lab.size - r * per for r in range(8)]
    assert sorted(np.unique(want["index"]).tolist()) == list(range(8))
    _, q = R.candidates(lab, xyz)
    sc = R.scores(q, 64, 3, 2)
    assert (sc == sc.max()).sum() >= 2 and want["planes"][0]["hyp"] == int(np.argmax(sc))      # tied: the lowest h wins


def test_parallel_pair_is_absorbed_or_split_by_the_removal_band():
    lab, xyz = P.parallel_pair()
    half = int((lab == 0).sum()) // 2
    wide = P.fit(lab, xyz, 4, 64, 3, 20, 3, 1)
    assert wide["count"] == 1 and wide["planes"][0]["inliers"] == half and wide["info"][0]["removed"] == 2 * half
    assert (wide["index"] == P.FRINGE).sum() == half and wide["planes"][1]["candidates"] == 0
    tight = P.fit(lab, xyz, 4, 64, 3, 3, 3, 1)
    assert tight["count"] == 2 and [p["inliers"] for p in tight["planes"][:2]] == [half, half]
    assert abs(abs(tight["info"][1]["offset0"]) - 0.015) < 1e-6 and tight["info"][1]["cos0"] > 0.999999


def test_stop_rule_frames():
    for name, left in (("grid", 0), ("two_left", 2), ("coincident_left", 7)):
        lab, xyz = P.STOPS[name]()
        want = P.fit(lab, xyz, 4, 64, 3, 6, 3, 1)
        top = want["planes"][0]["inliers"]
        assert want["count"] == 1 and top == lab.size - left and want["planes"][1]["candidates"] == left, name
        assert want["planes"][2]["candidates"] == 0 and (want["index"] == -1).sum() == left
        if left >= 3:
            _, q = R.candidates(lab, xyz)
            assert (R.scores(q[P.fit(lab, xyz, 1, 64, 3, 6, 3, 1)["index"].reshape(-1) == -1], 64, 3, 2) == -1).all()
        assert P.fit(lab, xyz, 4, 64, 3, 6, top, 1)["count"] == 1 and P.fit(lab, xyz, 4, 64, 3, 6, top + 1, 1)["count"] == 0
    lab, xyz = P.stairs()
    a, b = P.fit(lab, xyz, 2, 64, 3, 6, 3, 0xFFFFFFFF), P.fit(lab, xyz, 1, 64, 3, 6, 3, 0xFFFFFFFF)
    _, q = R.candidates(lab, xyz)
    left = q[~np.isin(b["index"].reshape(-1), (0, P.FRINGE))]
    assert a["count"] == 2 and a["planes"][1]["hyp"] == int(np.argmax(R.scores(left, 64, 3, 0)))       # round 1 wraps to seed 0


def test_fit_planes_argument_errors():
    import torch
    from unseenobjectclustering_amd import _native, support
    lab, xyz = torch.zeros(4, 5, dtype=torch.int32), torch.zeros(3, 4, 5)
    for kw in (dict(max_planes=0), dict(max_planes=9), dict(num_hyp=0), dict(num_hyp=1025), dict(tau=0.0), dict(tau=1.5),
               dict(remove=0.005), dict(remove=1.001), dict(min_inliers=2)):
        with pytest.raises(ValueError):
            support.fit_planes(lab, xyz, **kw)
    with pytest.raises(_native.NativeError):
        support.fit_planes(lab, xyz)                       # tensors on the CPU: there is no fall-back
    assert support._IW == 8 and support.INFO_FIELDS == ("round_candidates", "removed", "cos0", "offset0", "extent")
    assert _native.PLANES_MAX == P.MAX_PLANES and _native.PLANES_FRINGE == P.FRINGE
