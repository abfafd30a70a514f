"""The numpy restatement of uoc_placement (tests/placement_reference.py): its separable distance transform against the
all-pairs definition, a hand-counted 4x4 grid, the floor-division rule, need2, the engineered frames against where
their points are meant to land, and the seeded scenes against what the GPU tests use them for.  No GPU."""
import functools

import numpy as np
import pytest

from tests import placement_reference as R

# the parameter sets of the seeded scenes in tests/test_placement_gpu.py: (G, cell_mm, h_obs_mm, tau_mm, min_pts, unknown_blocks)
PARAMS = [(64, 10, 10, 10, 1, 1), (256, 10, 10, 10, 1, 1), (256, 5, 20, 8, 3, 0), (64, 50, 10, 10, 3, 1), (8, 50, 20, 8, 1, 0),
          (512, 5, 10, 10, 1, 1)]


@functools.lru_cache(maxsize=None)
def scene(H, W, seed):
    return R.tabletop(H, W, seed)


def test_separable_transform_matches_all_pairs():
    rng = np.random.default_rng(7)
    for G in (8, 16):
        for density in (0.0, 0.02, 0.1, 0.5, 1.0):
            for _ in range(3):
                blocking = rng.random((G, G)) < density
                assert np.array_equal(R.edt(blocking), R.edt_brute(blocking)), (G, density)
    one = np.zeros((8, 8), bool)
    one[0, 7] = True
    assert np.array_equal(R.edt(one), R.edt_brute(one))


def test_hand_counted_4x4():
    # blocking:  . . . .     dist2:  1 1 1 1      (the border of virtual blocking cells is one step from every edge cell;
    #            . . # .             1 1 0 1       the four centre cells would be 4 without the # at (1, 2))
    #            . . . .             1 2 1 1
    #            . . . .             1 1 1 1
    blocking = np.zeros((4, 4), bool)
    blocking[1, 2] = True
    assert R.edt(blocking).tolist() == [[1, 1, 1, 1], [1, 1, 0, 1], [1, 2, 1, 1], [1, 1, 1, 1]]
    assert R.column_distance(blocking).tolist() == [[1, 1, 1, 1], [2, 2, 0, 2], [2, 2, 1, 2], [1, 1, 1, 1]]
    free = np.zeros((4, 4), bool)
    assert R.edt(free).tolist() == [[1, 1, 1, 1], [1, 4, 4, 1], [1, 4, 4, 1], [1, 1, 1, 1]]
    assert not R.edt(np.ones((4, 4), bool)).any()
    # the same grid from points: four table points per row, the obstacle a labelled point 5 cm up; G = 8 holds it in its middle
    state = np.ones((4, 4), np.int64)
    state[1, 2] = 2
    d2 = R.edt(state == 2)
    assert R.answer(state, d2, (2, 0, 0, R.WIDEST)) == (2, 1, 2, 1) and R.answer(state, d2, (3, 0, 0, R.WIDEST)) == (2, 1, 2, 0)
    assert R.answer(state, d2, (1, 1, 2, R.NEAREST)) == (0, 2, 1, 1)          # four cells at distance 1, all dist2 1: lowest index
    assert R.answer(state, d2, (2, 0, 0, R.NEAREST)) == (2, 1, 2, 1) and R.answer(state, d2, (3, 0, 0, R.NEAREST)) == R.NO_ANSWER
    assert R.answer(np.zeros((4, 4), np.int64), d2, (0, 0, 0, R.WIDEST)) == R.NO_ANSWER


def test_floor_division_on_negative_coordinates():
    F = R.frame_record(R.flat_plane())
    assert F.tolist() == [0, 0, -16384, 16384000, 16384, 0, 0, 0, -16384, 0, 0, 0, 1000, 1, 0, 0]
    lab, xyz = R.frame_of([(-1, 0, 1000, 0), (-10, 0, 1000, 0), (-11, 0, 1000, 0), (0, 1, 1000, 0), (0, 10, 1000, 0), (0, 11, 1000, 0),
                           (0, -1, 1000, 0)], 1, 7)
    ev = R.point_events(lab, xyz, F, 16, 10, 20, 10)
    assert ev["i"].tolist() == [7, 7, 6, 8, 8, 8, 8] and ev["j"].tolist() == [8, 8, 8, 7, 7, 6, 8]      # C truncation would give 8, 7, 7
    assert (ev["T"] == 0).all() and (ev["cls"] == R.TABLE).all()


def test_frame_record_rules():
    p = R.true_plane()
    F = R.frame_record(p)
    assert F[13] == 1 and abs(int(F[0]) ** 2 + int(F[1]) ** 2 + int(F[2]) ** 2 - R.S ** 2) < 4 * R.S
    assert F[3] == int(np.rint(np.float64(np.float32(R.PLANE_D)) * 16384000.0))
    for bad in (dict(found=0), dict(found=2), dict(d=np.float32(np.nan)), dict(d=np.float32(1001.0)), dict(normal=np.array([0, np.inf, 0], np.float32)),
                dict(u=np.array([2.5, 0, 0], np.float32)), dict(centroid=np.array([0, 32.768, 1], np.float32)),
                dict(centroid=np.array([np.nan, 0, 1], np.float32))):
        assert not R.frame_record({**p, **bad}).any(), bad
    assert R.frame_record({**p, "centroid": np.array([0, 32.767, 1], np.float32)})[13] == 1
    r = R.free_space(*scene(24, 32, 1), {**p, "found": 0}, 8, 10, 10, 10, 1, 0, [(0, 0, 0, 0)])
    assert not any(r[k].any() for k in ("state", "owner", "dist2", "counts", "frame")) and r["answers"].tolist() == [list(R.NO_ANSWER)]


def test_need2():
    from unseenobjectclustering_amd import placement
    assert placement.need2(0.05, 0.010) == 36 and placement.need2(0.051, 0.010) == 49 and placement.need2(0.0, 0.010) == 1
    assert placement.need2(0.05, 0.050) == 4 and placement.need2(0.03, 0.005) == 49 and placement.need2(0.0004, 0.001) == 1
    with pytest.raises(ValueError):
        placement.need2(-0.01, 0.01)
    packed = placement.pack_planes(*(R.flat_plane()[k] for k in ("normal", "d", "centroid", "u", "v")))
    assert packed.shape == (1, 21) and packed.dtype == np.int32
    assert R.frame_record(R.plane_from_record(packed[0])).tolist() == R.frame_record(R.flat_plane()).tolist()


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_frames_land_where_they_are_meant_to(name):
    c = R.ENGINEERED[name]()
    r = R.run_case(c)                    # asserts every point's (cell, class)
    blocking = (r["state"] == 2) | (r["state"] == 0)
    if c["G"] <= 16:
        assert np.array_equal(r["dist2"], R.edt_brute(blocking))
    if name == "empty":
        assert not r["state"].any() and not r["dist2"].any() and (r["answers"] == np.array(R.NO_ANSWER)).all()
    if name == "all_table":
        assert (r["state"] == 1).all() and r["dist2"].max() == 16 and r["dist2"][0].tolist() == [1] * 8
        assert R.contenders(r["state"], r["dist2"], c["queries"][0]) == 4 and r["answers"][:2].tolist() == [[3, 3, 16, 1], [3, 3, 16, 0]]
    if name == "single_block":
        assert (r["state"] == 2).sum() == 1 and r["owner"][5, 6] == 4 and r["counts"][4] == 1 and r["dist2"][5, 6] == 0
        a = r["answers"]
        assert a[0, 3] == 1 and a[1, 3] == 0 and a[0, 2] == a[2, 2] and a[3].tolist() == list(R.NO_ANSWER)
        for k in (5, 6):
            assert R.contenders(r["state"], r["dist2"], c["queries"][k]) >= 2
        assert len(c["queries"]) == 16
    if name == "min_pts":
        assert r["state"][4, 2:8].tolist() == [2, 0, 1, 0, 1, 2] and r["owner"][4, 2] == 7 and r["counts"][7] == 1
        assert R.run_case(c, min_pts=2)["state"][4, 2:8].tolist() == [2, 2, 1, 1, 2, 2]
    if name == "grid_edge":
        assert r["counts"][0] == 6 and (r["state"] == 1).sum() == 4
    if name == "labels":
        assert r["owner"][6, 5:7].tolist() == [1, 127] and r["owner"][6, 9] == 90 and r["state"][6, 1:5].tolist() == [1] * 4
    if name == "invalid":
        assert r["counts"][0] == 2 and r["state"][8, 8] == 1 and (r["state"] != 0).sum() == 1


def has_shadow(state):
    """An unknown cell with table cells on both sides of it in its row and in its column: a hole inside the table."""
    t = state == 1
    before_i, after_i = np.cumsum(t, axis=0) > 0, np.cumsum(t[::-1], axis=0)[::-1] > 0
    before_j, after_j = np.cumsum(t, axis=1) > 0, np.cumsum(t[:, ::-1], axis=1)[:, ::-1] > 0
    return bool(((state == 0) & before_i & after_i & before_j & after_j).any())


def test_seeded_scenes_contain_what_they_are_used_for():
    plane = R.true_plane()
    lab, xyz = scene(224, 224, 1)
    assert len(np.unique(lab)) >= 5
    G, cell, h_obs, tau, min_pts, ub = PARAMS[1]
    ev = R.point_events(lab, xyz, R.frame_record(plane), G, cell, h_obs, tau)
    assert ev["outside"].sum() > 100                                               # points outside the grid
    assert ((ev["T"] < -tau * R.S) & ev["part"] & ~ev["outside"]).sum() > 100      # the floor past the table's edge, inside the grid
    assert ((ev["cls"] == R.OBSTACLE) & (ev["id"] > 0) & (np.abs(ev["T"]) <= tau * R.S)).sum() > 20      # the flat labelled patch
    r = R.free_space(lab, xyz, plane, G, cell, h_obs, tau, min_pts, ub)
    assert all((r["state"] == s).sum() > 20 for s in (0, 1, 2)) and has_shadow(r["state"])
    assert (r["counts"][1:] > 0).sum() >= 4 and r["counts"][0] == ev["outside"].sum()
    before, after = R.atomic_events(ev, G, 256)
    assert after < before and R.atomic_events(ev, G, 64)[1] >= after
    # a widest and a nearest query with different answers, and queries decided by their tie rules
    centre = (G // 2, G // 2)
    qs = [(4, 0, 0, R.WIDEST), (4, *centre, R.NEAREST), *R.tie_queries(r["state"].astype(np.int64), r["dist2"].astype(np.int64))]
    ans = [R.answer(r["state"], r["dist2"], q) for q in qs]
    assert ans[0][3] == 1 and ans[1][3] == 1 and ans[0][:2] != ans[1][:2]
    assert all(R.contenders(r["state"], r["dist2"], q) >= 2 for q in qs[2:])
    for H, W, k in ((24, 32, 0), (61, 83, 0), (61, 83, 3), (480, 640, 1)):          # all three states at the other sizes, too
        G, cell, h_obs, tau, min_pts, ub = PARAMS[k]
        rr = R.free_space(*scene(H, W, 2), plane, G, cell, h_obs, tau, min_pts, ub)
        assert all((rr["state"] == s).any() for s in (0, 1, 2)), (H, W, G)


def test_grid_of_40_has_obstacles_and_a_segment_carry_in_its_partial_strip():
    """What tests/test_placement_gpu.py's G = 40 case is there for: columns 32..39 are the column pass's second strip, and
    a distance along a column above G / 8 rows crosses from one row segment into the next."""
    G = 40
    r = R.free_space(*scene(61, 83, 1), R.true_plane(), G, 10, 10, 10, 1, 0, [(4, 0, 0, R.WIDEST)])
    blocking = r["state"] == 2                                                      # unknown_blocks = 0
    assert blocking[:, 32:].any() and R.column_distance(blocking)[:, 32:].max() > G // 8
    assert r["answers"][0, 3] == 1
