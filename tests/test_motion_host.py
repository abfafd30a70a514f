"""uoc_motion without a GPU: the numpy restatement (tests/motion_reference.py) on hand cases, constructed ties and
against ground truth, the rotation table and the key, motion.transform, and every error path of the C entry and of the
wrapper (they are refused before any device work)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import motion_reference as R
from unseenobjectclustering_amd import _native, motion, placement

EINVAL = -22


def run(ga, gb, A, radius, pairs, **kw):
    return R.motion(ga[0], ga[1], gb[0], gb[1], R.rotation_table(A), radius, pairs, **kw)


def fields(best):
    return dict(zip(R.BEST_FIELDS, (int(x) for x in best)))


# ---- hand cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [8, 64])
def test_l_shape_moved_is_found_at_the_centre_of_the_search(G):
    at = (0, 3) if G == 8 else (20, 30)
    ga, gb = R.l_pair(G, at, move=(3, -2))
    out = run(ga, gb, 16, 2, [(5, 5)])
    f = fields(out["best"][0])
    assert (f["status"], f["k"], f["si"], f["sj"], f["cost"]) == (1, 0, 0, 0, 0)
    assert (f["n_a"], f["n_b"], f["still"]) == (7, 7, 14 - 2 * len(set(map(tuple, (R.L_SHAPE + at).tolist())) & set(map(tuple, (R.L_SHAPE + at + (3, -2)).tolist()))))
    assert (f["pi"], f["pj"]) == (at[0] + 3, at[1]) and (f["ti"], f["tj"]) == (3, -2)         # the centroid (18/7, 3/7) rounds to (3, 0)
    assert R.key(0, 0, 0, 0, 16, 2) == 12 == (2 * 5 + 2)                                      # the key (0, 0, 0, 0, centre)
    assert out["rot"][0, 0].tolist() == [0, 0, 0, 0] and (out["rot"][0, 16:] == R.NO_ROW).all()
    assert (out["rot"][0, 1:16, 0] > 0).all()                                                 # the L has no symmetry


@pytest.mark.parametrize("turn,k", [(1, 4), (3, 12)])
def test_l_shape_quarter_turn_either_way(turn, k):
    ga, gb = R.l_pair(64, (30, 30), move=(2, 5), turn=turn)
    out = run(ga, gb, 16, 2, [(5, 5)])
    f = fields(out["best"][0])
    assert (f["status"], f["k"], f["cost"]) == (1, k, 0) and out["rot"][0, k, 0] == 0
    assert out["rot"][0, 16 - k, 0] > 0 and f["second"] > 0


# ---- constructed ties -------------------------------------------------------------------------------------------------
def test_square_and_bar_take_the_smaller_turn():
    sq = R.put(R.table(32), R.box(10, 16, 12, 18), 7)
    out = run(sq, sq, 16, 2, [(7, 7)])
    assert out["rot"][0, [0, 4, 8, 12], 0].tolist() == [0, 0, 0, 0]          # a four-fold tie on the cost ...
    f = fields(out["best"][0])
    assert (f["k"], f["si"], f["sj"], f["cost"], f["still"], f["second"]) == (0, 0, 0, 0, 0, 0)      # ... and k = 0 wins it
    bar = R.put(R.table(32), R.box(10, 16, 12, 13), 7)                       # 6 x 1: the pivot is not the centre
    out = run(bar, bar, 16, 2, [(7, 7)])
    assert out["rot"][0, 8].tolist() == [0, -1, 0, 0]                        # half a turn about the pivot and one cell back
    f = fields(out["best"][0])
    assert (f["k"], f["si"], f["sj"], f["cost"]) == (0, 0, 0, 0)             # k = 0, not A / 2
    # the same bar turned by half a turn for real, about its corner: still k = 0
    ga, gb = bar, R.put(R.table(32), R.box(5, 11, 12, 13), 7)
    f = fields(run(ga, gb, 16, 2, [(7, 7)])["best"][0])
    assert (f["k"], f["cost"], f["ti"], f["tj"]) == (0, 0, -5, 0)


# ---- the table and the key --------------------------------------------------------------------------------------------
def test_rotation_table_properties():
    for A in (1, 2, 3, 4, 5, 16, 32, 64):
        t = motion.rotation_table(A)
        assert t.dtype == np.int64 and t.shape == (A, 2) and np.array_equal(t, R.rotation_table(A))
        assert np.abs(t).max() <= R.S and t[0].tolist() == [R.S, 0]
        assert (np.abs(np.hypot(t[:, 0], t[:, 1]) - R.S) <= 1.0).all()
        for k in range(1, A):
            assert t[A - k].tolist() == [t[k, 0], -t[k, 1]]                 # the inverse rotation is in the table
    assert motion.rotation_table(4).tolist() == [[R.S, 0], [0, R.S], [-R.S, 0], [0, -R.S]]
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            motion.rotation_table(bad)
    # rd, forward and inverse: a quarter turn is exact and the inverse undoes it
    d = np.array([[3, -7], [0, 0], [-511, 511]], np.int64)
    assert R.forward(d, 0, R.S).tolist() == [[7, 3], [0, 0], [-511, -511]]
    assert R.inverse(R.forward(d, 0, R.S), 0, R.S).tolist() == d.tolist()
    assert [R.rd(x) for x in (0, R.S // 2 - 1, R.S // 2, -R.S // 2, -R.S // 2 - 1, 3 * R.S // 2)] == [0, 0, 1, 0, -1, 2]
    assert 527 * R.S < 1 << 24                                              # a product stays below 2^24


def test_key_round_trips_at_every_limit():
    for R_ in (0, 1, 16):
        for A in (1, 2, 64):
            for cost in (0, 1, 8192):
                for si in {-R_, 0, R_}:
                    for sj in {-R_, 0, R_}:
                        for k in {0, A // 2, A - 1}:
                            v = R.key(cost, si, sj, k, A, R_)
                            assert v < 1 << 63 and R.unkey(v, R_) == (cost, si * si + sj * sj, min(k, A - k), k, si, sj)
    # the order: cost, then the shift, then the turn, then k, then the shift index
    assert R.key(1, 0, 0, 0, 64, 16) > R.key(0, 16, 16, 32, 64, 16)
    assert R.key(0, 1, 0, 0, 64, 16) > R.key(0, 0, 0, 32, 64, 16)
    assert R.key(0, 0, 0, 63, 64, 16) < R.key(0, 0, 0, 2, 64, 16) and R.key(0, 0, 0, 1, 64, 16) < R.key(0, 0, 0, 63, 64, 16)
    assert R.key(0, -1, 0, 5, 64, 16) < R.key(0, 0, -1, 5, 64, 16) < R.key(0, 0, 1, 5, 64, 16) < R.key(0, 1, 0, 5, 64, 16)


def test_vector_and_scalar_counts_agree_and_targets_leave_the_grid():
    sa, oa, sb, ob = R.blobs(64, 1)
    for a, b in ((3, 3), (9, 3)):
        ca, cb = R.cells_of(sa, oa, a), R.cells_of(sb, ob, b)
        ma, mb = (sa == 2) & (oa == a), (sb == 2) & (ob == b)
        p, q = R.pivot(ca), R.pivot(cb)
        for k in (0, 3, 11):
            cx, cy = (int(x) for x in R.rotation_table(16)[k])
            c = R.costs(ca, cb, ma, mb, p, q, cx, cy, 2)
            for t, (si, sj) in enumerate(R.shifts_of(2).tolist()):
                assert c[t] == R.cost_one(ca, cb, 64, p, q, cx, cy, si, sj), (a, b, k, si, sj)
    # an object in the grid's corner: at the radius every target of some shift lies outside, and counts as a miss
    ga, gb = R.put(R.table(8), R.box(0, 2, 0, 3), 4), R.put(R.table(8), R.box(6, 8, 5, 8), 4)
    out = run(ga, gb, 8, 4, [(4, 4)])
    assert fields(out["best"][0])["cost"] == 0 and out["rot"][0, :8, 0].max() > 0
    ca, cb = R.cells_of(*ga, 4), R.cells_of(*gb, 4)
    assert R.cost_one(ca, cb, 8, R.pivot(ca), R.pivot(cb), R.S, 0, 4, 4) == 6 + 6            # every target of both masks lies outside


def test_statuses_and_membership():
    sa, oa, sb, ob = R.blobs(64, 2)
    out = R.motion(sa, oa, sb, ob, R.rotation_table(8), 1, R.BLOB_PAIRS)
    assert out["best"][:6, 0].tolist() == [1] * 6 and out["best"][6].tolist() == [2, -1] + [0] * 14
    assert (out["rot"][6] == R.NO_ROW).all()
    assert out["best"][0, 5] == ((sa == 2) & (oa == 3)).sum() and ((sa != 2) & (oa == 3)).any()      # an owner without state 2 is no cell
    big = R.put(R.table(128), R.box(0, 64, 0, 64), 1)
    assert run(big, big, 2, 0, [(1, 1)])["best"][0, :8].tolist() == [1, 0, 0, 0, 0, 4096, 4096, 0]
    more = R.put(R.put(R.table(128), R.box(0, 64, 0, 64), 1), [(100, 100)], 1)
    assert run(big, more, 2, 0, [(1, 1)])["best"][0].tolist() == [3, -1, 0, 0, 0, 4096, 4097] + [0] * 9
    f1, f2 = R.flat_frame(1), R.flat_frame(1)
    f2[5] += 1
    for fa, fb, status in ((f1, f1, 1), (f1, f2, 0), (R.flat_frame(0), R.flat_frame(0), 0), (R.flat_frame(2), R.flat_frame(2), 0)):
        o = R.motion(sa, oa, sb, ob, R.rotation_table(4), 1, [(3, 3)], fa, fb)
        assert o["best"][0, 0] == status and (status == 1 or o["best"][0].tolist() == [0, -1] + [0] * 14)


# ---- accuracy against ground truth ------------------------------------------------------------------------------------
def test_seeded_rectangles_recover_turn_and_centre():
    """Twenty rectangles, G = 64, A = 32, R = 4.  The angle, modulo half a turn, within one step; the image of the true
    centre within one cell: half a step and half a cell of quantisation plus the noise of the raster."""
    G, A, radius = 64, 32, 4
    step = 2 * np.pi / A
    worst_turn = worst_centre = 0.0
    for ca, cb, turn, centre_a, centre_b in R.ground_truth_cases(20, G):
        out = run(R.put(R.table(G), ca, 1), R.put(R.table(G), cb, 1), A, radius, [(1, 1)])
        f = fields(out["best"][0])
        assert f["status"] == 1 and len(ca) == f["n_a"] and len(cb) == f["n_b"]
        err = (f["k"] * step - turn) % np.pi
        err = min(err, np.pi - err) / step
        th = f["k"] * step
        d = centre_a - (np.array([f["pi"], f["pj"]]) + 0.5)
        image = np.array([f["qi"] + f["si"], f["qj"] + f["sj"]]) + 0.5 + np.array([d[0] * np.cos(th) - d[1] * np.sin(th), d[0] * np.sin(th) + d[1] * np.cos(th)])
        off = float(np.hypot(*(image - centre_b)))
        worst_turn, worst_centre = max(worst_turn, err), max(worst_centre, off)
        print(f"turn {turn:+.3f} k {f['k']:2d} error {err:.2f} steps, centre off {off:.2f} cells, cost {f['cost']} of {f['n_a'] + f['n_b']}")
    print(f"worst: {worst_turn:.2f} steps, {worst_centre:.2f} cells")
    assert worst_turn <= 1.0 and worst_centre <= 1.0


# ---- transform --------------------------------------------------------------------------------------------------------
def test_transform_sends_every_cell_where_the_search_did():
    """T applied to a cell's camera point lies within 0.54 cell per in-plane axis of the centre of the cell F_k sends it
    to: 0.5 from rd and below 0.032 from the rounded table over |d| < 512."""
    G, A, cell_mm = 64, 32, 10
    n = np.array([0.1, -0.6, -0.79]) / np.linalg.norm([0.1, -0.6, -0.79])
    u = np.cross(n, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    c0 = np.array([0.05, -0.02, 0.9])
    planes = placement.pack_planes(n, -float(n @ c0), c0, u, v)
    c32, u32, v32 = (np.asarray(x, np.float32).astype(np.float64) for x in (c0, u, v))
    for ca, cb, turn, _, _ in R.ground_truth_cases(4, G):
        out = run(R.put(R.table(G), ca, 1), R.put(R.table(G), cb, 1), A, 4, [(1, 1)])
        res = motion.MotionResult(rot=torch.from_numpy(out["rot"][None]), best=torch.from_numpy(out["best"][None]), table=R.rotation_table(A),
                                  pairs=np.array([[1, 1]]), angles=A, radius=4, grid=G, cell_mm=cell_mm, planes=planes)
        tr = motion.transform(res, 0, 0)
        f = fields(out["best"][0])
        assert -np.pi < tr.angle <= np.pi and abs((tr.angle - f["k"] * 2 * np.pi / A + np.pi) % (2 * np.pi) - np.pi) < 1e-12
        assert np.allclose(tr.shift_uv, (f["ti"] * 0.01, f["tj"] * 0.01)) and (tr.cost, tr.still, tr.k) == (f["cost"], f["still"], f["k"])
        assert np.allclose(tr.T[:3, :3] @ tr.T[:3, :3].T, np.eye(3), atol=1e-9) and abs(np.linalg.det(tr.T[:3, :3]) - 1) < 1e-9
        assert np.allclose(tr.T[:3, :3] @ n, n, atol=1e-6) and np.allclose(tr.T[3], [0, 0, 0, 1])
        assert np.allclose(tr.shift_xyz, f["ti"] * 0.01 * u32 + f["tj"] * 0.01 * v32, atol=1e-6)
        cx, cy = (int(x) for x in res.table[f["k"]])
        p, q, s = np.array([f["pi"], f["pj"]]), np.array([f["qi"], f["qj"]]), np.array([f["si"], f["sj"]])
        target = q + s + R.forward(ca - p, cx, cy) + 0.5
        worst = 0.0
        for c, t in zip(ca, target):
            x = placement.grid_point(c32, u32, v32, G, cell_mm, c[0] + 0.5, c[1] + 0.5)
            y = tr.T[:3, :3] @ x + tr.T[:3, 3]
            got = np.array([(y - c32) @ u32, (y - c32) @ v32]) / 0.01 + G // 2
            worst = max(worst, float(np.abs(got - t).max()))
        print(f"k {f['k']}: worst {worst:.3f} cell")
        assert worst <= 0.54
    none = motion.MotionResult(best=torch.tensor([[[2, -1] + [0] * 14]], dtype=torch.int32), angles=A, planes=planes, grid=G, cell_mm=cell_mm)
    assert motion.transform(none, 0, 0) is None


def test_moved_and_ambiguous_on_records():
    best = np.zeros((1, 5, 16), np.int32)
    best[0, 0, :5], best[0, 0, 12:15] = (1, 0, 0, 0, 0), (0, 0, 0)             # stayed, and every turn fits: a disc
    best[0, 1, :5], best[0, 1, 12:15] = (1, 0, 0, 0, 3), (1, 0, 40)            # one cell of 10 mm
    best[0, 2, :5], best[0, 2, 12:15] = (1, 31, 0, 0, 3), (0, 0, 9)            # one step back
    best[0, 3, :5], best[0, 3, 12:15] = (1, 0, 0, 0, 3), (0, 0, -1)            # stayed; no second
    best[0, 4, :2] = (2, -1)
    res = motion.MotionResult(best=torch.from_numpy(best), angles=32, cell_mm=10)
    assert motion.moved(res).tolist() == [[False, True, True, False, False]]
    assert motion.moved(res, min_shift=0.011).tolist() == [[False, False, True, False, False]]
    assert motion.moved(res, min_angle=0.3).tolist() == [[False, True, False, False, False]]
    assert motion.ambiguous(res, 6).tolist() == [[True, False, True, False, False]]
    assert motion.ambiguous(res, 5).tolist() == [[True, False, False, False, False]]


# ---- error paths ------------------------------------------------------------------------------------------------------
def test_every_einval_path_is_refused_before_device_work():
    lib = _native.lib()
    assert lib.uoc_motion_workspace_bytes(2, 64, 32, 3) >= 2 * 3 * (8 * 4 + 2 * 4096 * 4)
    for shape in ((0, 64, 32, 1), (65536, 64, 32, 1), (1, 12, 32, 1), (1, 520, 32, 1), (1, 0, 32, 1), (1, 64, 0, 1), (1, 64, 65, 1),
                  (1, 64, 32, 0), (1, 64, 32, 17)):
        assert lib.uoc_motion_workspace_bytes(*shape) == 0, shape
    B, G, A, radius, P = 2, 64, 4, 2, 2
    nws = lib.uoc_motion_workspace_bytes(B, G, A, P)
    good_rot, good_pairs = R.rotation_table(A).reshape(-1).tolist(), [1, 127, 127, 1]
    fake = lambda n: ctypes.c_void_p(4096 * n)          # noqa: E731  never dereferenced: every call below is refused first

    def call(B_=B, G_=G, rot=good_rot, A_=A, R_=radius, pairs=good_pairs, P_=P, ws=fake(9), nws_=nws, drop=(), frames=(fake(3), fake(6))):
        hr = (ctypes.c_int32 * max(len(rot), 1))(*rot)
        hp = (ctypes.c_int32 * max(len(pairs), 1))(*pairs)
        p = dict(state_a=fake(1), owner_a=fake(2), frame_a=frames[0], state_b=fake(4), owner_b=fake(5), frame_b=frames[1],
                 rot=ctypes.cast(hr, ctypes.c_void_p), pairs=ctypes.cast(hp, ctypes.c_void_p), out_rot=fake(7), out_best=fake(8), ws=ws)
        for k in drop:
            p[k] = None
        return lib.uoc_motion(p["state_a"], p["owner_a"], p["frame_a"], p["state_b"], p["owner_b"], p["frame_b"], B_, G_, p["rot"], A_, R_,
                              p["pairs"], P_, p["out_rot"], p["out_best"], p["ws"], nws_, None)

    over = [R.S, -R.S] * A
    cases = [dict(drop=(k,)) for k in ("state_a", "owner_a", "state_b", "owner_b", "rot", "pairs", "out_rot", "out_best", "ws", "frame_a", "frame_b")] + [
        dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(A_=0), dict(A_=65), dict(R_=-1), dict(R_=17),
        dict(P_=0), dict(P_=17), dict(rot=over[:-1] + [-R.S - 1]), dict(rot=[R.S + 1] + over[1:]), dict(pairs=[0, 1, 1, 1]), dict(pairs=[1, 1, 1, 128]),
        dict(pairs=[1, -3, 1, 1]), dict(nws_=nws - 1), dict(nws_=0), dict(ws=ctypes.c_void_p(4096 * 9 + 4))]
    for kw in cases:
        assert call(**kw) == EINVAL, kw
        assert b"uoc_motion" in lib.uoc_last_error(), kw
    assert b"aligned" in lib.uoc_last_error()


def test_wrapper_refuses_bad_arguments():
    z = torch.zeros((1, 8, 8), dtype=torch.int32)
    with pytest.raises(_native.NativeError):
        motion.motion_records(z, z, None, z, z, None, R.rotation_table(4), 1, [(1, 1)])          # no CPU fallback
    for bad in ([], [(1, 1)] * 17, [(0, 1)], [(1, 128)], [(1, 2, 3)], 5):
        with pytest.raises(ValueError):
            motion._check_pairs(bad)
    assert motion._check_pairs((3, 4)).tolist() == [[3, 4]] and motion.same_ids([2, 9]) == [(2, 2), (9, 9)]
    a = placement.PlacementResult(state=z, owner=z, grid=8, cell_mm=10)
    for other in (placement.PlacementResult(state=z, owner=z, grid=8, cell_mm=20), placement.PlacementResult(state=z[:, :, :4], owner=z, grid=8, cell_mm=10)):
        with pytest.raises(ValueError):
            motion.register(a, other, [(1, 1)])
    for kw in (dict(angles=0), dict(angles=65), dict(pairs="all"), dict(pairs=[(1, 200)])):
        with pytest.raises(ValueError):
            motion.register(a, a, **{**dict(pairs=[(1, 1)]), **kw})
    for kw in (dict(angles=65), dict(radius=17), dict(radius=-1)):
        with pytest.raises(ValueError):
            motion.Follower(None, **kw)
