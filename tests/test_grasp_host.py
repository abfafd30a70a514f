"""The numpy restatement of uoc_grasp (tests/grasp_reference.py) against hand-counted grids: an 8x8 grid whose every code is
written out, the 64x64 scene with its counts per object, the key order on constructed ties, the floor of a negative
coordinate, that the engineered grids of the GPU tests contain what they are used for; and the host side of the package:
the millimetre-to-cell conversion, the direction table and pose() on a synthetic result.  No GPU.

The scene's counts are those of the first prototype of the stage.  The definition differs from that prototype in one
place: an UNKNOWN sample between the fingers does not make a candidate PINCHED (only OTHER and OUT do).  The scene has no
unknown cell, so no count changed."""
import numpy as np
import pytest
import torch

from tests import grasp_reference as R

S = 16384
DIRS16 = R.direction_table(16)


def both(st, ow, dirs, **kw):
    """The restatement, held against the sample-by-sample definition."""
    r, q = R.grasp(st, ow, dirs, **kw), R.grasp_literal(st, ow, dirs, **kw)
    assert np.array_equal(r["cand"], q["cand"]) and np.array_equal(r["best"], q["best"])
    assert r["cand"].dtype == np.int32 and r["best"].dtype == np.int32
    return r


def test_hand_counted_8x8():
    # the box covers rows 3..4, columns 2..5: 8 cells, sum i = 28, sum j = 28, anchor (4 S, 4 S), a cell corner.
    # k = 0 closes along i: line l is column 4 + l, the box spans i = 3, 4, that is t = -1, 0
    # k = 1 closes along j: line l is row 4 - l, the box spans j = 2..5, that is t = -2..1; row 5 (l = -1) misses it
    st, ow = R.box8()
    d = R.direction_table(2)
    assert d.tolist() == [[S, 0], [0, S]]
    r = both(st, ow, d, M=1, Wmax=4, gap=0, F=1, Hp=0, unknown_blocks=1)
    assert r["cand"][1].tolist() == [[[2, -1], [2, -1], [2, -1]], [[-1, 0], [4, -2], [4, -2]]]
    assert r["best"][1].tolist() == [1, 0, 0, -1, 2, 4 * S, 4 * S, 5]              # m = 0 first, then the narrower: k = 0
    assert not r["cand"][0].any() and not r["cand"][2:].any() and not r["best"][0].any() and not r["best"][2:].any()
    r = both(st, ow, d, M=1, Wmax=3, gap=0, F=1, Hp=0, unknown_blocks=1)             # 4 cells do not fit an opening of 3
    assert r["cand"][1].tolist() == [[[2, -1], [2, -1], [2, -1]], [[-1, 0], [-2, -2], [-2, -2]]]
    assert r["best"][1].tolist() == [1, 0, 0, -1, 2, 4 * S, 4 * S, 3]
    r = both(st, ow, d, M=1, Wmax=4, gap=1, F=2, Hp=0, unknown_blocks=1)             # the finger zone j = -1..1 leaves the grid
    assert r["cand"][1].tolist() == [[[2, -1], [2, -1], [2, -1]], [[-1, 0], [-4, -2], [-4, -2]]]
    r = both(st, ow, d, M=1, Wmax=1, gap=0, F=1, Hp=0, unknown_blocks=1)
    assert r["cand"][1, :, :, 0].tolist() == [[-2, -2, -2], [-1, -2, -2]] and r["best"][1].tolist() == [0, -1, 0, 0, 0, 4 * S, 4 * S, 0]
    r = both(st, ow, d, M=1, Wmax=4, gap=0, F=1, Hp=1, unknown_blocks=1)             # pads of 3 lines: every strip meets the box
    assert r["cand"][1].tolist() == [[[2, -1], [2, -1], [2, -1]], [[4, -2], [4, -2], [4, -2]]]      # column 6, rows 2, 5, 6: table
    assert r["best"][1].tolist() == [1, 0, 0, -1, 2, 4 * S, 4 * S, 6]


def test_scene64_counts():
    st, ow = R.scene64()
    r = both(st, ow, DIRS16, **R.DEFAULT)
    want = {1: {"ok": 39, R.WIDE: 41}, 2: {"ok": 80}, 3: {R.WIDE: 80}, 4: {"ok": 21, R.PINCHED: 44, R.BLOCKED: 15},
            5: {"ok": 22, R.PINCHED: 43, R.BLOCKED: 15}, 6: {"ok": 37, R.WIDE: 43}}
    for a, w in want.items():
        counts = R.code_counts(r["cand"][a])
        assert counts == {**{"ok": 0, R.MISS: 0, R.WIDE: 0, R.PINCHED: 0, R.BLOCKED: 0}, **w}, (a, counts)
        assert r["best"][a, 7] == w.get("ok", 0) and r["best"][a, 0] == (1 if w.get("ok") else 0)
    assert r["best"][1, 1:5].tolist()[:2] == [10, 0] and r["best"][1, 4] == 5           # across the box: 120 degrees, 5 cells
    assert r["best"][2, 4] == 6 and r["best"][3].tolist()[:5] == [0, -1, 0, 0, 0]
    assert not r["best"][7:].any() and not r["cand"][7:].any()


def test_key_order_on_constructed_ties():
    kw = dict(M=1, Wmax=4, gap=0, F=1, Hp=0, unknown_blocks=1)
    # +m before -m: the box of box8 and one direction (along i); a cell of id 2 under the finger of m = 0
    st, ow = R.box8()
    st[5, 4], ow[5, 4] = 2, 2
    r = both(st, ow, R.direction_table(1), **kw)
    assert r["cand"][1, 0].tolist() == [[2, -1], [-4, -1], [2, -1]] and r["best"][1].tolist() == [1, 0, 1, -1, 2, 4 * S, 4 * S, 2]
    # the lower k: a 2x2 box is 2 wide along both directions
    st, ow = R.table(8)
    st[3:5, 3:5], ow[3:5, 3:5] = 2, 1
    r = both(st, ow, R.direction_table(2), **{**kw, "M": 0})
    assert r["cand"][1, :, 0].tolist() == [[2, -1], [2, -1]] and r["best"][1, :5].tolist() == [1, 0, 0, -1, 2]
    # the narrower w before the lower k: box8 turned by a quarter is 4 wide along k = 0 and 2 wide along k = 1
    st, ow = R.table(8)
    st[2:6, 3:5], ow[2:6, 3:5] = 2, 1
    r = both(st, ow, R.direction_table(2), **{**kw, "M": 0})
    assert r["cand"][1, :, 0].tolist() == [[4, -2], [2, -1]] and r["best"][1, :5].tolist() == [1, 1, 0, -1, 2]
    # the key itself: a strict total order over (k, m), the fields do not overlap at the limits
    keys = {R.key_of(k, m, w, 32, 8, 64) for k in range(32) for m in range(-8, 9) for w in (1, 64)}
    assert len(keys) == 32 * 17 * 2 and min(keys) >= 1 and max(keys) < 1 << 32
    assert R.key_of(0, 1, 2, 2, 1, 4) > R.key_of(0, -1, 2, 2, 1, 4) > R.key_of(1, 1, 2, 2, 1, 4)
    assert R.key_of(1, 0, 2, 2, 1, 4) > R.key_of(0, 0, 3, 2, 1, 4) > R.key_of(0, 1, 1, 2, 1, 4)


def test_floor_of_negative_coordinates():
    st, ow = R.table(8)
    st[0, 0], ow[0, 0] = 2, 1                                  # anchor (S/2, S/2); t = -1 gives X = -S/2: cell -1, not cell 0
    cls = R.classes(st, ow, 1, np.array([-S // 2, -1, 0, S - 1, S]), np.array([S // 2] * 5), 1)
    assert cls.tolist() == [R.OUT, R.OUT, R.OWN, R.OWN, R.FREE]
    r = both(st, ow, R.direction_table(1), M=0, Wmax=2, gap=0, F=1, Hp=0, unknown_blocks=1)
    assert r["best"][1, 5:7].tolist() == [S // 2, S // 2]
    assert r["cand"][1, 0, 0].tolist() == [R.BLOCKED, 0]       # truncation towards zero would give WIDE or tlo = -1
    st, ow = R.table(8)
    st[0, 3], ow[0, 3] = 2, 1
    r = both(st, ow, R.direction_table(2), M=0, Wmax=2, gap=0, F=1, Hp=0, unknown_blocks=1)
    assert r["cand"][1, :, 0].tolist() == [[R.BLOCKED, 0], [1, 0]]


def test_engineered_grids_contain_what_they_are_used_for():
    codes = lambda r, a: set(r["cand"][a, ..., 0].reshape(-1).tolist())
    r = both(*R.case_border(), DIRS16, **R.DEFAULT)
    assert R.BLOCKED in codes(r, 1) and R.PINCHED in codes(r, 2)
    r = both(*R.case_border(), R.direction_table(2), M=0, Wmax=8, gap=0, F=1, Hp=1, unknown_blocks=1)
    assert r["cand"][2, 1, 0].tolist() == [R.PINCHED, -2]         # along the bar: the pad's line in row 16 is outside the grid
    r = both(*R.case_border(), R.direction_table(2), M=0, Wmax=8, gap=0, F=1, Hp=0, unknown_blocks=1)
    assert r["cand"][2, :, 0].tolist() == [[R.BLOCKED, 0], [4, -2]]  # across it: the finger at i = 16 is outside
    kw = dict(M=0, Wmax=8, gap=1, F=1, Hp=0, unknown_blocks=1)
    r = both(*R.case_widths(8), R.direction_table(2), **kw)
    assert r["cand"][1, 1, 0].tolist() == [8, -4] and r["cand"][2, 1, 0, 0] == R.WIDE and r["cand"][2, 0, 0, 0] == 2
    r = both(*R.case_far_fingers(), R.direction_table(2), M=0, Wmax=8, gap=1, F=2, Hp=0, unknown_blocks=1)
    assert r["cand"][1, 1, 0].tolist() == [R.WIDE, -8]                                  # 17 wide: t = -8..8
    r = both(*R.case_far_fingers(), R.direction_table(2), M=0, Wmax=17, gap=0, F=1, Hp=0, unknown_blocks=1)
    assert r["cand"][1, 1, 0].tolist() == [17, -8]                                      # the cell of id 2 at t = 10 is out of reach
    r = both(*R.case_far_fingers(), R.direction_table(2), M=0, Wmax=17, gap=1, F=1, Hp=0, unknown_blocks=1)
    assert r["cand"][1, 1, 0].tolist() == [R.BLOCKED, -8]
    # finger zones beyond the search range: Wmax = 1 gives R = 2, gap + F = 12 zones at t = -12..-1 and 1..12
    far = dict(M=0, Wmax=1, gap=4, F=8, Hp=0)
    st, ow = R.case_beyond_range()
    r = both(st, ow, R.direction_table(2), **far, unknown_blocks=1)
    assert r["cand"][1].tolist() == [[[R.BLOCKED, 0]], [[R.BLOCKED, 0]]]                # unknown at t = -11 along i, id 2 at t = 6 along j
    r = both(st, ow, R.direction_table(2), **far, unknown_blocks=0)
    assert r["cand"][1].tolist() == [[[1, 0]], [[R.BLOCKED, 0]]] and r["best"][1].tolist() == [1, 0, 0, 0, 1, 16 * S + S // 2, 16 * S + S // 2, 1]
    r = both(st, ow, R.direction_table(2), **{**far, "F": 6}, unknown_blocks=1)          # zones to t = 10: the unknown cell is out of reach
    assert r["cand"][1].tolist() == [[[1, 0]], [[R.BLOCKED, 0]]]
    r = both(st, ow, R.direction_table(2), **{**far, "gap": 1, "F": 4}, unknown_blocks=1)  # zones to t = 5: id 2 is out of reach too
    assert r["cand"][1].tolist() == [[[1, 0]], [[1, 0]]]
    r = both(st, ow, R.direction_table(2), **{**far, "Wmax": 2}, unknown_blocks=1)       # the bar: R = 4, state 3 at t = 11 along j
    assert r["cand"][3].tolist() == [[[R.BLOCKED, 0]], [[R.BLOCKED, -1]]]                # along i the zone leaves the grid at i = 32
    st[16, 22], ow[16, 22], st[26, 25] = 1, 0, 1                                        # the two obstacles removed
    r = both(st, ow, R.direction_table(2), **far, unknown_blocks=0)
    assert r["cand"][1].tolist() == [[[1, 0]], [[1, 0]]] and r["best"][1, :5].tolist() == [1, 0, 0, 0, 1] and r["best"][1, 7] == 2
    r = both(st, ow, R.direction_table(2), **{**far, "Wmax": 2}, unknown_blocks=1)
    assert r["cand"][3].tolist() == [[[R.BLOCKED, 0]], [[2, -1]]] and r["best"][3].tolist() == [1, 1, 0, -1, 2, 26 * S + S // 2, 14 * S, 1]
    r = both(*R.case_single_cells(), DIRS16, **R.DEFAULT)
    assert r["best"][5, :5].tolist() == [1, 0, 0, 0, 1] and R.MISS in codes(r, 5) and r["best"][127, 0] == 1 and r["best"][1, 0] == 0
    r = R.grasp(*R.case_all_ids(), R.direction_table(4), **R.DEFAULT)
    assert (r["best"][1:, 5] > 0).all() and not r["best"][0].any()
    r = both(*R.case_empty(), DIRS16, **R.DEFAULT)
    assert not r["cand"].any() and not r["best"].any()
    r = both(*R.case_all_obstacle(), R.direction_table(4), **R.DEFAULT)
    assert codes(r, 3) <= {R.WIDE, R.PINCHED, R.BLOCKED} and r["best"][3, 0] == 0 and r["best"][3, 5] > 0
    for ub in (0, 1):
        r = both(*R.case_out_of_contract(), R.direction_table(2), M=0, Wmax=4, gap=0, F=1, Hp=0, unknown_blocks=ub)
        assert r["best"][7, 5:7].tolist() == [11 * S, 11 * S + S // 2]                  # six cells: the strays are not the object's
        assert r["cand"][7, 1, 0].tolist() == [3, -1]                                   # row 11, j = 10..12: (11, 8) owner 128 is out of reach
        assert not r["best"][[0] + list(range(8, 128))].any()
    r = both(*R.case_out_of_contract(), R.direction_table(2), M=0, Wmax=4, gap=1, F=1, Hp=0, unknown_blocks=0)
    assert r["cand"][7, 1, 0].tolist() == [R.BLOCKED, -1]                               # (11, 8): state 2, owner 128: unknown, not free
    r = both(*R.case_ring(), DIRS16, M=2, Wmax=24, gap=1, F=1, Hp=1, unknown_blocks=1)
    st, ow = R.case_ring()
    assert ow[r["best"][1, 5] >> 14, r["best"][1, 6] >> 14] == 2 and codes(r, 1) == {R.PINCHED} and r["best"][2, 0] == 1


def test_random_grids_hold_every_class():
    st, ow = R.random_grid(64, 1)
    assert {0, 1, 2, 3} <= set(np.unique(st).tolist()) and ow.min() < 0 and ow.max() > 127
    r = both(st, ow, R.direction_table(5), **R.DEFAULT)
    assert (r["best"][:, 7] > 0).any()
    seen = set()
    for seed in range(1, 5):
        seen |= set(R.grasp(*R.random_grid(64, seed), R.direction_table(5), **R.DEFAULT)["cand"][..., 0].reshape(-1).tolist())
    assert {R.MISS, R.WIDE, R.PINCHED, R.BLOCKED} <= seen and max(seen) > 0


def test_millimetres_to_cells():
    from unseenobjectclustering_amd import grasp
    assert grasp.cells_from_metres(10, 0.085, 0.005, 0.010, 0.020) == (8, 1, 1, 1)      # the defaults on 1 cm cells
    assert grasp.cells_from_metres(5, 0.085, 0.005, 0.010, 0.020) == (17, 1, 2, 2)
    assert grasp.cells_from_metres(20, 0.085, 0.005, 0.010, 0.020) == (4, 1, 1, 0)
    assert grasp.cells_from_metres(10, 0.089, 0.0, 0.011, 0.039) == (8, 0, 2, 1)        # floor, ceil, ceil, floor
    assert grasp.cells_from_metres(10, 0.64, 0.04, 0.08, 0.08) == (64, 4, 8, 4)         # the limits
    for bad, word in ((dict(max_open=0.005), "max_open"), (dict(max_open=0.65), "max_open"), (dict(gap=0.041), "gap"),
                      (dict(finger=0.0), "finger"), (dict(finger=0.081), "finger"), (dict(pad=0.1), "pad"), (dict(gap=-0.01), "gap")):
        kw = {**dict(max_open=0.085, gap=0.005, finger=0.010, pad=0.020), **bad}
        with pytest.raises(ValueError, match=word):
            grasp.cells_from_metres(10, **kw)
    assert (grasp.MISS, grasp.WIDE, grasp.PINCHED, grasp.BLOCKED) == (R.MISS, R.WIDE, R.PINCHED, R.BLOCKED)


def test_direction_table():
    from unseenobjectclustering_amd import grasp
    assert grasp.direction_table(1).tolist() == [[S, 0]] and grasp.direction_table(2).tolist() == [[S, 0], [0, S]]
    for A in (1, 2, 16, 32):
        d = grasp.direction_table(A)
        assert d.dtype == np.int32 and d.shape == (A, 2) and np.array_equal(d, R.direction_table(A)) and np.abs(d).max() <= S
        assert (np.abs(np.hypot(d[:, 0], d[:, 1]) - S) < 1).all() and (d[:, 1] >= 0).all()
    assert grasp.direction_table(16)[[4, 8, 12]].tolist() == [[11585, 11585], [0, S], [-11585, 11585]]
    assert grasp.direction_table(32)[[1, 16]].tolist() == [[16305, 1606], [0, S]]
    for bad in (0, 33):
        with pytest.raises(ValueError):
            grasp.direction_table(bad)


def test_pose_on_a_synthetic_result():
    from unseenobjectclustering_amd import grasp, placement
    n = np.array([0.1, -0.3, -1.0])
    n /= np.linalg.norm(n)
    u = np.cross(n, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    c = np.array([0.02, -0.05, 0.9])
    planes = torch.from_numpy(placement.pack_planes(n, -float(n @ c), c, u, v))
    G, M, A = 64, 2, 16
    best = torch.zeros((1, 128, 8), dtype=torch.int32)
    cand = torch.zeros((1, 128, A, 2 * M + 1, 2), dtype=torch.int32)
    best[0, 3] = torch.tensor([1, 4, -1, -2, 5, 40 * S + 100, 20 * S + S // 2, 7])
    cand[0, 3, 4, M - 1] = torch.tensor([5, -2])
    cand[0, 3, 8, M + 2] = torch.tensor([3, -1])
    cand[0, 3, 0, M] = torch.tensor([R.BLOCKED, -1])
    best[0, 9] = torch.tensor([0, -1, 0, 0, 0, 5 * S, 5 * S, 0])
    res = grasp.GraspResult(cand=cand, best=best, dirs=grasp.direction_table(A), angles=A, offsets=M, max_open=8, gap=1, finger=1, pad=1,
                            unknown_blocks=True, grid=G, cell_mm=10, planes=planes)
    assert grasp.graspable(res)[0].nonzero().reshape(-1).tolist() == [3]
    assert grasp.pose(res, 0, 9) is None and grasp.pose(res, 0, 1) is None and grasp.pose(res, 0, 3, k=0, m=0) is None
    p = grasp.pose(res, 0, 3)
    n32, u32, v32, c32 = (np.asarray(x, np.float32).astype(np.float64) for x in (n, u, v, c))
    assert abs(np.linalg.norm(p.axis) - 1) < 1e-6 and abs(p.axis @ n32) < 1e-6 and (p.k, p.m) == (4, -1)
    assert abs(p.width_m - 0.05) < 1e-12 and abs(p.opening_m - 0.07) < 1e-12
    cx, cy = 11585.0, 11585.0                                   # k = 4 of 16: 45 degrees; the middle of t = -2..2 is t = 0, l = -1
    X, Y = 40 * S + 100 + cy, 20 * S + S // 2 - cx
    want = c32 + (X / S - 32) * 0.01 * u32 + (Y / S - 32) * 0.01 * v32
    assert np.allclose(p.center, want, rtol=0, atol=1e-9) and abs(p.center @ n32 - n32 @ c32) < 1e-6
    assert np.allclose(p.axis, (u32 + v32) / np.sqrt(2), rtol=0, atol=1e-6)
    q = grasp.pose(res, 0, 3, k=8, m=2)                         # closes along v; the middle of t = -1..1 is t = 0, l = 2: X - 2 S
    assert np.allclose(q.axis, v32, rtol=0, atol=1e-6) and abs(q.width_m - 0.03) < 1e-12 and (q.k, q.m) == (8, 2)
    assert np.allclose(q.center, c32 + ((40 * S + 100 - 2 * S) / S - 32) * 0.01 * u32 + ((20 * S + S // 2) / S - 32) * 0.01 * v32, rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        grasp.pose(res, 0, 3, k=1)
    with pytest.raises(ValueError):
        grasp.pose(res, 0, 3, k=16, m=0)
