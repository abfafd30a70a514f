"""The numpy restatement of uoc_elevation (tests/elevation_reference.py): its shifted-array level rule and separable
transform against the cell-by-cell and all-pairs ones, hand-counted grids, the engineered frames against what they are
used for, the seeded scenes against what the GPU tests use them for; the UOC_EINVAL paths of uoc_elevation through ctypes
(validation comes before any device work, the pointers are never dereferenced) and the Python wrapper's range checks.
No GPU."""
import ctypes
import functools
import types

import numpy as np
import pytest

from tests import elevation_reference as R

EINVAL = -22
FLAT = R.frame_record(R.flat_plane())
FULL = (R.BAND[0], R.BAND[1])


@functools.lru_cache(maxsize=None)
def scene(H, W, seed, nobj):
    return R.tabletop(H, W, seed, nobj=nobj)


@functools.lru_cache(maxsize=None)
def scene_heights(H, W, seed, nobj, G, cell):
    return R.heights(*scene(H, W, seed, nobj), R.frame_record(R.true_plane()), G, cell, 10, 5, 2)


def test_separable_reference_matches_all_pairs():
    rng = np.random.default_rng(11)
    for G in (8, 16):
        for density in (0.0, 0.05, 0.3, 1.0):
            for _ in range(3):
                solid = rng.random((G, G)) >= density
                owner = rng.integers(0, 3, (G, G))
                elev = rng.integers(0, 4, (G, G)) * 3
                for step in (1, 3, 6):
                    a, b = R.blocking_of(solid, owner, elev, step), R.level_brute(solid, owner, elev, step)
                    assert np.array_equal(a, b), (G, density, step)
                    assert np.array_equal(R.P.edt(a), R.P.edt_brute(b))
    # and through the whole of heights() on frames of points
    for name in ("step", "lone_point", "two_owners", "grid_edge", "two_ids"):
        c = R.ENGINEERED[name]()
        fast, slow = R.run_case(c), R.run_case(c, brute=True)
        for k in R.FIELDS:
            assert np.array_equal(fast[k], slow[k]), (name, k)


def test_hand_counted_4x4_and_staircase():
    one = np.ones((4, 4), bool)
    zero = np.zeros((4, 4), np.int64)
    blk = R.blocking_of(one, zero, zero, 5)
    assert blk.tolist() == [[True] * 4, [True, False, False, True], [True, False, False, True], [True] * 4]
    assert R.P.edt(blk).tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    own = zero.copy()
    own[1, 1] = 2                                                # another owner: it and its two inner neighbours block
    assert R.blocking_of(one, own, zero, 5)[1:3, 1:3].tolist() == [[True, True], [True, False]]
    hole = one.copy()
    hole[0, 1] = False                                           # a border cell that is not solid blocks the cell below it
    assert R.blocking_of(hole, zero, zero, 5)[1:3, 1:3].tolist() == [[True, False], [False, False]]
    # a staircase along j on 8 x 8: steps of 5, one of 6 between the columns 2 and 3
    cols = np.array([0, 5, 10, 16, 21, 26, 31, 36])
    elev = np.tile(cols, (8, 1))
    s8, z8 = np.ones((8, 8), bool), np.zeros((8, 8), np.int64)
    blk = R.blocking_of(s8, z8, elev, 5)
    assert blk[3].tolist() == [True, False, True, True, False, False, False, True]
    assert R.P.edt(blk)[3].tolist() == [0, 1, 0, 0, 1, 4, 1, 0]
    assert R.blocking_of(s8, z8, elev, 6)[1:-1, 1:-1].any() == False and R.blocking_of(s8, z8, elev, 4).all()      # noqa: E712
    tops = R.tops_of(s8, blk, z8, elev, R.P.edt(blk))
    assert tops[0].tolist() == [64, 24, 2, 5, 4, 26, 36, (6 * (5 + 21 + 26 + 31)) // 24] and tops[1].tolist() == list(R.NO_TOP)
    neg = R.tops_of(s8, blk, z8, elev - 30, R.P.edt(blk))
    assert neg[0, 7] == (6 * (5 + 21 + 26 + 31 - 120)) // 24 == -10 and neg[0, 6] == 6      # -9.25 floors to -10


def test_engineered_height_boundaries():
    r = R.run_case(R.case_height_bounds())
    assert r["elev"][3, 3:8].tolist() == [-10, R.NONE, -1, 0, 900] and r["pts"][3, 3:8].tolist() == [1, 0, 1, 1, 1]
    assert r["owner"][3, 6:8].tolist() == [2, 3] and r["info"].tolist() == [1, 0, 4, 4]
    c = R.case_height_shifted()
    cell, key, ident, _, _ = R.kept_points(c["lab"], c["xyz"], c["F"], 16, 10, 10)
    ev = R.P.point_events(c["lab"], c["xyz"], c["F"], 16, 10, 0, 10)
    assert ev["T"].reshape(-1)[:5].tolist() == [-10 * R.S - 1, -11 * R.S - 1, -R.S - 1, -1, 900 * R.S - 1]
    r = R.run_case(c)
    assert r["elev"][3, 3:8].tolist() == [R.NONE, R.NONE, -2, -1, 899]                  # T = -tau*S - 1 ignored; T = -1: hq = -1
    r = R.run_case(R.case_height_clamp())
    assert r["elev"][3, 3:8].tolist() == [32767] * 5 and R.frame_ok(R.case_height_clamp()["F"])


def test_engineered_frames_contain_what_they_are_used_for():
    r = R.run_case(R.case_two_ids())
    assert r["owner"][4, 4] == 9 and r["pts"][4, 4] == 3 and r["near"][4, 4] == 3 and r["owner"][4, 6] == 5 and r["elev"][4, 6] == 31
    r = R.run_case(R.case_step())
    assert r["elev"][7, 5:11].tolist() == [50, 55, 60, 66, 66, 66] and r["pts"][7, 5] == 3 and r["near"][7, 5] == 2
    assert r["blocking"][7, 5:11].tolist() == [True, False, True, True, False, True] and r["tops"][1, :2].tolist() == [42, 10]
    c = R.case_lone_point()
    r = R.run_case(c)
    assert r["pts"][8, 8] == 3 and r["near"][8, 8] == 1 and not r["solid"][8, 8] and r["elev"][8, 8] == 40
    assert all(r["blocking"][i, j] for i, j in ((7, 8), (9, 8), (8, 7), (8, 9))) and not r["blocking"][7, 7] and r["info"][3] == 255
    r1 = R.run_case(c, min_pts=1)
    assert r1["solid"][8, 8] and r1["blocking"][8, 8] and all(r1["blocking"][i, j] for i, j in ((7, 8), (9, 8), (8, 7), (8, 9)))
    assert r1["tops"][0, 0] == 256 and r1["tops"][0, 6] == 40
    r = R.run_case(R.case_two_owners())
    assert r["blocking"][5:11, 7:9].all() and not r["blocking"][5:11, 5:7].any() and not r["blocking"][5:11, 9:11].any()
    assert r["tops"][1].tolist() == [32, 12, 5, 5, 1, 30, 30, 30] and r["tops"][2, :4].tolist() == [32, 12, 5, 9]
    r = R.run_case(R.case_grid_edge())
    assert r["info"].tolist() == [1, 5, 64, 64] and not r["dist2"][0].any() and not r["dist2"][:, 7].any() and r["dist2"][3, 3] == 9
    assert r["answers"].tolist() == [[3, 3, 9, 1], [3, 3, 9, 1]]
    for name in ("empty", "not_found", "bad_word_0", "bad_word_3", "bad_word_10", "bad_word_13"):
        c = R.ENGINEERED[name]()
        r = R.run_case(c)
        assert (r["elev"] == R.NONE).all() and not any(r[k].any() for k in ("owner", "pts", "near", "dist2")), name
        assert (r["tops"] == np.array(R.NO_TOP)).all() and (r["answers"] == np.array(R.NO_ANSWER)).all() and len(r["answers"]), name
        assert r["info"].tolist() == ([1, 0, 0, 0] if name == "empty" else [0, 0, 0, 0])
        assert R.frame_ok(c["F"]) == (name == "empty")
    assert R.frame_ok(FLAT) and [c["name"] for c in R.bad_word_cases()] == ["bad_word_0", "bad_word_3", "bad_word_10", "bad_word_13"]
    edge = FLAT.copy()
    edge[0], edge[3], edge[10] = -32768, -(1 << 34), 32767
    assert R.frame_ok(edge)
    r = R.run_case(R.case_all_ids())
    assert (r["tops"][1:, 0] == 9).all() and (r["tops"][1:, 1] == 1).all() and (r["tops"][1:, 5] == 20 + np.arange(1, 128)).all()
    assert r["answers"].tolist() == [[53, 33, 1, 1], [28, 18, 1, 0], [3, 3, 1, 1], [0, 0, 0, 0]][:3] + [r["answers"][3].tolist()]
    assert r["answers"][3, 2] >= 1 and r["owner"][r["answers"][3, 0], r["answers"][3, 1]] == 0


def test_engineered_queries():
    c = R.case_two_plateaus()
    r = R.run_case(c)
    t3 = r["tops"][3].tolist()
    assert t3 == [50, 18, 6, 6, 4, 40, 40, 40]                   # two plateaus of 25 cells, 9 level each; the first one wins
    assert r["dist2"][6, 22] == 4 and r["tops"][7].tolist() == [9, 1, 21, 5, 1, 90, 90, 90]
    a = r["answers"].tolist()
    assert a[0] == [6, 6, 4, 1] and a[1] == [6, 6, 4, 0] and a[2] == [6, 6, 4, 1]      # need2 = dist2: 1; one above: 0; any object
    assert a[3][2] > 4 and r["owner"][a[3][0], a[3][1]] == 0      # the table is wider, and id = -1 did not answer with it
    assert a[4][3] == 1 and a[5][3] == 0 and a[4][:3] == a[5][:3] == a[3][:3]
    assert a[6] == [6, 6, 4, 1] and a[7] == list(R.NO_ANSWER) and a[8] == [21, 5, 1, 1] and a[9] == [21, 5, 1, 1]
    assert a[10] == list(R.NO_ANSWER) and a[11] == list(R.NO_ANSWER) and a[12] == list(R.NO_ANSWER)
    assert a[13] == [6, 6, 4, 1] and a[14] == [6, 6, 4, 1] and a[15] == [21, 5, 1, 0]


def test_seeded_scenes_hold_the_prototype_condition():
    for seed in (0, 1, 2):
        r = scene_heights(480, 640, seed, 5, 256, 10)
        assert (r["tops"][1:6, 1] >= 25).all(), (seed, r["tops"][:7].tolist())
        assert r["tops"][0, 4] >= 400 and r["info"][0] == 1 and r["info"][3] > 8000
        r = scene_heights(120, 160, seed, 4, 64, 20)
        assert (r["tops"][1:5, 1] >= 5).all(), (seed, r["tops"][:6].tolist())
    lab, xyz = scene(480, 640, 1, 5)
    F = R.frame_record(R.true_plane())
    before, after = R.atomic_events(lab, xyz, F, 256, 10, 10, 5, 256)
    assert after < before and R.atomic_events(lab, xyz, F, 256, 10, 10, 5, 64)[1] >= after


def test_grid_of_40_has_level_cells_in_its_partial_strip():
    """What tests/test_elevation_gpu.py's G = 40 case is there for: columns 32..39 are the column pass's second strip."""
    lab, xyz = scene(120, 160, 1, 5)
    r = R.heights(lab, xyz, R.frame_record(R.true_plane()), 40, 20, 10, 5, 1)
    assert (~r["blocking"][:, 32:]).sum() > 100 and r["dist2"][:, 32:].max() >= 25     # the reference gives 264 cells, dist2 up to 49


def test_einval_paths_and_workspace_bytes():
    from unseenobjectclustering_amd import _native
    lib = _native.lib()
    for s in ("uoc_elevation", "uoc_elevation_workspace_bytes"):
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s)
    wsb = lib.uoc_elevation_workspace_bytes
    B, H, W, G = 2, 24, 32, 16
    nws = wsb(B, H, W, G)
    assert nws > 0 and wsb(0, H, W, G) == 0 and wsb(B, 0, W, G) == 0 and wsb(B, H, -1, G) == 0 and wsb(65536, H, W, G) == 0
    assert wsb(65535, 1, 1, 8) > 0 and wsb(1, 1 << 16, 1 << 15, G) == 0 and wsb(1, (1 << 31) - 1, 1, G) > 0
    assert wsb(B, H, W, 0) == 0 and wsb(B, H, W, 12) == 0 and wsb(B, H, W, 520) == 0 and wsb(B, H, W, -8) == 0 and wsb(B, H, W, 512) > wsb(B, H, W, 8) > 0
    fake = ctypes.c_void_p(0x1000)                               # never dereferenced: validation fails before any HIP call
    names = ("lab", "xyz", "frame", "elev", "owner", "pts", "near", "dist2", "tops", "info", "answers", "ws")
    good_q = [(4, -1, FULL[0], FULL[1]), (1, 3, 0, 100)]

    def call(G_=G, cell=10, tau=10, step=5, min_pts=2, qs=good_q, Q_=None, nws_=nws, B_=B, H_=H, W_=W, drop=None, null_q=False, ws_=fake):
        hq = (ctypes.c_int32 * (4 * max(len(qs), 1)))(*[x for q in qs for x in q])
        p = {k: (None if k == drop else fake) for k in names}
        p["ws"] = None if drop == "ws" else ws_
        return lib.uoc_elevation(p["lab"], p["xyz"], p["frame"], B_, H_, W_, G_, cell, tau, step, min_pts,
                                 None if null_q else ctypes.cast(hq, ctypes.c_void_p), len(qs) if Q_ is None else Q_, p["elev"], p["owner"],
                                 p["pts"], p["near"], p["dist2"], p["tops"], p["info"], p["answers"], p["ws"], nws_, None)

    bad = [dict(drop=k) for k in names] + [
        dict(null_q=True), dict(G_=0), dict(G_=12), dict(G_=520), dict(G_=-8), dict(cell=0), dict(cell=1001), dict(tau=0), dict(tau=1001),
        dict(step=0), dict(step=1001), dict(min_pts=0), dict(min_pts=65536), dict(Q_=-1), dict(Q_=17), dict(B_=0), dict(B_=65536), dict(H_=0),
        dict(W_=-1), dict(H_=1 << 16, W_=1 << 15), dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ctypes.c_void_p(0x1008)),
        dict(ws_=ctypes.c_void_p(0x1004)), dict(qs=[(-1, 0, 0, 0)]), dict(qs=[((1 << 30) + 1, 0, 0, 0)]), dict(qs=[(1, -2, 0, 0)]),
        dict(qs=[(1, 128, 0, 0)]), dict(qs=[(1, 0, -32769, 0)]), dict(qs=[(1, 0, 32768, 0)]), dict(qs=[(1, 0, 0, -32769)]),
        dict(qs=[(1, 0, 0, 32768)]), dict(qs=[(1, 0, 0, 0), (1, 128, 0, 0)])]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    call(ws_=ctypes.c_void_p(0x1008))
    assert b"aligned" in lib.uoc_last_error()
    call(drop="frame")
    assert b"null" in lib.uoc_last_error().lower()


def test_wrapper_value_errors_and_on_top():
    import torch
    from unseenobjectclustering_amd import _native, elevation, placement
    placed = types.SimpleNamespace(grid=256, cell_mm=10, tau_mm=10, frame=None)
    lab, xyz = torch.zeros((4, 4), dtype=torch.int32), torch.zeros((3, 4, 4))
    for bad in (dict(step=0.0), dict(step=1.5), dict(step=0.0004), dict(min_pts=0), dict(min_pts=65536), dict(queries=[(1, 0, 0)]),
                dict(queries=[(-1, 0, 0, 0)]), dict(queries=[(1, 128, 0, 0)]), dict(queries=[(1, -2, 0, 0)]), dict(queries=[(1, 0, 40000, 0)]),
                dict(queries=[(1, 0, 0, -40000)]), dict(queries=[(1, 0, 0, 0)] * 17), dict(queries=[((1 << 30) + 1, 0, 0, 0)])):
        with pytest.raises(ValueError):
            elevation.heights(lab, xyz, placed, **bad)
    for over in (dict(grid=12), dict(grid=1024), dict(cell_mm=0), dict(tau_mm=1001)):
        with pytest.raises(ValueError):
            elevation.heights(lab, xyz, types.SimpleNamespace(**{**placed.__dict__, **over}))
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        elevation.heights(lab, xyz, placed)
    res = types.SimpleNamespace(cell_mm=10)
    assert elevation.on_top(res, 0.05) == (36, -1, -32768, 32767) == (placement.need2(0.05, 0.010), elevation.ANY_OBJECT, *FULL)
    assert elevation.on_top(res, 0.03, id=7, hmin=0.05, hmax=0.1205) == (16, 7, 50, 120)
    assert elevation.on_top(types.SimpleNamespace(cell_mm=20), 0.0, id=0, hmin=-0.01) == (1, 0, -10, 32767)
    for bad in (dict(id=128), dict(id=-2), dict(hmin=40.0), dict(hmax=-33.0), dict(radius=-0.01)):
        with pytest.raises(ValueError):
            elevation.on_top(res, **{"radius": 0.03, **bad})
    assert elevation.ELEV_NONE == R.NONE == -32768 and elevation.TOPS_FIELDS[5] == "elev_at" and len(elevation.INFO_FIELDS) == 4
    # cell_to_camera / spot on a synthetic result: the flat frame, cell (8, 8) of a 16-grid starts at the origin
    syn = types.SimpleNamespace(frame=torch.from_numpy(FLAT)[None], grid=16, cell_mm=10, tops=torch.zeros((1, 128, 8), dtype=torch.int32))
    assert np.allclose(elevation.cell_to_camera(syn, 0, 8, 8, 0), [0.005, -0.005, 1.0], rtol=0, atol=1e-12)
    assert np.allclose(elevation.cell_to_camera(syn, 0, 7, 9, 50), [-0.005, -0.015, 0.95], rtol=0, atol=1e-12)
    assert elevation.spot(syn, 0, 3) is None
    syn.tops[0, 3] = torch.tensor([9, 4, 7, 9, 4, 50, 52, 50], dtype=torch.int32)
    s = elevation.spot(syn, 0, 3)
    assert s.cell == (7, 9) and abs(s.clearance_m - 0.02) < 1e-12 and s.height_m == 0.05 and np.allclose(s.xyz, [-0.005, -0.015, 0.95], atol=1e-12)
    assert placement.camera_to_cell(syn, 0, s.xyz) == (7, 9)
