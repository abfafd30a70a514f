"""The routes stage on the CPU: the numpy restatement (tests/routes_reference.py) against hand-counted cases, its two
forms of PASSABLE against each other and against the placement stage's clearance, the rules of the definition one at a
time, the grids the GPU tests rely on, and the argument validation of uoc_routes and of the Python wrapper (validation
comes before any device work, so it runs without a GPU)."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from tests import placement_reference as PR
from tests import routes_reference as R
from unseenobjectclustering_amd import _native, placement, routes

EINVAL = -22


def test_hand_counted_8x8():
    st, ow = R.hand8()
    out = R.routes(st, ow, [R.record(0, (2, 2), (7, 7)), R.record(0, (2, 2), (2, 5)), R.record(0, (2, 2))], 1, 16)
    c = out["cost"][0]
    assert (c[2, 2], c[2, 3], c[6, 3], c[6, 4], c[7, 5], c[7, 7], c[6, 5], c[2, 5]) == (0, 5, 22, 27, 34, 44, 32, 52)
    assert (c[:6, 4] == -1).all() and (c >= 0).sum() == 58
    assert out["info"][0].tolist() == [1, 1, 7, 7, 44, 8, 58, 58] and out["info"][1].tolist() == [1, 1, 2, 5, 52, 10, 58, 58]
    assert out["path"][0, :9].tolist() == [[7, 7], [7, 6], [7, 5], [7, 4], [6, 3], [5, 3], [4, 3], [3, 3], [2, 2]]
    assert (out["path"][0, 9:] == -1).all() and (out["path"][2] == -1).all()
    assert out["info"][2].tolist() == [1, 0, -1, -1, 0, 0, 58, 58] and np.array_equal(out["cost"][2], c)


def test_span_form_of_passable_matches_all_offsets():
    for G in (8, 16, 24, 64):
        for seed in (1, 2):
            st, ow = R.random_grid(G, seed)
            P = R.present_id(ow, st)
            for ub in (0, 1):
                for ignore in (0, P):
                    free = R.free_cells(st, ow, ignore, ub)
                    for need2 in (0, 1, 2, 3, 4, 5, 9, 10, 25, 26, 50, 4096 if G == 64 else 100):
                        a, b = R.passable(free, need2), R.passable_spans(free, need2)
                        assert np.array_equal(a, b), (G, seed, ub, ignore, need2)
    free = np.ones((64, 64), bool)                              # the largest disc: 63 cells to every side
    assert not R.passable(free, 4096).any() and not R.passable_spans(free, 4096).any()
    free = np.ones((128, 128), bool)
    a = R.passable(free, 4096)
    assert np.array_equal(a, R.passable_spans(free, 4096)) and a.sum() == 2 * 2 and a[63, 63] and a[64, 64]
    assert R.disc_spans(4096)[0] == 63 and R.disc_spans(4096)[63] == 11 and 64 not in R.disc_spans(4096)
    assert R.disc_offsets(0) == [] and R.disc_offsets(1) == [(0, 0)] and len(R.disc_offsets(2)) == 5 and len(R.disc_offsets(4)) == 9


def test_passable_is_the_placement_clearance_without_ignore():
    for G in (8, 16, 64):
        for seed in (1, 2, 3):
            st, ow = R.random_grid(G, seed)
            for ub in (0, 1):
                free = R.free_cells(st, ow, 0, ub)
                d2 = PR.edt(~free)                              # §15 E on the blocking cells
                if G <= 16:
                    assert np.array_equal(d2, PR.edt_brute(~free))
                for need2 in (0, 1, 2, 4, 5, 9, 16, 17, 64):
                    assert np.array_equal(R.passable(free, need2), free & (d2 >= need2)), (G, seed, ub, need2)


def test_no_corner_cutting_on_a_checker():
    st, ow = R.table(8)
    st[3, 4], ow[3, 4] = 2, 3
    st[4, 3], ow[4, 3] = 2, 3                                   # (3,3) and (4,4) table, (3,4) and (4,3) obstacle
    pas = R.free_cells(st, ow, 0, 1)
    assert not R.move_allowed(pas, (3, 3), 7) and not R.move_allowed(pas, (4, 4), 4)
    c = R.dijkstra(pas, (3, 3))
    assert c[4, 4] == 30 == min(c[4, 5], c[5, 4]) + 5           # six orthogonal moves around an obstacle, never across the corner
    st[3, 4], ow[3, 4] = 1, 0                                   # one of the two is enough to forbid the move
    pas = R.free_cells(st, ow, 0, 1)
    assert not R.move_allowed(pas, (3, 3), 7) and R.dijkstra(pas, (3, 3))[4, 4] == 10
    st[4, 3], ow[4, 3] = 1, 0
    assert R.dijkstra(R.free_cells(st, ow, 0, 1), (3, 3))[4, 4] == 7
    # the chink of the GPU tests: the halves are connected by nothing but the forbidden move
    st, ow = R.chink()
    pas = R.free_cells(st, ow, 0, 1)
    c = R.dijkstra(pas, (8, 8))
    assert pas[8, 8] and pas[7, 9] and c[7, 9] == -1 and (c >= 0).sum() == 136
    open_ = pas.copy()
    open_[7, 8] = True
    assert R.dijkstra(open_, (8, 8))[7, 9] == 10


def test_closest_approach_ties():
    G = 16
    cost = np.full((G, G), -1, np.int32)
    # first level: two cells equally near the target (da = 4), the cheaper one wins whatever its index
    cost[5, 7], cost[9, 7] = 40, 30
    assert R.closest(cost, (7, 7)) == (9, 7)
    cost[9, 7] = 50
    assert R.closest(cost, (7, 7)) == (5, 7)
    # second level: equally near and equally dear: the lowest index
    cost[9, 7], cost[7, 5], cost[7, 9] = 40, 40, 40
    assert R.closest(cost, (7, 7)) == (5, 7)
    cost[5, 7] = -1
    assert R.closest(cost, (7, 7)) == (7, 5)
    cost[8, 8] = 2000                                           # nearer beats cheaper
    assert R.closest(cost, (7, 7)) == (8, 8)
    # the key's fields do not run into each other at the limits
    assert R.key_of(0, 0, 0) > R.key_of(0, 0, 1) > R.key_of(0, 1, 0) > R.key_of(1, 0, 0) > 0
    assert R.key_of(2 * 511 ** 2, 7 * 512 * 512, 512 * 512 - 1) > 0 and R.key_of(0, 0, 0) < 1 << 64
    # on a grid: a walled target, two reached cells tie in da and the cheaper is taken
    st, ow = R.walled_target()
    out = R.routes(st, ow, [R.record(0, (8, 2), (8, 13))], 1, 32)
    assert out["info"][0].tolist()[:6] == [1, 0, 8, 9, 35, 7]


def test_backtrack_takes_the_first_neighbour_in_order():
    st, ow = R.table(8)
    out = R.routes(st, ow, [R.record(0, (2, 2), (4, 5)), R.record(0, (2, 2), (5, 4)), R.record(0, (5, 4), (2, 2))], 1, 8)
    c = out["cost"][0]
    # (4,5) from (2,2): two diagonals and one orthogonal move in any order, 19.  Back from (4,5): (-1,0) -> (3,5) = 17 is
    # no predecessor; (0,-1) -> (4,4) = 14 and (-1,-1) -> (3,4) = 12 both are, two paths of equal cost: the order takes
    # (0,-1).  Back from (5,4): (-1,0) -> (4,4) comes before (-1,-1) -> (4,3).
    assert (c[4, 5], c[3, 5], c[4, 4], c[3, 4], c[4, 3]) == (19, 17, 14, 12, 12)
    assert out["info"][0].tolist()[:6] == [1, 1, 4, 5, 19, 3] and out["info"][1].tolist()[:6] == [1, 1, 5, 4, 19, 3]
    assert out["path"][0, :5].tolist() == [[4, 5], [4, 4], [3, 3], [2, 2], [-1, -1]]
    assert out["path"][1, :5].tolist() == [[5, 4], [4, 4], [3, 3], [2, 2], [-1, -1]]
    assert out["path"][2, :5].tolist() == [[2, 2], [3, 2], [4, 3], [5, 4], [-1, -1]]      # (1,0) before (1,1)
    for q in range(3):                                          # every step is the first predecessor in MOVES' order
        cq = out["cost"][q]
        cells = [tuple(x) for x in out["path"][q, :4].tolist()]
        for a, b in zip(cells, cells[1:]):
            pred = [k for k, (di, dj) in enumerate(R.MOVES) if 0 <= a[0] + di < 8 and 0 <= a[1] + dj < 8 and
                    cq[a[0] + di, a[1] + dj] + R.COST[k] == cq[a]]
            assert R.MOVES[pred[0]] == (b[0] - a[0], b[1] - a[1]) and (len(pred) > 1 or cells.index(a) > 0)


def test_chamfer_bounds_on_an_empty_grid():
    G = 64
    st, ow = R.table(G)
    c = R.dijkstra(R.free_cells(st, ow, 0, 1), (0, 0)).astype(np.float64)
    I, J = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    a, b = np.maximum(I, J), np.minimum(I, J)
    assert np.array_equal(c, 5.0 * (a - b) + 7.0 * b)           # b diagonal moves and a - b orthogonal ones
    e = np.hypot(I, J)
    ratio = (c / 5.0)[e > 0] / e[e > 0]
    lo, hi = ratio.min(), ratio.max()
    print("chamfer ratio on 64x64: min %.6f max %.6f" % (lo, hi))
    # 5a + 2b against 5 sqrt(a^2 + b^2), 0 <= b <= a: the minimum 7 / (5 sqrt 2) = 0.98995 on the diagonal, the maximum
    # sqrt(29) / 5 = 1.07703 at b / a = 2 / 5 (the derivative's zero); rounded outwards as the definition states them
    assert 7 / (5 * math.sqrt(2)) - 1e-12 <= lo and hi <= math.sqrt(29) / 5 + 1e-12
    assert 0.98995 <= lo + 1e-5 and hi <= 1.07704
    assert abs(lo - 0.98995) < 1e-5 and abs(hi - 1.07703) < 1e-5          # both are attained on this grid: (k, k) and (5k, 2k)


def test_serpentines_are_what_the_gpu_tests_need():
    for G in (8, 64, 256):
        st, ow = R.serpentine(G)
        end, want = R.serpentine_end(G)
        pas = R.free_cells(st, ow, 0, 1)
        assert pas[0, 0] and pas[end] and pas.sum() == (G // 2) * G + G // 2
        if G < 256:
            assert R.dijkstra(pas, (0, 0))[end] == want
    out = R.routes(*R.serpentine(256), [R.record(0, (0, 0), R.serpentine_end(256)[0])], 1, 64)
    assert out["info"][0].tolist() == [1, 1, 254, 0, 164470, 32894, 32896, 32896]
    assert out["cost"].max() == 164475 > 65535 and (out["path"][0, 63] >= 0).all()      # the open cell of the last wall: one move more


def test_generated_grids_contain_what_they_are_used_for():
    E = R.engineered()
    info = lambda name, ub: R.routes(*E[name][:2], E[name][2], ub, 64)["info"]      # noqa: E731
    assert info("gap_3", 1)[0, 1] == 1 and info("gap_2", 1)[0, 1] == 0 and info("gap_2", 1)[2, 1] == 1      # need2 = 4 against need2 = 1
    assert info("chink", 1)[:, 1].tolist() == [0, 0, 0, 0] and info("chink", 1)[0, 6] == 136
    assert info("source_not_passable", 1)[0].tolist() == [0, 0, -1, -1, 0, 0, 0, 229]
    assert info("walled_target", 1)[0].tolist()[:4] == [1, 0, 8, 9]
    assert info("target_is_source", 1)[0].tolist() == [1, 1, 5, 5, 0, 0, 256, 256]
    ig = info("ignore", 1)
    assert ig[0, 0] == 1 and ig[4, 0] == 0 and ig[1, 4] < ig[2, 4] == ig[3, 4]       # through the ignored box, or around it
    assert (info("out_of_contract", 1) != info("out_of_contract", 0)).any()
    assert (info("all_unknown_8", 1) == R.NO_ROUTE).all() and info("all_unknown_8", 0)[0, 1] == 1
    assert {len(v[2]) for v in E.values()} >= {3, 8} and {v[0].shape[0] for v in E.values()} == {8, 16}
    for G in (8, 64, 256):
        st, ow = R.random_grid(G, 1)
        qs = R.random_queries(G, 1, st, ow)
        R.check_params(G, qs, 1, 1024)
        pairs = [(q[5], q[0]) for q in qs]
        assert len(set(pairs)) < len(pairs) and len(set(pairs)) >= 5 and qs[3][3:5] == (-1, -1) and qs[6][1:3] == qs[6][3:5]
    st, ow = R.random_grid(256, 1)
    assert {-1, 0, 1, 2, 3} <= set(np.unique(st).tolist()) and {-5, 0, 128, 129} <= set(np.unique(ow).tolist())
    st, ow = R.big_grid()
    pas = R.passable_spans(R.free_cells(st, ow, 0, 1), 4096)
    assert pas[100, 100] and not pas[400, 100] and pas.sum() == 94898       # the target is too near the lone obstacle: a closest approach


def test_grid_of_72_has_queries_that_reach_their_targets():
    """What tests/test_routes_gpu.py's G = 72 case is there for: a second, partial ballot word per row of the run table."""
    st, ow = R.random_grid(72, 1)
    qs = R.random_queries(72, 1, st, ow)
    R.check_params(72, qs, 1, 256)
    assert R.routes(st, ow, qs, 1, 256)["info"][:, 1].sum() >= 1


def test_query_conversions():
    assert routes.query(0.04, (120, 40), (60, 200), 10) == (25, 120, 40, 60, 200, 0, 0, 0)       # ceil(40 / 10) + 1 = 5
    assert routes.query(0.04, (1, 2), None, 10, ignore=7) == (25, 1, 2, -1, -1, 7, 0, 0)
    assert routes.query(0.0, (0, 0), (511, 511), 20)[0] == 1 and routes.query(0.041, (0, 0), None, 10)[0] == 36
    assert routes.query(0.63, (0, 0), None, 10)[0] == 4096
    assert all(routes.query(r, (0, 0), None, c)[0] == placement.need2(r, c / 1000.0) for r, c in ((0.013, 7), (0.2, 25), (0.05, 10)))
    for bad in (dict(radius_m=0.64, src=(0, 0), dst=None, cell_mm=10), dict(radius_m=-0.01, src=(0, 0), dst=None, cell_mm=10),
                dict(radius_m=0.01, src=(-1, 0), dst=None, cell_mm=10), dict(radius_m=0.01, src=(0, 512), dst=None, cell_mm=10),
                dict(radius_m=0.01, src=(0, 0), dst=(-1, -1), cell_mm=10), dict(radius_m=0.01, src=(0, 0), dst=(0, 512), cell_mm=10),
                dict(radius_m=0.01, src=(0, 0), dst=None, cell_mm=0), dict(radius_m=0.01, src=(0, 0), dst=None, cell_mm=10, ignore=128),
                dict(radius_m=0.01, src=(0, 0), dst=None, cell_mm=10, ignore=-1)):
        with pytest.raises(ValueError):
            routes.query(**bad)


def test_error_paths_through_ctypes():
    lib = _native.lib()
    B, G, Q, P = 2, 16, 2, 64
    wsb = lib.uoc_routes_workspace_bytes
    nws = wsb(B, G, Q)
    assert nws >= B * Q * G * G * 3
    assert wsb(0, G, Q) == 0 and wsb(65536, G, Q) == 0 and wsb(65535, G, Q) > 0 and wsb(-1, G, Q) == 0
    assert wsb(B, 0, Q) == 0 and wsb(B, 12, Q) == 0 and wsb(B, 520, Q) == 0 and wsb(B, 512, Q) > 0 and wsb(B, 8, Q) > 0
    assert wsb(B, G, 0) == 0 and wsb(B, G, 9) == 0 and wsb(B, G, 8) > wsb(B, G, 1) > 0
    fake = ctypes.c_void_p(0x1000)                                   # never dereferenced: validation comes first
    good = list(R.record(4, (1, 2), (15, 15), 7)) + list(R.record(4096, (15, 0), None, 127))

    def call(B_=B, G_=G, queries=good, Q_=Q, ub=1, P_=P, nws_=nws, ws_=fake, drop=None):
        hq = (ctypes.c_int32 * max(len(queries), 1))(*queries)
        p = {k: fake for k in ("state", "owner", "frame", "cost", "info", "path")}
        p["queries"], p["ws"] = ctypes.cast(hq, ctypes.c_void_p), ws_
        if drop:
            p[drop] = None
        return lib.uoc_routes(p["state"], p["owner"], p["frame"], B_, G_, p["queries"], Q_, ub, P_, p["cost"], p["info"], p["path"], p["ws"],
                              nws_, None)

    def second(**kw):
        base = dict(need2=4, si=1, sj=2, ti=3, tj=4, ignore=0, w6=0, w7=0)
        base.update(kw)
        return good[:8] + [base[k] for k in ("need2", "si", "sj", "ti", "tj", "ignore", "w6", "w7")]

    bad = [dict(drop=k) for k in ("state", "owner", "queries", "cost", "info", "path", "ws")] + [
        dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(G_=-8), dict(Q_=0), dict(Q_=9), dict(Q_=-1),
        dict(ub=2), dict(ub=-1), dict(P_=0), dict(P_=4097), dict(P_=-1), dict(queries=second(need2=-1)), dict(queries=second(need2=4097)),
        dict(queries=second(si=-1)), dict(queries=second(si=16)), dict(queries=second(sj=-1)), dict(queries=second(sj=16)),
        dict(queries=second(ti=16)), dict(queries=second(tj=16)), dict(queries=second(ti=-1)), dict(queries=second(tj=-1)),
        dict(queries=second(ti=-2, tj=-2)), dict(queries=second(ignore=128)), dict(queries=second(ignore=-1)), dict(queries=second(w6=1)),
        dict(queries=second(w7=-1)), dict(queries=second(si=8), G_=8), dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ctypes.c_void_p(0x1008)),
        dict(ws_=ctypes.c_void_p(0x1004))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    for kw, word in ((dict(ws_=ctypes.c_void_p(0x1004)), b"aligned"), (dict(drop="owner"), b"null"), (dict(Q_=9), b"queries"),
                     (dict(queries=second(ignore=128)), b"ignore"), (dict(queries=second(need2=4097)), b"need2"),
                     (dict(queries=second(si=16)), b"source"), (dict(queries=second(ti=-1)), b"target"), (dict(queries=second(w6=1)), b"reserved"),
                     (dict(G_=12), b"grid"), (dict(nws_=nws - 1), b"workspace"), (dict(P_=0), b"max_path"), (dict(ub=2), b"unknown_blocks"),
                     (dict(B_=0), b"B=")):
        assert call(**kw) == EINVAL and word in lib.uoc_last_error(), (kw, lib.uoc_last_error())


def test_wrapper_value_errors_and_helpers():
    cpu = torch.zeros((1, 16, 16), dtype=torch.int32)
    with pytest.raises(_native.NativeError):
        routes.routes_records(cpu, cpu, None, [R.record(0, (0, 0))], 1)          # no CPU fallback
    for qs in ([], [R.record(0, (0, 0))] * 9, [R.record(4097, (0, 0))], [R.record(-1, (0, 0))], [R.record(0, (512, 0))], [R.record(0, (0, -1))],
               [R.record(0, (0, 0), (5, -1))], [R.record(0, (0, 0), (0, 512))], [R.record(0, (0, 0), ignore=128)], [(0, 0, 0, -1, -1, 0, 1, 0)],
               [(0, 0, 0)]):
        with pytest.raises(ValueError):
            routes._check_queries(qs)
    with pytest.raises(ValueError):
        routes._check_queries([R.record(0, (16, 0))], 16)                         # inside 512, outside this grid
    assert routes._check_queries(R.record(5, (1, 2), (3, 4), 6)).tolist() == [[5, 1, 2, 3, 4, 6, 0, 0]]
    placed = types.SimpleNamespace(state=cpu, owner=cpu, frame=None, grid=16, cell_mm=10, planes=None, unknown_blocks=True)
    for kw in (dict(queries=[R.record(0, (16, 16))]), dict(queries=[])):
        with pytest.raises(ValueError):
            routes.plan(placed, **kw)
    # helpers on a synthetic result: the flip, the truncation flag, the length and the camera points
    planes = torch.from_numpy(placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0]))
    cost = torch.full((1, 3, 16, 16), -1, dtype=torch.int32)
    cost[0, 0, 2, 2:5] = torch.tensor([0, 5, 10], dtype=torch.int32)
    info = torch.tensor([[[1, 1, 2, 4, 10, 2, 3, 200], [1, 0, -1, -1, 0, 0, 3, 200], [1, 0, 9, 9, 50, 10, 99, 200]]], dtype=torch.int32)
    path = torch.full((1, 3, 4, 2), -1, dtype=torch.int32)
    path[0, 0, :3] = torch.tensor([[2, 4], [2, 3], [2, 2]], dtype=torch.int32)
    path[0, 2] = torch.tensor([[9, 9], [8, 8], [7, 7], [6, 6]], dtype=torch.int32)
    res = types.SimpleNamespace(cost=cost, info=info, path=path, max_path=4, grid=16, cell_mm=10, planes=planes)
    assert routes.reachable_mask(res, 0).sum() == 3 and routes.reachable_mask(res, 0).shape == (1, 16, 16)
    w = routes.waypoints(res, 0, 0)
    assert w.cells.tolist() == [[2, 2], [2, 3], [2, 4]] and not w.truncated and w.reached_target and w.cost == 10
    assert routes.waypoints(res, 0, 1) is None and routes.length_m(res, 0, 1) is None and routes.path_to_camera(res, 0, 1) is None
    w = routes.waypoints(res, 0, 2)
    assert w.truncated and not w.reached_target and w.cells.tolist() == [[6, 6], [7, 7], [8, 8], [9, 9]]
    assert routes.length_m(res, 0, 0) == 10 * 10 / 5000.0
    xyz = routes.path_to_camera(res, 0, 0)
    assert xyz.shape == (3, 3) and xyz.dtype == np.float64
    assert np.allclose(xyz[2], placement.cell_to_camera(res, 0, 2, 4), rtol=0, atol=1e-15)
