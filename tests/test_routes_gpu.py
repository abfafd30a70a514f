"""uoc_routes / routes.plan on the GPU against the heap Dijkstra of tests/routes_reference.py.

The stage has no floating-point output: cost, info and path are compared with np.array_equal, nothing is sampled.  The
grids are generated in the reference module and tests/test_routes_host.py asserts on the CPU that they contain what they
are used for here.

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import ctypes
import faulthandler
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import routes_reference as R
from unseenobjectclustering_amd import _native, routes

pytestmark = pytest.mark.gpu
EINVAL = -22
KEYS = ("cost", "info", "path")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def random_grid(G, seed):
    return R.random_grid(G, seed)


def dev(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run(device, st, ow, queries, ub, max_path=64, frame=None):
    """uoc_routes through the raw entry on host grids [G,G] or [B,G,G]; returns host arrays cost, info, path."""
    cost, info, path = routes.routes_records(dev(device, st), dev(device, ow), None if frame is None else dev(device, frame), queries, ub, max_path)
    B, G, Q = (1 if st.ndim == 2 else st.shape[0]), st.shape[-1], len(queries)
    assert cost.shape == (B, Q, G, G) and info.shape == (B, Q, 8) and path.shape == (B, Q, max_path, 2)
    assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in (cost, info, path))
    return {"cost": cost.cpu().numpy(), "info": info.cpu().numpy(), "path": path.cpu().numpy()}


def check(got, b, want, where, q=None):
    for k in KEYS:
        g, w = got[k][b], want[k]
        if q is not None:
            g, w = g[q[0]], w[q[1]]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, g.shape, w.shape)
        bad = g != w
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6], w[bad][:6])
    return want


@pytest.mark.parametrize("name", list(R.engineered()))
def test_engineered_grids_match_reference(device, name):
    st, ow, queries = R.engineered()[name]
    for ub in (1, 0):
        want = check(run(device, st, ow, queries, ub), 0, R.routes(st, ow, queries, ub, 64), (name, ub))
        if name.startswith("all_obstacle") or (name.startswith("all_unknown") and ub == 1):
            keep = [q for q, r in enumerate(queries) if r[5] != 4]                   # ignore = 4 would free the obstacle
            assert (want["cost"][keep] == -1).all() and all(want["info"][q].tolist() == list(R.NO_ROUTE) for q in keep)


def test_hand_counted_grid_on_the_device(device):
    st, ow = R.hand8()
    out = run(device, st, ow, [R.record(0, (2, 2), (7, 7)), R.record(0, (2, 2), (2, 5)), R.record(0, (2, 2))], 1, 16)
    c = out["cost"][0, 0]
    assert (c[2, 2], c[2, 3], c[6, 3], c[6, 4], c[7, 5], c[7, 7], c[6, 5], c[2, 5]) == (0, 5, 22, 27, 34, 44, 32, 52)
    assert (c[:6, 4] == -1).all() and (c >= 0).sum() == 58
    assert out["info"][0].tolist() == [[1, 1, 7, 7, 44, 8, 58, 58], [1, 1, 2, 5, 52, 10, 58, 58], [1, 0, -1, -1, 0, 0, 58, 58]]
    assert out["path"][0, 0, :9].tolist() == [[7, 7], [7, 6], [7, 5], [7, 4], [6, 3], [5, 3], [4, 3], [3, 3], [2, 2]]
    assert (out["path"][0, 0, 9:] == -1).all() and (out["path"][0, 2] == -1).all()
    # the border band of an empty table: need2 0 and 1 reach every cell, 2 leaves a band of one cell, 25 a band of four
    st, ow = R.table(16)
    out = run(device, st, ow, [R.record(n, (8, 8)) for n in (0, 1, 2, 25)], 1)
    assert out["info"][0, :, 6].tolist() == [256, 256, 196, 64]
    assert (out["cost"][0, 2, 1:15, 1:15] >= 0).all() and (out["cost"][0, 2, 0] == -1).all() and (out["cost"][0, 3, 3] == -1).all()


@pytest.mark.parametrize("G", [8, 64, 256])
def test_random_grids_match_reference(device, G):
    frames = [random_grid(G, seed) for seed in (1, 2, 3)]
    st3, ow3 = (np.stack([f[n] for f in frames]) for n in range(2))
    queries = R.random_queries(G, 1, *frames[0])
    pairs = [(q[5], q[0]) for q in queries]
    assert len(set(pairs)) < len(pairs)                         # queries that share (ignore, need2) and queries that differ
    for ub in ((1, 0) if G < 256 else (1,)):
        if G < 256:
            want = [R.routes(*frames[b], queries, ub, 256) for b in range(3)]        # once, shared by both batch sizes
            got = run(device, st3, ow3, queries, ub, 256)                           # B = 3, Q = 8
            for b in range(3):
                check(got, b, want[b], (G, ub, b))
            check(run(device, *frames[1], queries[2:3], ub, 256), 0, want[1], (G, ub, "alone"), q=(slice(0, 1), slice(2, 3)))      # B = 1, Q = 1
        else:                                                   # the reference takes a second per eight fields: B = 1 with Q = 8, B = 3 with Q = 1
            want = R.routes(*frames[0], queries, ub, 256)
            check(run(device, *frames[0], queries, ub, 256), 0, want, (G, ub, "Q = 8"))
            got = run(device, st3, ow3, queries[:1], ub, 256)
            check(got, 0, want, (G, ub, "B = 3", 0), q=(slice(0, 1), slice(0, 1)))
            for b in (1, 2):
                check(got, b, R.routes(*frames[b], queries[:1], ub, 256), (G, ub, "B = 3", b))
            assert want["info"][:, 1].sum() >= 4 and want["info"][:, 5].max() > 100


def test_partial_ballot_word_of_the_runs_matches_reference(device):
    """G = 72: a row of the run table is one ballot word of 64 cells and one of 8; that queries reach their targets on this
    grid is asserted in tests/test_routes_host.py."""
    st, ow = random_grid(72, 1)
    queries = R.random_queries(72, 1, st, ow)
    check(run(device, st, ow, queries, 1, 256), 0, R.routes(st, ow, queries, 1, 256), "G = 72")


def test_largest_disc_on_the_largest_grid(device):
    st, ow = R.big_grid()
    queries = [R.record(4096, (100, 100), (400, 100)), R.record(4096, (100, 100), (380, 440), ignore=9)]
    want = R.routes(st, ow, queries, 1, 1024, passable_fn=R.passable_spans)        # the all-offsets form takes 12 861 shifts of the grid
    check(run(device, st, ow, queries, 1, 1024), 0, want, "G = 512")
    assert want["info"][0].tolist()[:2] == [1, 0] and want["info"][1].tolist()[:2] == [1, 1] and want["info"][0, 5] > 500


def test_serpentines_and_the_path_buffer(device):
    # G = 64: 32-bit words; the path is 2078 moves long: max_path of 1, of exactly steps, and of steps + 1
    st, ow = R.serpentine(64)
    end, cost = R.serpentine_end(64)
    q = [R.record(0, (0, 0), end)]
    full = R.routes(st, ow, q, 1, 4096)
    steps = int(full["info"][0, 5])
    assert full["info"][0].tolist()[:6] == [1, 1, end[0], end[1], cost, steps] and steps == 32 * 63 + 2 * 31
    for P in (1, steps, steps + 1):
        want = {"cost": full["cost"], "info": full["info"], "path": full["path"][:, :P]}
        got = check(run(device, st, ow, q, 1, P), 0, want, ("serpentine 64", P))
        assert (got["path"][0, -1] >= 0).all() and (P <= steps) == (got["path"][0, -1].tolist() != [0, 0])
    # G = 256, need2 = 0: costs above 65535, the smallest grid at which 16-bit words can go wrong
    st, ow = R.serpentine(256)
    end, cost = R.serpentine_end(256)
    q = [R.record(0, (0, 0), end), R.record(0, (128, 5), (0, 0))]
    want = check(run(device, st, ow, q, 1, 64), 0, R.routes(st, ow, q, 1, 64), "serpentine 256")
    assert want["info"][0].tolist()[:6] == [1, 1, end[0], end[1], cost, 32894] and cost > 65535 and want["cost"].max() > 65535


def test_frames_alone_among_mates_rerun_layouts_and_frame_records(device):
    frames = [random_grid(64, seed) for seed in (1, 2, 3, 4)]
    st, ow = (dev(device, np.stack([f[n] for f in frames])) for n in range(2))
    queries = R.random_queries(64, 1, *frames[0])
    call = lambda s, o, fr=None: routes.routes_records(s, o, fr, queries, 1, 128)      # noqa: E731
    same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))                 # noqa: E731
    whole, again = call(st[:3], ow[:3]), call(st[:3], ow[:3])
    assert same(whole, again)                                                        # two runs, the same bits
    order = [3, 2, 0]
    other = call(st[order], ow[order])                                               # frame 0 among other mates
    assert all(torch.equal(w[0], o[2]) for w, o in zip(whole, other))
    for b in range(3):
        alone = call(st[b], ow[b])                                                   # [G,G]
        assert all(torch.equal(w[b], a[0]) for w, a in zip(whole, alone))
    wide = call(st[:3].long(), ow[:3].long())
    ts, to = (t[:3].transpose(1, 2).contiguous().transpose(1, 2) for t in (st, ow))
    assert not ts.is_contiguous() and torch.equal(ts, st[:3])
    assert same(whole, wide) and same(whole, call(ts, to))
    got = {k: v.cpu().numpy() for k, v in zip(KEYS, whole)}
    check(got, 1, R.routes(*frames[1], queries, 1, 128), "batch")
    # frame records: word 13 = 0 and 2 next to a good frame; NULL evaluates every frame
    rec = np.stack([R.flat_frame(0), R.flat_frame(1), R.flat_frame(2)])
    with_frames = call(st[:3], ow[:3], dev(device, rec))
    got = {k: v.cpu().numpy() for k, v in zip(KEYS, with_frames)}
    for b in range(3):
        want = check(got, b, R.routes(*frames[b], queries, 1, 128, rec[b]), ("frame", b))
        assert (b == 1) == bool((want["cost"] >= 0).any())
        if b != 1:
            assert (got["cost"][b] == -1).all() and (got["path"][b] == -1).all() and all(r.tolist() == list(R.NO_ROUTE) for r in got["info"][b])
    assert all(torch.equal(w[1], f[1]) for w, f in zip(whole, with_frames))


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, G, Q, P = 2, 16, 2, 32
    nws = lib.uoc_routes_workspace_bytes(B, G, Q)
    st, ow = R.only_obstacle(G)
    ds, do = (dev(device, np.stack([x] * B)) for x in (st, ow))
    frame = dev(device, np.stack([R.flat_frame(1)] * B))
    cost = torch.full((B, Q, G, G), -7, dtype=torch.int32, device=device)
    info = torch.full((B, Q, 8), -7, dtype=torch.int32, device=device)
    path = torch.full((B, Q, P, 2), -7, dtype=torch.int32, device=device)
    ws = torch.full((nws,), 0x55, dtype=torch.uint8, device=device)
    ws_big = torch.full((nws + 16,), 0x55, dtype=torch.uint8, device=device)
    ws_off = ws_big[4:]                                         # large enough, but 4 bytes off a 16-byte boundary
    ptr, stream = _native.ptr, _native.stream_ptr(device)
    assert ws.data_ptr() % 16 == 0 and ws_off.data_ptr() % 16 == 4
    recs = [R.record(4, (2, 5), (12, 5), 7), R.record(1, (2, 5), (7, 5))]
    good = [x for r in recs for x in r]

    def call(B_=B, G_=G, queries=good, Q_=Q, ub=1, P_=P, ws_=ws, nws_=nws, drop=None):
        hq = (ctypes.c_int32 * max(len(queries), 1))(*queries)
        p = dict(state=ptr(ds), owner=ptr(do), frame=ptr(frame), cost=ptr(cost), info=ptr(info), path=ptr(path), ws=ptr(ws_),
                 queries=ctypes.cast(hq, ctypes.c_void_p))
        if drop:
            p[drop] = None
        return lib.uoc_routes(p["state"], p["owner"], p["frame"], B_, G_, p["queries"], Q_, ub, P_, p["cost"], p["info"], p["path"], p["ws"],
                              nws_, stream)

    def second(**kw):
        base = dict(need2=4, si=1, sj=2, ti=3, tj=4, ignore=0, w6=0, w7=0)
        base.update(kw)
        return good[:8] + [base[k] for k in ("need2", "si", "sj", "ti", "tj", "ignore", "w6", "w7")]

    for kw in [dict(drop=k) for k in ("state", "owner", "queries", "cost", "info", "path", "ws")] + [
            dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(Q_=0), dict(Q_=9), dict(ub=2), dict(ub=-1),
            dict(P_=0), dict(P_=4097), dict(queries=second(need2=-1)), dict(queries=second(need2=4097)), dict(queries=second(si=-1)),
            dict(queries=second(sj=16)), dict(queries=second(ti=16)), dict(queries=second(tj=-1)), dict(queries=second(ti=-2, tj=-2)),
            dict(queries=second(ignore=128)), dict(queries=second(ignore=-1)), dict(queries=second(w6=1)), dict(queries=second(w7=1)),
            dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ws_off)]:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (cost, info, path)) and bool((ws == 0x55).all()) and bool((ws_big == 0x55).all())
    assert call() == 0 and call(drop="frame") == 0 and call() == 0
    torch.cuda.synchronize()
    got = {"cost": cost.cpu().numpy(), "info": info.cpu().numpy(), "path": path.cpu().numpy()}
    check(got, 1, R.routes(st, ow, recs, 1, P), "after the rejected calls")
    for bad in (dict(queries=[]), dict(queries=[recs[0]] * 9), dict(queries=[R.record(4097, (0, 0))]), dict(queries=[R.record(0, (16, 0))]),
                dict(queries=[R.record(0, (0, 0), ignore=128)]), dict(max_path=0), dict(max_path=4097)):
        kw = {**dict(queries=recs, unknown_blocks=1), **bad}
        with pytest.raises(ValueError):
            routes.routes_records(ds, do, None, **kw)
    kw = dict(queries=recs, unknown_blocks=1)
    for args in ((ds.cpu(), do, None), (ds, do[:1], None), (ds, do[:, :8], None), (ds[:, :12, :12], do[:, :12, :12], None), (ds, do, frame[:1]),
                 (ds, do, frame.int())):
        with pytest.raises(_native.NativeError):
            routes.routes_records(*args, **kw)


def test_plan_on_a_placement_result_and_helpers(device):
    from tests import placement_reference as PR
    from unseenobjectclustering_amd import placement, support
    lab, xyz = PR.tabletop(120, 160, 1)
    dl, dx = dev(device, lab), dev(device, xyz)
    fitted = support.fit_plane(dl, dx)
    placed = placement.free_space(dl, dx, fitted, grid=64, cell=0.02, queries=[(placement.need2(0.03, 0.02), 0, 0, placement.WIDEST)])
    st, ow, d2, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "dist2", "frame"))
    assert fr[13] == 1 and (st == 1).sum() > 100 and (st == 2).any()
    a = R.present_id(ow, st)
    spot = tuple(int(x) for x in placed.answers[0, 0, :2].cpu().tolist())
    assert spot[0] >= 0
    mine = routes.of_object(placed, fitted, 0, a, spot, margin=0.005)
    h = max(fitted.half[0, a, :2].cpu().tolist())
    centre = placement.camera_to_cell(placed, 0, fitted.center[0, a].cpu().tolist())
    assert mine[5] == a and mine[1:3] == tuple(centre) and mine[3:5] == spot and mine[0] == placement.need2(h + 0.005, 0.02)
    bare = routes.of_object(placed, fitted, 0, a, None, radius_m=0.01)
    assert (bare[0], bare[3:]) == (4, (-1, -1, a, 0, 0)) and bare[1:3] == mine[1:3]
    table = [tuple(int(x) for x in c) for c in np.argwhere((st == 1) & (d2 >= 9))]
    queries = [routes.query(0.03, table[0], table[-1], placed.cell_mm), mine, routes.query(0.0, table[len(table) // 2], None, placed.cell_mm)]
    for over in (None, False):
        res = routes.plan(placed, queries, unknown_blocks=over, max_path=256)
        want_ub = 1 if over is None else 0
        assert res.unknown_blocks == bool(want_ub) and res.max_path == 256 and res.queries.tolist() == [list(q) for q in queries]
        got = {k: getattr(res, k).cpu().numpy() for k in KEYS}
        want = check(got, 0, R.routes(st, ow, queries, want_ub, 256, fr), ("plan", over))
    # with ignore == 0 the stage's PASSABLE is the placement stage's own clearance (§15 E)
    res1 = routes.plan(placed, queries, max_path=256)
    m = routes.reachable_mask(res1, 0)
    assert m.shape == (1, 64, 64) and m.dtype == torch.bool and m.device.type == "cuda"
    n2 = queries[0][0]
    assert int(res1.info[0, 0, 7]) == int(((placed.state[0] == 1) & (placed.dist2[0] >= n2)).sum())
    assert not bool((m[0] & ~((placed.state[0] == 1) & (placed.dist2[0] >= n2))).any())
    w = routes.waypoints(res, 0, 0)
    info = want["info"][0]
    assert info[0] == 1 and w.cells[0].tolist() == list(queries[0][1:3]) and w.cells[-1].tolist() == info[2:4].tolist()
    assert len(w.cells) == info[5] + 1 and not w.truncated and w.cost == info[4] and w.reached_target == bool(info[1])
    assert routes.length_m(res, 0, 0) == info[4] * 20 / 5000.0 and routes.waypoints(res, 0, 2) is None
    xyz_path = routes.path_to_camera(res, 0, 0)
    assert xyz_path.shape == (len(w.cells), 3) and xyz_path.dtype == np.float64
    for k in (0, len(w.cells) // 2, len(w.cells) - 1):
        assert np.allclose(xyz_path[k], placement.cell_to_camera(placed, 0, *w.cells[k]), rtol=0, atol=1e-12)
    steps = np.linalg.norm(np.diff(xyz_path, axis=0), axis=1) / 0.02                     # cells: 1 or sqrt 2 per move
    assert all(min(abs(s - 1.0), abs(s - 2.0 ** 0.5)) < 1e-4 for s in steps.tolist())
    cut = routes.plan(placed, queries[:1], unknown_blocks=False, max_path=2)
    assert routes.waypoints(cut, 0, 0).truncated == (info[5] >= 2)


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_routes_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    queries = [routes.query(0.03, (128, 100), (100, 160), 10), routes.query(0.0, (128, 128), None, 10, ignore=1)]
    np.random.seed(3)
    out = O.segment_objects(sample, net, net_crop, routes=True, routes_args=dict(queries=queries, max_path=512))
    assert len(out) == 6                                        # implies placement, which implies the plane
    placed, routed = out[4], out[5]
    assert hasattr(out[3], "normal") and hasattr(placed, "dist2") and routed.planes.data_ptr() == placed.planes.data_ptr()
    st, ow, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "frame"))
    got = {k: getattr(routed, k).cpu().numpy() for k in KEYS}
    check(got, 0, R.routes(st, ow, queries, 1, 512, fr), "demo")
    with pytest.raises(ValueError):
        O.segment_objects(sample, net, net_crop, routes=True)
    np.random.seed(3)
    every = O.segment_objects(sample, net, net_crop, elevation=True, routes=True, routes_args=dict(queries=queries[:1], unknown_blocks=False))
    assert len(every) == 7 and hasattr(every[5], "elev") and torch.equal(every[4].state, placed.state)
    got = {k: getattr(every[6], k).cpu().numpy() for k in KEYS}
    check(got, 0, R.routes(st, ow, queries[:1], 0, 1024, fr), "demo, other arguments")
