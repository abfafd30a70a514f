"""uoc_motion / motion.register on the GPU against the numpy restatement (tests/motion_reference.py).

The stage has no floating-point output: rot and best are compared with np.array_equal, nothing is sampled.  The grids
are generated in the reference module and tests/test_motion_host.py asserts on the CPU what the hand cases contain.

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import ctypes
import faulthandler
import functools
import sys

import numpy as np
import pytest
import torch

from tests import motion_reference as R
from unseenobjectclustering_amd import _native, motion

pytestmark = pytest.mark.gpu
EINVAL = -22


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def blobs(G, seed):
    return R.blobs(G, seed)


def dev(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run(device, sa, oa, sb, ob, A, radius, pairs, fa=None, fb=None):
    """uoc_motion through the raw entry on host grids [G,G] or [B,G,G]; returns host arrays rot, best."""
    rot, best = motion.motion_records(dev(device, sa), dev(device, oa), None if fa is None else dev(device, fa), dev(device, sb),
                                      dev(device, ob), None if fb is None else dev(device, fb), R.rotation_table(A), radius, pairs)
    B, P = (1 if sa.ndim == 2 else sa.shape[0]), len(pairs)
    assert rot.shape == (B, P, 64, 4) and best.shape == (B, P, 16)
    assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in (rot, best))
    return {"rot": rot.cpu().numpy(), "best": best.cpu().numpy()}


def check(got, b, want, where):
    for k in ("rot", "best"):
        g = got[k][b]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (where, k, g.dtype, g.shape)
        bad = g != want[k]
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6], want[k][bad][:6])
    return want


def both(device, ga, gb, A, radius, pairs, where, **frames):
    """One frame on the device and in the reference; returns the reference's result."""
    got = run(device, ga[0], ga[1], gb[0], gb[1], A, radius, pairs, frames.get("fa"), frames.get("fb"))
    return check(got, 0, R.motion(ga[0], ga[1], gb[0], gb[1], R.rotation_table(A), radius, pairs, frames.get("fa"), frames.get("fb")), where)


# ---- hand cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [8, 64])
def test_hand_cases_match_reference(device, G):
    at = (0, 3) if G == 8 else (20, 30)
    want = both(device, *R.l_pair(G, at, move=(3, -2)), 16, 2, [(5, 5)], ("moved", G))
    assert want["best"][0, :5].tolist() == [1, 0, 0, 0, 0] and want["best"][0, 12:14].tolist() == [3, -2]
    for turn, k in ((1, 4), (3, 12)):
        ga, gb = R.l_pair(G, (2, 2) if G == 8 else (30, 30), move=(0, 1) if G == 8 else (2, 5), turn=turn)
        want = both(device, ga, gb, 16, 2, [(5, 5)], ("turned", G, turn))
        if G == 64:
            assert want["best"][0, [1, 4]].tolist() == [k, 0]
    sq = R.put(R.table(G), R.box(1, 7, 1, 7), 7)
    assert both(device, sq, sq, 16, 2, [(7, 7)], ("square", G))["best"][0, :5].tolist() == [1, 0, 0, 0, 0]
    bar = R.put(R.table(G), R.box(1, 7, 4, 5), 7)
    want = both(device, bar, bar, 16, 2, [(7, 7)], ("bar", G))
    assert want["best"][0, :5].tolist() == [1, 0, 0, 0, 0] and want["rot"][0, 8, 0] == 0
    # an object in each corner of the grid: with R = 4 the targets leave the grid on every side
    for n, (ca, cb) in enumerate(((R.box(0, 2, 0, 3), R.box(G - 2, G, G - 3, G)), (R.box(0, 3, G - 2, G), R.box(G - 3, G, 0, 2)))):
        ga, gb = R.put(R.table(G), ca, 4), R.put(R.table(G), cb, 4)
        want = both(device, ga, gb, 8, 4, [(4, 4)], ("corner", G, n))
        assert want["best"][0, 0] == 1 and want["rot"][0, :8, 0].max() > 0
        both(device, gb, ga, 8, 4, [(4, 4)], ("corner back", G, n))


# ---- degenerate pairs -------------------------------------------------------------------------------------------------
def test_degenerate_pairs_match_reference(device):
    one = R.put(R.table(16), [(5, 9)], 2)
    big = R.put(R.table(16), R.box(2, 9, 3, 12), 2)
    for n, (ga, gb) in enumerate(((one, one), (one, big), (big, one))):
        want = both(device, ga, gb, 8, 3, [(2, 2), (2, 6), (6, 2), (6, 6)], ("n = 1", n))
        assert want["best"][:, 0].tolist() == [1, 2, 2, 2] and want["best"][0, 5:7].min() == 1
    full = R.put(R.table(128), R.box(0, 64, 0, 64), 1)                     # 4096 cells
    more = R.put(R.put(R.table(128), R.box(0, 64, 0, 64), 1), [(100, 100)], 1)
    want = both(device, full, full, 2, 1, [(1, 1)], "n = 4096")
    assert want["best"][0, :8].tolist() == [1, 0, 0, 0, 0, 4096, 4096, 0]
    for n, (ga, gb) in enumerate(((full, more), (more, full), (more, more))):
        want = both(device, ga, gb, 2, 1, [(1, 1)], ("n = 4097", n))
        assert want["best"][0, 0] == 3 and want["best"][0, 5:7].max() == 4097 and (want["rot"][0] == R.NO_ROW).all()


# ---- frame records ----------------------------------------------------------------------------------------------------
def test_frame_records_match_reference(device):
    frames = [blobs(64, s) for s in (1, 2, 3, 4)]
    sa, oa, sb, ob = (np.stack([f[n] for f in frames]) for n in range(4))
    fa = np.stack([R.flat_frame(0), R.flat_frame(1), R.flat_frame(2), R.flat_frame(1)])
    fb = fa.copy()
    fb[3, 8] += 1                                                           # one word differs
    pairs = R.BLOB_PAIRS[:3]
    table = R.rotation_table(8)
    got = run(device, sa, oa, sb, ob, 8, 2, pairs, fa, fb)
    for b in range(4):
        want = check(got, b, R.motion(sa[b], oa[b], sb[b], ob[b], table, 2, pairs, fa[b], fb[b]), ("frame", b))
        assert want["best"][:, 0].tolist() == [1 if b == 1 else 0] * 3
    free = run(device, sa, oa, sb, ob, 8, 2, pairs)                          # both NULL: every frame as it stands
    for b in range(4):
        check(free, b, R.motion(sa[b], oa[b], sb[b], ob[b], table, 2, pairs), ("no frames", b))
    assert np.array_equal(free["best"][1], got["best"][1]) and np.array_equal(free["rot"][1], got["rot"][1])


# ---- parameter limits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 3, 5, 64])
def test_rotation_counts_match_reference(device, A):
    sa, oa, sb, ob = blobs(64, 5)
    want = both(device, (sa, oa), (sb, ob), A, 1, [(3, 3), (9, 3)], ("A", A))
    assert (want["best"][:, 0] == 1).all() and ((want["best"][:, 14] == -1).all() == (A <= 3))
    assert (want["rot"][:, A:] == R.NO_ROW).all() and (want["rot"][:, :A, 0] >= 0).all()


def test_radius_limits_and_sixteen_pairs_match_reference(device):
    sa, oa, sb, ob = blobs(32, 6)
    for radius in (0, 16):
        both(device, (sa, oa), (sb, ob), 4, radius, [(3, 3), (64, 64)], ("R", radius))
    ids = (3, 9, 64, 127)
    pairs = [(a, b) for a in ids for b in ids]                              # repeated and crossed ids: 16 pairs
    want = both(device, (sa, oa), (sb, ob), 6, 2, pairs, "P = 16")
    assert len(pairs) == 16 and (want["best"][:, 0] == 1).all()
    both(device, (sa, oa), (sb, ob), 64, 1, pairs, "A = 64, P = 16")         # 1024 (rotation, pair) blocks: a block owns a rotation's shifts


# ---- cell membership --------------------------------------------------------------------------------------------------
def test_only_state_two_with_the_exact_owner_is_a_cell(device):
    ga, gb = R.put(R.table(16), R.box(4, 9, 4, 7), 6), R.put(R.table(16), R.box(5, 10, 6, 9), 6)
    for (st, ow), at in ((ga, (4, 8)), (gb, (7, 10))):
        for n, (s, o) in enumerate(((2, 0), (2, 128), (2, -5), (3, 6), (-1, 6), (0, 6), (1, 6), (2, 6 + 128), (2, 7))):
            st[at[0] + n // 5, (at[1] + n) % 16], ow[at[0] + n // 5, (at[1] + n) % 16] = s, o
    want = both(device, ga, gb, 8, 2, [(6, 6), (7, 7), (6, 7)], "membership")
    assert want["best"][:, 5:7].tolist() == [[15, 15], [1, 1], [15, 1]]


# ---- seeded blobs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [8, 64, 256])
def test_seeded_blobs_match_reference(device, G):
    frames = [blobs(G, s) for s in (1, 2, 3)]
    sa, oa, sb, ob = (np.stack([f[n] for f in frames]) for n in range(4))
    A, radius = (8, 2) if G == 256 else (12, 3)
    table = R.rotation_table(A)
    want = [R.motion(*frames[b], table, radius, R.BLOB_PAIRS) for b in range(3)]      # once, shared by both batch sizes
    got = run(device, sa, oa, sb, ob, A, radius, R.BLOB_PAIRS)             # B = 3
    for b in range(3):
        check(got, b, want[b], (G, b))
    check(run(device, *frames[1], A, radius, R.BLOB_PAIRS), 0, want[1], (G, "alone"))      # B = 1
    assert any((w["best"][:, 0] == 1).any() for w in want) and all(w["best"][6, 0] == 2 for w in want)


def test_largest_grid_matches_reference(device):
    """G = 512: the bit planes take 64 KB of the block's LDS; cells in the last rows and columns, a mask at the limit."""
    G = 512
    ga = R.put(R.put(R.table(G), R.rectangle(G, (485.0, 490.5), 0.3, (30, 12)), 3), R.box(0, 64, 448, 512), 8)
    gb = R.put(R.put(R.table(G), R.rectangle(G, (487.5, 488.0), 0.9, (30, 12)), 3), R.box(448, 512, 0, 64), 8)
    want = both(device, ga, gb, 8, 2, [(3, 3), (8, 8), (8, 3)], "G = 512")
    assert want["best"][:, 0].tolist() == [1, 1, 1] and want["best"][1, 5:7].tolist() == [4096, 4096]
    assert (ga[1][511] == 3).any() and (gb[1][:, 511] == 3).any()                 # the object touches the last row and column


# ---- reproducibility and inputs ---------------------------------------------------------------------------------------
def test_frames_alone_among_mates_rerun_and_layouts(device):
    frames = [blobs(64, s) for s in (1, 2, 3, 4)]
    sa, oa, sb, ob = (dev(device, np.stack([f[n] for f in frames])) for n in range(4))
    table, pairs = R.rotation_table(16), R.BLOB_PAIRS[:5]
    call = lambda a, b, c, d: motion.motion_records(a, b, None, c, d, None, table, 3, pairs)      # noqa: E731
    same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))                            # noqa: E731
    whole, again = call(sa[:3], oa[:3], sb[:3], ob[:3]), call(sa[:3], oa[:3], sb[:3], ob[:3])
    assert same(whole, again)                                               # two runs, the same bits
    order = [3, 2, 0]
    other = call(sa[order], oa[order], sb[order], ob[order])                # frame 0 among other mates
    assert all(torch.equal(w[0], o[2]) for w, o in zip(whole, other))
    for b in range(3):
        alone = call(sa[b], oa[b], sb[b], ob[b])                            # [G,G]
        assert all(torch.equal(w[b], a[0]) for w, a in zip(whole, alone))
    assert same(whole, call(sa[:3].long(), oa[:3].long(), sb[:3].long(), ob[:3].long()))
    t = [x[:3].transpose(1, 2).contiguous().transpose(1, 2) for x in (sa, oa, sb, ob)]
    assert not t[0].is_contiguous() and torch.equal(t[0], sa[:3]) and same(whole, call(*t))
    one = motion.motion_records(sa[:3], oa[:3], None, sb[:3], ob[:3], None, table, 3, pairs[2:3])      # a pair alone
    assert torch.equal(one[0][:, 0], whole[0][:, 2]) and torch.equal(one[1][:, 0], whole[1][:, 2])
    got = {"rot": whole[0].cpu().numpy(), "best": whole[1].cpu().numpy()}
    check(got, 2, R.motion(*frames[2], table, 3, pairs), "batch")


# ---- rejected calls ---------------------------------------------------------------------------------------------------
def test_rejected_calls_do_no_device_work(device):
    lib = _native.lib()
    B, G, A, radius, P = 2, 16, 4, 2, 2
    nws = lib.uoc_motion_workspace_bytes(B, G, A, P)
    sa, oa, sb, ob = blobs(16, 1)
    d = [dev(device, np.stack([x] * B)) for x in (sa, oa, sb, ob)]
    frame = dev(device, np.stack([R.flat_frame(1)] * B))
    rot = torch.full((B, P, 64, 4), -7, dtype=torch.int32, device=device)
    best = torch.full((B, P, 16), -7, dtype=torch.int32, device=device)
    ws = torch.full((nws,), 0x55, dtype=torch.uint8, device=device)
    ws_big = torch.full((nws + 16,), 0x55, dtype=torch.uint8, device=device)
    ws_off = ws_big[4:]                                         # large enough, but 4 bytes off a 16-byte boundary
    Pt, stream = _native.ptr, _native.stream_ptr(device)
    assert ws.data_ptr() % 16 == 0 and ws_off.data_ptr() % 16 == 4
    good_rot, pairs = R.rotation_table(A).reshape(-1).tolist(), [(3, 3), (9, 3)]
    good_pairs = [x for p in pairs for x in p]

    def call(B_=B, G_=G, table=good_rot, A_=A, R_=radius, pr=good_pairs, P_=P, ws_=ws, nws_=nws, drop=()):
        hr = (ctypes.c_int32 * max(len(table), 1))(*table)
        hp = (ctypes.c_int32 * max(len(pr), 1))(*pr)
        p = dict(sa=Pt(d[0]), oa=Pt(d[1]), fa=Pt(frame), sb=Pt(d[2]), ob=Pt(d[3]), fb=Pt(frame), rot=Pt(rot), best=Pt(best), ws=Pt(ws_),
                 table=ctypes.cast(hr, ctypes.c_void_p), pairs=ctypes.cast(hp, ctypes.c_void_p))
        for k in drop:
            p[k] = None
        return lib.uoc_motion(p["sa"], p["oa"], p["fa"], p["sb"], p["ob"], p["fb"], B_, G_, p["table"], A_, R_, p["pairs"], P_, p["rot"],
                              p["best"], p["ws"], nws_, stream)

    over = [R.S, -R.S] * A
    for kw in [dict(drop=(k,)) for k in ("sa", "oa", "sb", "ob", "table", "pairs", "rot", "best", "ws", "fa", "fb")] + [
            dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(A_=0), dict(A_=65), dict(R_=-1), dict(R_=17),
            dict(P_=0), dict(P_=17), dict(table=over[:-1] + [-R.S - 1]), dict(table=[R.S + 1] + over[1:]), dict(pr=[0, 3, 9, 3]),
            dict(pr=[3, 3, 9, 128]), dict(pr=[3, -1, 9, 3]), dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ws_off)]:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (rot, best)) and bool((ws == 0x55).all()) and bool((ws_big == 0x55).all())
    assert call() == 0 and call(drop=("fa", "fb")) == 0 and call() == 0
    torch.cuda.synchronize()
    got = {"rot": rot.cpu().numpy(), "best": best.cpu().numpy()}
    check(got, 1, R.motion(sa, oa, sb, ob, R.rotation_table(A), radius, pairs, R.flat_frame(1), R.flat_frame(1)), "after the rejected calls")
    for args in ((d[0].cpu(), d[1], None, d[2], d[3], None), (d[0], d[1][:1], None, d[2], d[3], None), (d[0], d[1], None, d[2][:, :8, :8], d[3][:, :8, :8], None),
                 (d[0], d[1], frame, d[2], d[3], None), (d[0], d[1], frame[:1], d[2], d[3], frame), (d[0], d[1], frame.int(), d[2], d[3], frame)):
        with pytest.raises(_native.NativeError):
            motion.motion_records(*args, R.rotation_table(A), radius, pairs)
    for kw in (dict(table=np.zeros((65, 2), np.int64)), dict(table=R.rotation_table(A) * 2), dict(radius=17), dict(pairs=[(0, 1)]), dict(pairs=[])):
        full = {**dict(table=R.rotation_table(A), radius=radius, pairs=pairs), **kw}
        with pytest.raises(ValueError):
            motion.motion_records(d[0], d[1], None, d[2], d[3], None, full["table"], full["radius"], full["pairs"])


# ---- end to end -------------------------------------------------------------------------------------------------------
def _scene(device):
    """The placement generator's scene, its plane, a labelled object that owns cells, and the scene with that object's
    points moved by `cells` cells of 2 cm along the plane's axes."""
    from tests import placement_reference as PR
    from unseenobjectclustering_amd import placement, support
    lab, xyz = PR.tabletop(120, 160, 1)
    dl, dx = dev(device, lab), dev(device, xyz)
    fitted = support.fit_plane(dl, dx)
    placed = placement.free_space(dl, dx, fitted, grid=64, cell=0.02)
    cells = placed.cells[0].cpu().numpy()
    a = int(np.argmax(cells[1:])) + 1
    _, _, u, v = placement.plane_axes(placed.planes, 0)

    def moved(ci, cj):
        out = xyz.copy()
        valid = (lab == a) & (xyz[2] > 0)
        out[:, valid] += ((ci * 0.02 * u + cj * 0.02 * v)[:, None]).astype(np.float32)
        return dev(device, out)
    return dl, dx, fitted, placed, a, moved


def host_grids(placed):
    return tuple(getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner"))


def test_register_on_two_placements_of_the_generators_scene(device):
    from unseenobjectclustering_amd import placement
    dl, dx, fitted, placed, a, moved = _scene(device)
    after = placement.free_space(dl, moved(2, -3), fitted, grid=64, cell=0.02)
    res = motion.register(placed, after, [(a, a)], angles=16, radius=4)
    assert res.angles == 16 and res.radius == 4 and res.pairs.tolist() == [[a, a]] and res.grid == 64 and res.cell_mm == 20
    fr = placed.frame[0].cpu().numpy()
    want = R.motion(*host_grids(placed), *host_grids(after), R.rotation_table(16), 4, [(a, a)], fr, after.frame[0].cpu().numpy())
    check({"rot": res.rot.cpu().numpy(), "best": res.best.cpu().numpy()}, 0, want, "register")
    f = dict(zip(R.BEST_FIELDS, want["best"][0].tolist()))
    assert f["status"] == 1 and f["k"] == 0 and abs(f["ti"] - 2) <= 1 and abs(f["tj"] + 3) <= 1 and f["cost"] < f["still"]
    tr = motion.transform(res, 0, 0)
    assert tr.angle == 0.0 and np.allclose(tr.T[:3, :3], np.eye(3), atol=1e-9) and np.allclose(tr.T[:3, 3], tr.shift_xyz)
    assert motion.moved(res).tolist() == [[True]]
    # a frame against itself, every id on the grid: nothing moved
    still = motion.register(placed, placed, "same")
    ids = still.pairs[:, 0].tolist()
    cells = placed.cells[0].cpu().numpy()
    assert ids == [i for i in range(1, 128) if cells[i] > 0] and len(ids) >= 2
    for p, i in enumerate(ids):
        assert still.best[0, p].tolist() == [1, 0, 0, 0, 0, cells[i], cells[i], 0] + still.best[0, p, 8:12].tolist() + [0, 0] + still.best[0, p, 14:].tolist()
    assert not bool(motion.moved(still).any())
    with pytest.raises(ValueError):
        motion.register(placed, placement.free_space(dl, dx, fitted, grid=32, cell=0.02), [(a, a)])


def test_follower_over_three_frames(device):
    dl, dx, fitted, placed, a, moved = _scene(device)
    follow = motion.Follower(fitted, grid=64, cell=0.02, angles=16, radius=4)
    assert follow.update(dl, dx) is None
    travel = []
    for step in ((2, 0), (2, 3)):
        before = follow.last
        res = follow.update(dl, moved(*step), ids=[a])
        want = R.motion(*host_grids(before), *host_grids(follow.last), R.rotation_table(16), 4, [(a, a)],
                        before.frame[0].cpu().numpy(), follow.last.frame[0].cpu().numpy())
        check({"rot": res.rot.cpu().numpy(), "best": res.best.cpu().numpy()}, 0, want, ("follower", step))
        assert want["best"][0, 0] == 1
        travel.append(want["best"][0, 12:14].tolist())
    assert abs(travel[0][0] - 2) <= 1 and abs(travel[0][1]) <= 1 and abs(travel[1][0]) <= 1 and abs(travel[1][1] - 3) <= 1
    every = follow.update(dl, dx)                                          # ids=None: every id on both grids
    assert every is not None and a in every.pairs[:, 0].tolist() and bool((every.best[0, :, 0] == 1).all())


def test_readme_snippet_on_the_demo_pair(device, golden_dir):
    """The demo frame registered against itself: every id on the grid stays where it is."""
    import json
    import os
    from unseenobjectclustering_amd import io as uio, networks, objects as O, placement, support, synth
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    net, net_crop = (networks.seg_resnet34_8s_embedding(2, 64, sd).eval() for _ in range(2))
    np.random.seed(3)
    out_label, out_refined, _ = O.segment_objects(sample, net, net_crop)
    labels = (out_refined if out_refined is not None else out_label)[0].to(device)
    xyz = sample["depth"][0].to(device)
    fitted = support.fit_plane(labels, xyz)
    placed = placement.free_space(labels, xyz, fitted)
    res = motion.register(placed, placed, "same")
    cells = placed.cells[0].cpu().numpy()
    ids = res.pairs[:, 0].tolist()
    assert len(ids) >= 1 and ids == [i for i in range(1, 128) if cells[i] > 0]
    best = res.best[0].cpu().numpy()
    for p, i in enumerate(ids):
        assert best[p, :8].tolist() == [1, 0, 0, 0, 0, cells[i], cells[i], 0] and best[p, 12:14].tolist() == [0, 0], (i, best[p])
    assert not bool(motion.moved(res).any())
