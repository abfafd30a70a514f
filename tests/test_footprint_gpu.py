"""uoc_footprint / footprint.fit on the GPU against the numpy restatement (tests/footprint_reference.py).

The stage has no floating-point output: fits, count and best are compared with np.array_equal, nothing is sampled.  The
grids are generated in the reference module and tests/test_footprint_host.py asserts on the CPU that they contain what
they are used for here.

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

from tests import footprint_reference as R
from unseenobjectclustering_amd import _native, footprint

pytestmark = pytest.mark.gpu
EINVAL = -22


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


def run(device, st, ow, d2, A, rects, ub, frame=None):
    """uoc_footprint through the raw entry on host grids [G,G] or [B,G,G]; returns host arrays fits, count, best."""
    fits, count, best = footprint.footprint_records(dev(device, st), dev(device, ow), dev(device, d2),
                                                    None if frame is None else dev(device, frame), R.direction_table(A), rects, ub)
    B, G, F = (1 if st.ndim == 2 else st.shape[0]), st.shape[-1], len(rects)
    assert fits.shape == (B, F, G, G) and count.shape == (B, F, 32) and best.shape == (B, F, 8)
    assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in (fits, count, best))
    return {"fits": fits.cpu().numpy(), "count": count.cpu().numpy(), "best": best.cpu().numpy()}


def check(got, b, want, where):
    for k in ("fits", "count", "best"):
        g = got[k][b]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (where, k, g.dtype, g.shape)
        bad = g != want[k]
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6], want[k][bad][:6])
    return want


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_grids_match_reference(device, name):
    st, ow = R.ENGINEERED[name]()
    for ub in (1, 0):
        d2 = R.clearance(st, ow, ub)
        for A, rects in R.ENGINEERED_SETS:
            want = check(run(device, st, ow, d2, A, rects, ub), 0, R.footprint(st, ow, d2, R.direction_table(A), rects, ub), (name, A, ub))
            if name == "all_obstacle" or (name == "all_unknown" and ub == 1):
                keep = [f for f, r in enumerate(rects) if r[2] != 4]               # ignore = 4 would free the obstacle
                assert not want["fits"][keep].any() and all(want["best"][f].tolist() == list(R.NO_POSE) for f in keep)


def test_hand_counted_grids_on_the_device(device):
    st, ow = R.bar8()
    d2 = R.clearance(st, ow)
    out = run(device, st, ow, d2, 2, [R.record(256, 0), R.record(256, 0, mode=R.NEAREST, ai=7, aj=4), R.record(256, 0, ignore=3)], 1)
    assert out["count"][0, :, :2].tolist() == [[18, 8], [18, 8], [48, 48]] and not out["count"][0, :, 2:].any()
    assert out["best"][0, 0].tolist() == [1, 1, 4, 0, 4, 17, 26, 20] and out["best"][0, 1].tolist() == [1, 7, 4, 1, 1, 0, 26, 20]
    f = out["fits"][0, 0]
    assert (f[1:7, 3] == 1).all() and (f[1:7, 4] == 3).all() and f[0, 4] == 2 and f[7, 4] == 2 and not f[:, :3].any() and not f[:, 6:].any()
    # the empty table: the border band is excluded
    st, ow = R.table(32)
    out = run(device, st, ow, R.clearance(st, ow), 2, [R.record(640, 0)], 1)
    assert out["count"][0, 0, :2].tolist() == [28 * 32, 32 * 28] and out["fits"][0, 0][2, 2] == 3 and out["fits"][0, 0][1, 2] == 2
    # the corridor exactly as wide as the mask, and one cell narrower
    for name, k, n in (("corridor_i_5", 1, 32), ("corridor_i_4", 1, 0), ("corridor_j_5", 0, 32), ("corridor_j_4", 0, 0)):
        st, ow = R.ENGINEERED[name]()
        assert run(device, st, ow, R.clearance(st, ow), 2, [R.record(640, 0)], 1)["count"][0, 0, k] == n, name
    # one orientation only; the last row and column
    st, ow = R.case_one_orientation()
    out = run(device, st, ow, R.clearance(st, ow), 16, [R.record(1920, 128)], 1)
    assert out["count"][0, 0, 8] == 3 and out["count"][0, 0].sum() == 3 and out["best"][0, 0, :4].tolist() == [1, 15, 13, 8]
    st, ow = R.case_last_row_column()
    f = run(device, st, ow, R.clearance(st, ow), 2, [R.record(640, 0)], 1)["fits"][0, 0]
    assert f[15, 2] == 2 and f[2, 15] == 1 and f[15, 13] == 2 and f[15, 14] == 0
    # ignore: the only obstacle's id, an absent id
    st, ow = R.case_only_obstacle()
    c = run(device, st, ow, R.clearance(st, ow), 2, [R.record(640, 0, ignore=g) for g in (7, 9, 0)], 1)["count"][0, :, 0]
    assert c[0] == 20 * 24 and c[1] == c[2] < c[0]


def test_clamp_bit_31_and_anchor_outside(device):
    st, ow = R.table(16)
    d2 = np.full((16, 16), 9, np.int32)
    d2[5, 7], d2[11, 2] = 70000, 65536
    out = run(device, st, ow, d2, 4, [R.record(0, 0)], 1)
    assert out["best"][0, 0].tolist() == [1, 5, 7, 0, 65536, 5 * 5 + 7 * 7, 4 * 256, 256]       # 70000 clamps to 65536: a tie, the lower index
    d2[:] = -1
    out = run(device, st, ow, d2, 4, [R.record(0, 0), R.record(0, 0, mode=R.NEAREST, ai=-4096, aj=4095)], 1)
    assert out["best"][0, 0, :5].tolist() == [1, 0, 0, 0, 0]                                      # -1 clamps to 0
    assert out["best"][0, 1, :6].tolist() == [1, 0, 15, 0, 0, 4096 ** 2 + 4080 ** 2]
    for A in (1, 32):
        out = run(device, st, ow, d2, A, [R.record(0, 0)], 1)
        word = 1 if A == 1 else -1
        assert (out["fits"][0, 0] == word).all() and (out["count"][0, 0, :A] == 256).all() and not out["count"][0, 0, A:].any()
    st2, ow2 = R.corridor(16, 1, along_i=True, at=6)                                              # only k = 31's neighbour k = 0 and bit 31
    out = run(device, st2, ow2, d2, 32, [R.record(256, 20)], 1)
    want = R.footprint(st2, ow2, d2, R.direction_table(32), [R.record(256, 20)], 1)
    check(out, 0, want, "bit 31")
    assert want["count"][0, 31] > 0 and (want["fits"][0] < 0).any()


def test_longest_bar_on_the_largest_grid(device):
    G = 512
    st, ow = R.table(G)
    st[200:204, 100:400], ow[200:204, 100:400] = 2, 5
    st[300, 300] = 0
    d2 = R.seeded_dist2(G, 5)
    rects = [R.record(16384, 0)]
    want = R.footprint(st, ow, d2, R.direction_table(32), rects, 1)
    check(run(device, st, ow, d2, 32, rects, 1), 0, want, "G = 512")
    assert want["count"][0, 0] > 0 and want["count"][0, 16] > 0 and want["best"][0, 0] == 1


@pytest.mark.parametrize("G", [8, 64, 256])
def test_random_grids_match_reference(device, G):
    frames = [random_grid(G, seed) for seed in (1, 2, 3)]
    st3, ow3, d3 = (np.stack([f[n] for f in frames]) for n in range(3))
    P = R.present_id(ow3[0], st3[0])
    for n, (A, specs, ub) in enumerate(R.RANDOM_SETS):
        rects, dirs = R.resolve(specs, P), R.direction_table(A)
        want = [R.footprint(*frames[b], dirs, rects, ub) for b in range(3)]      # once, shared by both batch sizes
        got = run(device, st3, ow3, d3, A, rects, ub)               # B = 3
        for b in range(3):
            check(got, b, want[b], (G, n, b))
        b = n % 3                                                   # B = 1
        check(run(device, *frames[b], A, rects, ub), 0, want[b], (G, n, "alone", b))


def test_partial_ballot_word_of_the_runs_matches_reference(device):
    """G = 72: a row of the run table is one ballot word of 64 cells and one of 8; the fitting cells in those 8 columns are
    asserted in tests/test_footprint_host.py."""
    st, ow, d2 = random_grid(72, 1)
    A, specs, ub = R.RANDOM_SETS[0]
    rects = R.resolve(specs, R.present_id(ow, st))
    check(run(device, st, ow, d2, A, rects, ub), 0, R.footprint(st, ow, d2, R.direction_table(A), rects, ub), "G = 72")


def test_frames_alone_among_mates_rerun_layouts_and_frame_records(device):
    frames = [random_grid(64, seed) for seed in (1, 2, 3, 4)]
    st, ow, d2 = (dev(device, np.stack([f[n] for f in frames])) for n in range(3))
    A, specs, ub = R.RANDOM_SETS[5]
    rects, dirs = R.resolve(specs, R.present_id(frames[0][1], frames[0][0])), R.direction_table(A)
    call = lambda s, o, d, fr=None: footprint.footprint_records(s, o, d, fr, dirs, rects, ub)      # noqa: E731
    same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))                              # noqa: E731
    whole, again = call(st[:3], ow[:3], d2[:3]), call(st[:3], ow[:3], d2[:3])
    assert same(whole, again)                                                                     # two runs, the same bits
    order = [3, 2, 0]
    other = call(st[order], ow[order], d2[order])                                                 # frame 0 among other mates
    assert all(torch.equal(w[0], o[2]) for w, o in zip(whole, other))
    for b in range(3):
        alone = call(st[b], ow[b], d2[b])                                                         # [G,G]
        assert all(torch.equal(w[b], a[0]) for w, a in zip(whole, alone))
    wide = call(st[:3].long(), ow[:3].long(), d2[:3].long())
    ts, to, td = (t[:3].transpose(1, 2).contiguous().transpose(1, 2) for t in (st, ow, d2))
    assert not ts.is_contiguous() and torch.equal(ts, st[:3])
    assert same(whole, wide) and same(whole, call(ts, to, td))
    got = {k: v.cpu().numpy() for k, v in zip(("fits", "count", "best"), whole)}
    check(got, 1, R.footprint(*frames[1], dirs, rects, ub), "batch")
    # frame records: word 13 = 0 and 2 next to a good frame; NULL evaluates every frame
    rec = np.stack([R.flat_frame(0), R.flat_frame(1), R.flat_frame(2)])
    with_frames = call(st[:3], ow[:3], d2[:3], dev(device, rec))
    got = {k: v.cpu().numpy() for k, v in zip(("fits", "count", "best"), with_frames)}
    for b in range(3):
        want = check(got, b, R.footprint(*frames[b], dirs, rects, ub, rec[b]), ("frame", b))
        assert (b == 1) == bool(want["fits"].any())
        if b != 1:
            assert not got["count"][b].any() and all(r.tolist() == list(R.NO_POSE) for r in got["best"][b])
    assert all(torch.equal(w[1], f[1]) for w, f in zip(whole, with_frames))


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, G, A, F = 2, 16, 4, 2
    nws = lib.uoc_footprint_workspace_bytes(B, G, A, F)
    st, ow = R.case_one_blocker(G)
    d2 = R.clearance(st, ow)
    ds, do, dd = (dev(device, np.stack([x] * B)) for x in (st, ow, d2))
    frame = dev(device, np.stack([R.flat_frame(1)] * B))
    fits = torch.full((B, F, G, G), -7, dtype=torch.int32, device=device)
    count = torch.full((B, F, 32), -7, dtype=torch.int32, device=device)
    best = torch.full((B, F, 8), -7, dtype=torch.int32, device=device)
    ws = torch.full((nws,), 0x55, dtype=torch.uint8, device=device)
    ws_big = torch.full((nws + 16,), 0x55, dtype=torch.uint8, device=device)
    ws_off = ws_big[4:]                                         # large enough, but 4 bytes off a 16-byte boundary
    P, stream = _native.ptr, _native.stream_ptr(device)
    assert ws.data_ptr() % 16 == 0 and ws_off.data_ptr() % 16 == 4
    good_dirs = R.direction_table(A).reshape(-1).tolist()
    recs = [R.record(640, 200), R.record(300, 0, 9, R.NEAREST, -4096, 4095)]
    good_rects = [x for r in recs for x in r]

    def call(B_=B, G_=G, dirs=good_dirs, A_=A, rects=good_rects, F_=F, ub=1, ws_=ws, nws_=nws, drop=None):
        hd = (ctypes.c_int32 * max(len(dirs), 1))(*dirs)
        hr = (ctypes.c_int32 * max(len(rects), 1))(*rects)
        p = dict(state=P(ds), owner=P(do), dist2=P(dd), frame=P(frame), fits=P(fits), count=P(count), best=P(best), ws=P(ws_),
                 dirs=ctypes.cast(hd, ctypes.c_void_p), rects=ctypes.cast(hr, ctypes.c_void_p))
        if drop:
            p[drop] = None
        return lib.uoc_footprint(p["state"], p["owner"], p["dist2"], p["frame"], B_, G_, p["dirs"], A_, p["rects"], F_, ub, p["fits"],
                                 p["count"], p["best"], p["ws"], nws_, stream)

    def second(**kw):
        base = dict(HL=640, HW=200, ignore=0, mode=0, ai=0, aj=0, w6=0, w7=0)
        base.update(kw)
        return good_rects[:8] + [base[k] for k in ("HL", "HW", "ignore", "mode", "ai", "aj", "w6", "w7")]

    over = [16384] * 2 * A
    for kw in [dict(drop=k) for k in ("state", "owner", "dist2", "dirs", "rects", "fits", "count", "best", "ws")] + [
            dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(A_=0), dict(A_=33), dict(F_=0), dict(F_=9),
            dict(ub=2), dict(ub=-1), dict(dirs=over[:-1] + [16385]), dict(dirs=[-16385] + over[1:]), dict(rects=second(HL=16385, HW=0)),
            dict(rects=second(HL=-1)), dict(rects=second(HL=16384, HW=1)), dict(rects=second(HL=11586, HW=11585)), dict(rects=second(ignore=128)),
            dict(rects=second(ignore=-1)), dict(rects=second(mode=2)), dict(rects=second(ai=4096)), dict(rects=second(aj=-4097)),
            dict(rects=second(w6=1)), dict(rects=second(w7=1)), dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ws_off)]:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (fits, count, best)) and bool((ws == 0x55).all()) and bool((ws_big == 0x55).all())
    assert call() == 0 and call(dirs=over) == 0 and call(drop="frame") == 0 and call() == 0
    torch.cuda.synchronize()
    got = {"fits": fits.cpu().numpy(), "count": count.cpu().numpy(), "best": best.cpu().numpy()}
    check(got, 1, R.footprint(st, ow, d2, R.direction_table(A), recs, 1), "after the rejected calls")
    dirs = R.direction_table(A)
    for bad in (dict(rects=[]), dict(rects=[R.record(0, 0)] * 9), dict(rects=[R.record(16385, 0)]), dict(rects=[R.record(1, 1, ignore=128)]),
                dict(dirs=np.zeros((33, 2), np.int64)), dict(dirs=np.zeros((0, 2), np.int64)), dict(dirs=dirs * 2), dict(dirs=dirs.reshape(-1))):
        kw = {**dict(dirs=dirs, rects=recs, unknown_blocks=1), **bad}
        with pytest.raises(ValueError):
            footprint.footprint_records(ds, do, dd, None, **kw)
    kw = dict(dirs=dirs, rects=recs, unknown_blocks=1)
    for args in ((ds.cpu(), do, dd, None), (ds, do[:1], dd, None), (ds, do, dd[:, :8], None), (ds[:, :12, :12], do[:, :12, :12], dd[:, :12, :12], None),
                 (ds, do, dd, frame[:1]), (ds, do, dd, frame.int())):
        with pytest.raises(_native.NativeError):
            footprint.footprint_records(*args, **kw)


def test_fit_on_a_placement_result_and_helpers(device):
    from tests import placement_reference as PR
    from unseenobjectclustering_amd import placement, support
    lab, xyz = PR.tabletop(120, 160, 1)
    dl, dx = dev(device, lab), dev(device, xyz)
    fitted = support.fit_plane(dl, dx)
    placed = placement.free_space(dl, dx, fitted, grid=64, cell=0.02)
    st, ow, d2, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "dist2", "frame"))
    assert fr[13] == 1 and (st == 1).sum() > 100 and (st == 2).any()
    a = R.present_id(ow, st)
    mine = footprint.of_object(fitted, 0, a, placed.cell_mm, margin=0.005)
    h = sorted(fitted.half[0, a, :2].cpu().tolist())
    assert mine[2] == a and mine[0] == -(-(int(round((2 * h[1] + 0.01) * 1000)) * 128) // 20) + 184 and mine[0] >= mine[1]
    rects = [footprint.rect(0.20, 0.06, placed.cell_mm), mine, footprint.rect(0.10, 0.04, placed.cell_mm, near=(10, 50), conservative=False)]
    for ub, over in ((True, None), (True, False)):
        res = footprint.fit(placed, rects, angles=16, unknown_blocks=over)
        want_ub = 1 if over is None else 0
        assert res.unknown_blocks == bool(want_ub) and res.angles == 16 and res.rects.tolist() == [list(r) for r in rects]
        got = {k: getattr(res, k).cpu().numpy() for k in ("fits", "count", "best")}
        want = check(got, 0, R.footprint(st, ow, d2, R.direction_table(16), rects, want_ub, fr), ("fit", ub, over))
    assert want["best"][0, 0] == 1 and want["best"][2, 0] == 1
    m = footprint.fits_mask(res, 0)
    assert m.shape == (1, 64, 64) and m.dtype == torch.bool and m.device.type == "cuda"
    assert np.array_equal(m[0].cpu().numpy(), want["fits"][0] != 0)
    assert np.array_equal(footprint.fits_mask(res, 2, 5)[0].cpu().numpy(), (want["fits"][2] >> 5) & 1 != 0)
    p = footprint.pose(res, 0, 0)
    i, j, k = (int(x) for x in want["best"][0, 1:4])
    assert (p.cell, p.k, p.dist2) == ((i, j), k, int(want["best"][0, 4])) and abs(p.angle - np.pi * k / 16) < 1e-15
    assert np.allclose(p.center, placement.cell_to_camera(placed, 0, i, j), rtol=0, atol=1e-12)
    n = fitted.normal[0].cpu().numpy().astype(np.float64)
    assert abs(np.linalg.norm(p.axis) - 1) < 1e-12 and abs(p.axis @ n) < 1e-6
    step = placement.cell_to_camera(placed, 0, i + 1, j) - placement.cell_to_camera(placed, 0, i, j)     # along u
    assert abs(p.axis @ step / np.linalg.norm(step) - np.cos(p.angle)) < 1e-4
    none = footprint.fit(placed, [footprint.rect(1.2, 0.2, placed.cell_mm, conservative=False)])
    assert footprint.pose(none, 0, 0) is None and not bool(footprint.fits_mask(none, 0).any())


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_footprint_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    rects = [footprint.rect(0.30, 0.06, 10), footprint.rect(0.05, 0.05, 10, near=(128, 128))]
    np.random.seed(3)
    out = O.segment_objects(sample, net, net_crop, footprint=True, footprint_args=dict(rects=rects, angles=8))
    assert len(out) == 6                                        # implies placement, which implies the plane
    placed, fitting = out[4], out[5]
    assert hasattr(out[3], "normal") and hasattr(placed, "dist2") and fitting.planes.data_ptr() == placed.planes.data_ptr()
    st, ow, d2, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "dist2", "frame"))
    got = {k: getattr(fitting, k).cpu().numpy() for k in ("fits", "count", "best")}
    check(got, 0, R.footprint(st, ow, d2, R.direction_table(8), rects, 1, fr), "demo")
    with pytest.raises(ValueError):
        O.segment_objects(sample, net, net_crop, footprint=True)
    np.random.seed(3)
    every = O.segment_objects(sample, net, net_crop, elevation=True, footprint=True, footprint_args=dict(rects=rects[:1], unknown_blocks=False))
    assert len(every) == 7 and hasattr(every[5], "elev") and torch.equal(every[4].state, placed.state)
    got = {k: getattr(every[6], k).cpu().numpy() for k in ("fits", "count", "best")}
    check(got, 0, R.footprint(st, ow, d2, R.direction_table(16), rects[:1], 0, fr), "demo, other arguments")
