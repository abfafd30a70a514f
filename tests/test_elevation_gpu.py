"""uoc_elevation / elevation.heights on the GPU against the numpy restatement (tests/elevation_reference.py).

The stage has no floating-point output: every grid, the per-id table, the counters and the answers are compared with
np.array_equal.  The scenes and the engineered frames are generated in the reference modules and
tests/test_elevation_host.py asserts on the CPU that they contain what they are used for here.

Sizes: 5x7 (H*W not a multiple of 4: the scalar path) with G = 8; 48x64 (the vector path, one block) with G = 64 and
with G = 512 on 2 mm cells; 120x160 (five blocks) with G = 64 and with G = 40 (a second strip of the column pass with 8
of its 32 columns); 480x640 with G = 256.

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import ctypes
import faulthandler
import functools
import sys
import types

import numpy as np
import pytest
import torch

from tests import elevation_reference as R
from unseenobjectclustering_amd import _native, elevation, placement, support

pytestmark = pytest.mark.gpu
EINVAL = -22
FULL = (R.BAND[0], R.BAND[1])
KEYS = ("elev", "owner", "pts", "near", "dist2", "tops", "info", "answers")
# (H, W, seed, nobj, G, cell_mm, step_mm, min_pts)
SCENES = [(5, 7, 0, 2, 8, 40, 5, 1), (48, 64, 0, 4, 64, 40, 5, 2), (48, 64, 1, 4, 64, 40, 1, 1), (120, 160, 0, 4, 64, 20, 5, 2),
          (120, 160, 1, 4, 64, 20, 1000, 65535), (120, 160, 2, 4, 64, 20, 1, 1), (480, 640, 1, 5, 256, 10, 5, 2), (48, 64, 2, 4, 512, 2, 5, 2)]


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def scene(H, W, seed, nobj):
    return R.tabletop(H, W, seed, nobj=nobj)


def to_dev(device, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays)


def placed_of(device, frames, G, cell_mm, tau_mm):
    """What heights() reads of a PlacementResult, from host frame records [B,16]."""
    return types.SimpleNamespace(frame=torch.from_numpy(np.ascontiguousarray(np.asarray(frames, np.int64).reshape(-1, 16))).to(device),
                                 grid=G, cell_mm=cell_mm, tau_mm=tau_mm)


def host(res, b):
    return {k: getattr(res, k)[b].cpu().numpy() for k in KEYS}


def check_frame(got, want, where):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k, got[k].dtype, got[k].shape)
        bad = got[k] != want[k]
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[k][bad][:6], want[k][bad][:6])


def scene_queries(cell_mm):
    return [(4, R.ANY, *FULL), (placement.need2(0.03, cell_mm / 1000.0), 1, 20, 200), (1, 0, -10, 10), (1, 2, *FULL), (1, R.ANY, 60, 160)]


TRUE_F = R.frame_record(R.true_plane())


@pytest.mark.parametrize("H,W,seed,nobj,G,cell,step,min_pts", SCENES)
def test_tabletop_scenes_match_reference(device, H, W, seed, nobj, G, cell, step, min_pts):
    lab, xyz = scene(H, W, seed, nobj)
    dl, dx = to_dev(device, lab, xyz)
    qs = scene_queries(cell)
    res = elevation.heights(dl, dx, placed_of(device, TRUE_F, G, cell, 10), step=step / 1000.0, min_pts=min_pts, queries=qs)
    assert res.elev.shape == (1, G, G) and res.tops.shape == (1, 128, 8) and res.info.shape == (1, 4) and res.answers.shape == (1, 5, 4)
    assert res.elev.device.type == "cuda" and (res.step_mm, res.min_pts, res.grid, res.cell_mm, res.tau_mm) == (step, min_pts, G, cell, 10)
    want = R.heights(lab, xyz, TRUE_F, G, cell, 10, step, min_pts, qs)
    assert want["info"][0] == 1 and want["info"][2] > 0
    check_frame(host(res, 0), want, (H, W, seed, G))


def test_partial_strip_of_the_column_pass_matches_reference(device):
    """G = 40: cell_kernel's second strip holds 8 of its 32 columns; the level cells of those columns are asserted in
    tests/test_elevation_host.py."""
    G, cell, tau, step, min_pts = 40, 20, 10, 5, 1
    lab, xyz = scene(120, 160, 1, 5)
    dl, dx = to_dev(device, lab, xyz)
    res = elevation.heights(dl, dx, placed_of(device, TRUE_F, G, cell, tau), step=step / 1000.0, min_pts=min_pts)
    assert res.elev.shape == (1, G, G) and res.answers.shape == (1, 0, 4)
    check_frame(host(res, 0), R.heights(lab, xyz, TRUE_F, G, cell, tau, step, min_pts), "G = 40")


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_cases_match_reference(device, name):
    c = R.ENGINEERED[name]()
    dl, dx = to_dev(device, c["lab"], c["xyz"])
    res = elevation.heights(dl, dx, placed_of(device, c["F"], c["G"], c["cell_mm"], c["tau_mm"]), step=c["step_mm"] / 1000.0,
                            min_pts=c["min_pts"], queries=c["queries"])
    assert res.answers.shape == (1, len(c["queries"]), 4)
    check_frame(host(res, 0), R.run_case(c), name)
    for over in (dict(min_pts=1), dict(min_pts=2), dict(min_pts=65535), dict(step_mm=1), dict(step_mm=6), dict(step_mm=1000),
                 dict(G=8, cell_mm=50), dict(G=64, cell_mm=5, tau_mm=1), dict(queries=[])):
        kw = {k: over.get(k, c[k]) for k in ("G", "cell_mm", "tau_mm", "step_mm", "min_pts", "queries")}
        got = elevation.heights(dl, dx, placed_of(device, c["F"], kw["G"], kw["cell_mm"], kw["tau_mm"]), step=kw["step_mm"] / 1000.0,
                                min_pts=kw["min_pts"], queries=kw["queries"])
        check_frame(host(got, 0), R.run_case(c, **over), (name, over))


def test_unaligned_pointers_label_dtypes_and_unbatched_input(device):
    H, W, seed, nobj, G, cell, step, min_pts = SCENES[1]
    lab, xyz = scene(H, W, seed, nobj)
    dl, dx = to_dev(device, lab, xyz)
    qs = scene_queries(cell)
    pl = placed_of(device, TRUE_F, G, cell, 10)
    a = elevation.heights(dl[None], dx[None], pl, queries=qs)
    check_frame(host(a, 0), R.heights(lab, xyz, TRUE_F, G, cell, 10, 5, 2, qs), "batched")
    for other in (elevation.heights(dl, dx, pl, queries=qs), elevation.heights(dl.float(), dx, pl, queries=qs),
                  elevation.heights(dl.long()[None], dx.double()[None], pl, queries=qs)):
        for k in KEYS:
            assert torch.equal(getattr(a, k), getattr(other, k)), k
    # H*W is a multiple of 4 but the buffers start 4 bytes off a 16-byte boundary: the scalar-load path, the same bits
    n = H * W
    big_l, big_x = torch.zeros(n + 4, dtype=torch.int32, device=device), torch.zeros(3 * n + 4, dtype=torch.float32, device=device)
    big_l[1:n + 1], big_x[1:3 * n + 1] = dl.reshape(-1), dx.reshape(-1)
    ol, ox = big_l[1:n + 1].view(1, H, W), big_x[1:3 * n + 1].view(1, 3, H, W)
    assert ol.data_ptr() % 16 == 4 and ox.data_ptr() % 16 == 4 and ol.is_contiguous() and ox.is_contiguous()
    got = elevation.elevation_records(ol, ox, pl.frame, G, cell, 10, 5, 2, qs)
    for t, k in zip(got, KEYS):
        assert torch.equal(t, getattr(a, k)), k


def test_deterministic_and_batch_independent(device):
    H, W, nobj, G, cell = 120, 160, 4, 64, 20
    frames = [scene(H, W, s, nobj) for s in (0, 1, 2, 3)]
    dl, dx = to_dev(device, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
    qs = scene_queries(cell)
    shifted = {**R.true_plane(), "d": np.float32(R.P.PLANE_D + 0.004)}
    Fs = [TRUE_F, R.frame_record(shifted), TRUE_F, TRUE_F]
    assert Fs[1][13] == 1 and Fs[1][3] != Fs[0][3]

    def same(a, b, rows_a, rows_b, where):
        for k in KEYS:
            assert torch.equal(getattr(a, k)[rows_a], getattr(b, k)[rows_b]), (where, k)

    whole = elevation.heights(dl[:3], dx[:3], placed_of(device, Fs[:3], G, cell, 10), queries=qs)            # B = 3
    same(whole, elevation.heights(dl[:3], dx[:3], placed_of(device, Fs[:3], G, cell, 10), queries=qs), slice(None), slice(None), "rerun")
    order = [3, 2, 0]
    other = elevation.heights(dl[order], dx[order], placed_of(device, [Fs[k] for k in order], G, cell, 10), queries=qs)
    same(whole, other, slice(0, 1), slice(2, 3), "mates")
    for b in range(3):
        alone = elevation.heights(dl[b], dx[b], placed_of(device, Fs[b], G, cell, 10), queries=qs)
        same(whole, alone, slice(b, b + 1), slice(None), ("alone", b))
        check_frame(host(whole, b), R.heights(frames[b][0], frames[b][1], Fs[b], G, cell, 10, 5, 2, qs), ("batch", b))


def test_frames_without_a_plane_next_to_one_with(device):
    c = R.case_two_plateaus()
    cases = [R.case_not_found()["F"], c["F"]] + [b["F"] for b in R.bad_word_cases()] + [np.zeros(16, np.int64)]
    B = len(cases)
    dl, dx = to_dev(device, np.stack([c["lab"]] * B), np.stack([c["xyz"]] * B))
    res = elevation.heights(dl, dx, placed_of(device, cases, c["G"], 10, 10), step=0.005, min_pts=1, queries=c["queries"])
    assert res.info[:, 0].cpu().tolist() == [0, 1] + [0] * (B - 2)
    for b, F in enumerate(cases):
        check_frame(host(res, b), R.heights(c["lab"], c["xyz"], F, c["G"], 10, 10, 5, 1, c["queries"]), ("plane", b))


def test_fitted_plane_through_placement(device):
    H, W, G, cell = 120, 160, 64, 20
    lab, xyz = scene(H, W, 1, 4)
    dl, dx = to_dev(device, lab, xyz)
    fitted = support.fit_plane(dl, dx)
    placed = placement.free_space(dl, dx, fitted, grid=G, cell=cell / 1000.0)
    q = [elevation.on_top(placed, 0.03), elevation.on_top(placed, 0.03, id=1, hmin=0.02), elevation.on_top(placed, 0.0, id=0)]
    res = elevation.heights(dl, dx, placed, queries=q)
    assert res.frame.data_ptr() == placed.frame.data_ptr()                               # the device record, in place
    F = placed.frame[0].cpu().numpy()
    assert F[13] == 1
    want = R.heights(lab, xyz, F, G, cell, placed.tau_mm, 5, 2, q)
    check_frame(host(res, 0), want, "fitted")
    with_top = [a for a in range(5) if want["tops"][a, 1] > 0]
    assert 0 in with_top and len(with_top) >= 3                                         # the table and at least two boxes
    # the two grids coincide: a cell that placement calls an obstacle or table has kept points here (the owner may differ:
    # there the largest id of the cell, here the id of its highest point)
    st = placed.state[0].cpu().numpy()
    assert (want["pts"][st != 0] > 0).all()
    mask = elevation.level_mask(res, 0.03)[0].cpu().numpy()
    assert np.array_equal(mask, want["dist2"] >= q[0][0]) and mask.dtype == bool
    # helpers: spot() and cell_to_camera() round-trip through placement.camera_to_cell
    for a in with_top:
        s = elevation.spot(res, 0, a)
        row = want["tops"][a]
        assert s is not None and s.cell == (int(row[2]), int(row[3])) and s.height_m == row[5] / 1000.0
        assert abs(s.clearance_m - np.sqrt(row[4]) * cell / 1000.0) < 1e-12
        assert placement.camera_to_cell(res, 0, s.xyz) == s.cell == placement.camera_to_cell(placed, 0, s.xyz)
        n = fitted.normal[0].double().cpu().numpy()
        # the height above the fitted plane: qc is the centroid rounded to whole millimetres (at most 0.5 sqrt(3) mm off the
        # plane), N and D are rounded to 2^-14
        assert abs(float(n @ s.xyz + float(fitted.d[0])) - s.height_m) < 1e-3
        p0 = elevation.cell_to_camera(res, 0, *s.cell)
        assert np.allclose(p0, placement.cell_to_camera(placed, 0, *s.cell), rtol=0, atol=1e-3)
    assert elevation.spot(res, 0, 100) is None and all(elevation.spot(res, 0, a) is None for a in range(5) if a not in with_top)


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, H, W, G, Q = 2, 48, 64, 16, 2
    lab, xyz = scene(H, W, 1, 4)
    dl, dx = to_dev(device, np.stack([lab] * B), np.stack([xyz] * B))
    frame = placed_of(device, [TRUE_F] * B, G, 40, 10).frame
    nws = lib.uoc_elevation_workspace_bytes(B, H, W, G)
    shapes = dict(elev=(B, G, G), owner=(B, G, G), pts=(B, G, G), near=(B, G, G), dist2=(B, G, G), tops=(B, 128, 8), info=(B, 4), answers=(B, Q, 4))
    outs = {k: torch.full(s, -7, dtype=torch.int32, device=device) for k, s in shapes.items()}
    ws = torch.full((nws + 16,), 0x55, dtype=torch.uint8, device=device)
    P, st = _native.ptr, _native.stream_ptr(device)
    good_q = [(4, -1, *FULL), (1, 0, -10, 10)]

    def call(G_=G, cell=40, tau=10, step=5, min_pts=2, qs=good_q, Q_=None, ws_=ws, nws_=nws, lab_=dl, xyz_=dx, frame_=frame, B_=B, H_=H, W_=W,
             drop=None, null_q=False):
        hq = (ctypes.c_int32 * (4 * max(len(qs), 1)))(*[x for q in qs for x in q])
        o = {k: (None if k == drop else v) for k, v in outs.items()}
        return lib.uoc_elevation(P(lab_), P(xyz_), P(frame_), B_, H_, W_, G_, cell, tau, step, min_pts,
                                 None if null_q else ctypes.cast(hq, ctypes.c_void_p), len(qs) if Q_ is None else Q_, P(o["elev"]),
                                 P(o["owner"]), P(o["pts"]), P(o["near"]), P(o["dist2"]), P(o["tops"]), P(o["info"]), P(o["answers"]),
                                 P(ws_), nws_, st)

    for kw in [dict(drop=k) for k in shapes] + [
            dict(G_=0), dict(G_=12), dict(G_=520), dict(cell=0), dict(cell=1001), dict(tau=0), dict(tau=1001), dict(step=0), dict(step=1001),
            dict(min_pts=0), dict(min_pts=65536), dict(Q_=-1), dict(Q_=17), dict(null_q=True), dict(ws_=None), dict(nws_=nws - 1),
            dict(ws_=ws[4:]), dict(lab_=None), dict(xyz_=None), dict(frame_=None), dict(B_=0), dict(B_=65536), dict(H_=0), dict(W_=-1),
            dict(H_=1 << 16, W_=1 << 15), dict(qs=[(-1, 0, 0, 0)]), dict(qs=[((1 << 30) + 1, 0, 0, 0)]), dict(qs=[(1, 128, 0, 0)]),
            dict(qs=[(1, -2, 0, 0)]), dict(qs=[(1, 0, 32768, 0)]), dict(qs=[(1, 0, 0, -32769)]), dict(qs=[(1, 0, 0, 0), (1, 0, 0, 40000)])]:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs.values()) and bool((ws == 0x55).all())
    assert call() == 0 and call(qs=[], null_q=True, drop="answers") == 0
    torch.cuda.synchronize()
    want = R.heights(lab, xyz, TRUE_F, G, 40, 10, 5, 2, good_q)
    for b in range(B):
        check_frame({k: outs[k][b].cpu().numpy() for k in KEYS}, want, ("raw", b))
    pl = placed_of(device, [TRUE_F] * B, G, 40, 10)
    for bad in (dict(step=0.0), dict(step=1.5), dict(min_pts=0), dict(queries=[(1, 128, 0, 0)]), dict(queries=[(1, 0, 0, 0)] * 17)):
        with pytest.raises(ValueError):
            elevation.heights(dl, dx, pl, **bad)
    with pytest.raises(_native.NativeError):
        elevation.heights(dl.cpu(), dx, pl)
    with pytest.raises(_native.NativeError):
        elevation.heights(dl, dx[:, :2], pl)
    with pytest.raises(_native.NativeError):
        elevation.heights(dl, dx, placed_of(device, [TRUE_F], G, 40, 10))            # one record for two frames
