"""uoc_placement / placement.free_space on the GPU against the numpy restatement (tests/placement_reference.py).

The feature has no floating-point output: every grid, counter, frame record and answer is compared with np.array_equal.
The scenes and the engineered frames are generated in the reference module and tests/test_placement_host.py asserts on
the CPU that they contain what they are used for here.  The seeded scenes take their plane from support.fit_plane on the
device; the reference reads that record back and restates everything after it.

Sizes: 1x1 and 3x1 (no plane: fewer than three candidates), 24x32 (H*W a multiple of 4: the vector-load path, one
block), 61x83 (odd: the scalar path, two blocks), 224x224 and 480x640; grids 8, 64, 256, 512, and 40 (a second strip of
the column pass with 8 of its 32 columns).

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import faulthandler
import functools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import placement_reference as R
from unseenobjectclustering_amd import _native, placement, support

pytestmark = pytest.mark.gpu
EINVAL = -22

# (G, cell_mm, h_obs_mm, tau_mm, min_pts, unknown_blocks), as in tests/test_placement_host.py
PARAMS = [(64, 10, 10, 10, 1, 1), (256, 10, 10, 10, 1, 1), (256, 5, 20, 8, 3, 0), (64, 50, 10, 10, 3, 1), (8, 50, 20, 8, 1, 0),
          (512, 5, 10, 10, 1, 1)]
COMBOS = {(1, 1): [(1, PARAMS[0])], (3, 1): [(1, PARAMS[4])], (24, 32): [(s, p) for s in (1, 2) for p in PARAMS[:5]],
          (61, 83): [(s, p) for s in (1, 2) for p in PARAMS[:5]], (224, 224): [(1, PARAMS[1]), (2, PARAMS[2])],
          (480, 640): [(1, PARAMS[1]), (2, PARAMS[5])]}


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def scene(H, W, seed):
    return R.tabletop(H, W, seed)


def to_dev(device, lab, xyz):
    return torch.from_numpy(np.ascontiguousarray(lab)).to(device), torch.from_numpy(np.ascontiguousarray(xyz)).to(device)


def kwargs(p, queries=None):
    G, cell, h_obs, tau, min_pts, ub = p
    return dict(grid=G, cell=cell / 1000.0, h_obs=h_obs / 1000.0, tau=tau / 1000.0, min_pts=min_pts, unknown_blocks=bool(ub),
                queries=queries)


def scene_queries(G):
    return [(4, 0, 0, R.WIDEST), (placement.need2(0.03, 0.01), G // 2, G // 2, R.NEAREST), (1, -5, G + 3, R.NEAREST)]


def host(res, b):
    out = {k: getattr(res, k)[b].cpu().numpy() for k in ("state", "owner", "dist2", "frame", "answers")}
    out["counts"] = res.cells[b].cpu().numpy()
    return out


def check_frame(got, want, where):
    for k in R.FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k, got[k].dtype, got[k].shape)
        bad = got[k] != want[k]
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[k][bad][:6], want[k][bad][:6])


def reference(lab, xyz, res, b, p, queries):
    G, cell, h_obs, tau, min_pts, ub = p
    plane = R.plane_from_record(res.planes[b].cpu().numpy())
    return R.free_space(lab, xyz, plane, G, cell, h_obs, tau, min_pts, ub, queries or ())


@pytest.mark.parametrize("H,W", list(COMBOS))
def test_tabletop_scenes_match_reference(device, H, W):
    for seed, p in COMBOS[(H, W)]:
        lab, xyz = scene(H, W, seed)
        dl, dx = to_dev(device, lab, xyz)
        fitted = support.fit_plane(dl, dx)
        qs = scene_queries(p[0])
        res = placement.free_space(dl, dx, fitted, **kwargs(p, qs))
        assert res.state.shape == (1, p[0], p[0]) and res.answers.shape == (1, 3, 4) and res.state.device.type == "cuda"
        assert res.planes.data_ptr() == fitted.records.data_ptr()                 # the device record, in place
        want = reference(lab, xyz, res, 0, p, qs)
        assert int(want["frame"][13]) == (1 if H * W >= 64 else 0)
        check_frame(host(res, 0), want, (H, W, seed, p))
        assert int(res.outside[0]) == want["counts"][0]


def test_partial_strip_of_the_column_pass_matches_reference(device):
    """G = 40: the column pass's second strip holds 8 of its 32 columns and a row segment 5 rows; the obstacles of those
    columns and a column distance longer than a segment are asserted in tests/test_placement_host.py."""
    p, qs, plane = (40, 10, 10, 10, 1, 0), [(4, 0, 0, R.WIDEST)], R.true_plane()
    lab, xyz = scene(61, 83, 1)
    dl, dx = to_dev(device, lab, xyz)
    res = placement.free_space(dl, dx, tuple(plane[k] for k in ("normal", "d", "centroid", "u", "v")), **kwargs(p, qs))
    assert res.state.shape == (1, 40, 40) and res.answers.shape == (1, 1, 4)
    check_frame(host(res, 0), R.free_space(lab, xyz, plane, *p, qs), "G = 40")


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_cases_match_reference(device, name):
    c = R.ENGINEERED[name]()
    dl, dx = to_dev(device, c["lab"], c["xyz"])
    plane = tuple(c["plane"][k] for k in ("normal", "d", "centroid", "u", "v"))
    base = (c["G"], c["cell_mm"], c["h_obs_mm"], c["tau_mm"], c["min_pts"], 1)
    res = placement.free_space(dl, dx, plane, **kwargs(base, c["queries"]))
    assert res.answers.shape == (1, len(c["queries"]), 4)
    check_frame(host(res, 0), R.run_case(c), name)
    for over in (dict(unknown_blocks=0), dict(min_pts=2, unknown_blocks=0), dict(G=8, cell_mm=50), dict(G=64, cell_mm=5, h_obs_mm=0, tau_mm=1),
                 dict(queries=[])):
        p = tuple(over.get(k, v) for k, v in zip(("G", "cell_mm", "h_obs_mm", "tau_mm", "min_pts", "unknown_blocks"), base))
        qs = over.get("queries", c["queries"])
        check_frame(host(placement.free_space(dl, dx, plane, **kwargs(p, qs)), 0), R.run_case(c, **over), (name, over))


def records(device, planes):
    """Plane records [B,21] on the device from reference-style plane dicts (found is taken as given)."""
    rec = np.concatenate([placement.pack_planes(*(p[k] for k in ("normal", "d", "centroid", "u", "v"))) for p in planes])
    rec[:, 0] = [p["found"] for p in planes]
    return types.SimpleNamespace(records=torch.from_numpy(rec).to(device))


def test_frames_without_a_plane_next_to_one_with(device):
    c = R.case_single_block()
    nan_plane = {**R.flat_plane(), "normal": np.array([0, np.nan, -1], np.float32)}
    far_plane = {**R.flat_plane(), "centroid": np.array([0, 0, 40.0], np.float32)}
    shifted = {**R.flat_plane(), "d": np.float32(1.004), "centroid": np.array([0.013, -0.02, 1.004], np.float32)}
    planes = [R.flat_plane(found=0), c["plane"], nan_plane, shifted, R.flat_plane(found=2), far_plane]
    dl, dx = to_dev(device, np.stack([c["lab"]] * len(planes)), np.stack([c["xyz"]] * len(planes)))
    p = (c["G"], c["cell_mm"], c["h_obs_mm"], c["tau_mm"], 1, 1)
    res = placement.free_space(dl, dx, records(device, planes), **kwargs(p, c["queries"]))
    found = res.frame[:, 13].cpu().tolist()
    assert found == [0, 1, 0, 1, 0, 0]
    for b, plane in enumerate(planes):
        check_frame(host(res, b), R.free_space(c["lab"], c["xyz"], plane, *p, c["queries"]), ("plane", b))
    for b in (0, 2, 4, 5):
        assert not any(bool(getattr(res, k)[b].any()) for k in ("state", "owner", "dist2", "cells", "frame"))
        assert res.answers[b].cpu().tolist() == [list(R.NO_ANSWER)] * 16


def test_label_dtypes_unbatched_input_and_unaligned_pointers(device):
    lab, xyz = scene(24, 32, 1)
    dl, dx = to_dev(device, lab, xyz)
    plane = tuple(R.true_plane()[k] for k in ("normal", "d", "centroid", "u", "v"))
    kw = kwargs(PARAMS[0], scene_queries(64))
    a = placement.free_space(dl[None], dx[None], plane, **kw)
    check_frame(host(a, 0), R.free_space(lab, xyz, R.true_plane(), *PARAMS[0], kw["queries"]), "uploaded plane")
    for other in (placement.free_space(dl, dx, plane, **kw), placement.free_space(dl.float(), dx, plane, **kw),
                  placement.free_space(dl.long()[None], dx.double()[None], plane, **kw)):
        for k in ("state", "owner", "dist2", "cells", "frame", "answers"):
            assert torch.equal(getattr(a, k), getattr(other, k)), k
    # H*W is a multiple of 4 but the buffers start 4 bytes off a 16-byte boundary: the scalar-load path, the same bits
    n = 24 * 32
    big_l, big_x = torch.zeros(n + 4, dtype=torch.int32, device=device), torch.zeros(3 * n + 4, dtype=torch.float32, device=device)
    big_l[1:n + 1], big_x[1:3 * n + 1] = dl.reshape(-1), dx.reshape(-1)
    ol, ox = big_l[1:n + 1].view(1, 24, 32), big_x[1:3 * n + 1].view(1, 3, 24, 32)
    assert ol.data_ptr() % 16 == 4 and ox.data_ptr() % 16 == 4 and ol.is_contiguous() and ox.is_contiguous()
    got = placement.placement_records(ol, ox, a.planes, 64, 10, 10, 10, 1, 1, kw["queries"])
    for t, k in zip(got, ("state", "owner", "dist2", "cells", "frame", "answers")):
        assert torch.equal(t, getattr(a, k)), k


def test_deterministic_and_batch_independent(device):
    frames = [scene(61, 83, 1), scene(61, 83, 2), scene(61, 83, 3), scene(61, 83, 4)]
    dl, dx = to_dev(device, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
    p = PARAMS[1]
    kw = kwargs(p, scene_queries(p[0]))
    keys = ("state", "owner", "dist2", "cells", "frame", "answers")

    def same(a, b, rows_a, rows_b, where):
        for k in keys:
            assert torch.equal(getattr(a, k)[rows_a], getattr(b, k)[rows_b]), (where, k)

    fit3 = support.fit_plane(dl[:3], dx[:3])
    whole = placement.free_space(dl[:3], dx[:3], fit3, **kw)                      # B = 3
    same(whole, placement.free_space(dl[:3], dx[:3], fit3, **kw), slice(None), slice(None), "rerun")
    order = [3, 2, 0]
    other = placement.free_space(dl[order], dx[order], support.fit_plane(dl[order], dx[order]), **kw)      # frame 0 among other mates
    same(whole, other, slice(0, 1), slice(2, 3), "mates")
    for b in range(3):
        alone = placement.free_space(dl[b], dx[b], support.fit_plane(dl[b], dx[b]), **kw)
        same(whole, alone, slice(b, b + 1), slice(None), ("alone", b))
        check_frame(host(whole, b), reference(frames[b][0], frames[b][1], whole, b, p, kw["queries"]), ("batch", b))


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, H, W, G, Q = 2, 24, 32, 16, 2
    lab, xyz = to_dev(device, np.stack([scene(H, W, 1)[0]] * B), np.stack([scene(H, W, 1)[1]] * B))
    planes = records(device, [R.true_plane()] * B).records
    nws = lib.uoc_placement_workspace_bytes(B, H, W, G)
    wsb = lib.uoc_placement_workspace_bytes
    assert nws > 0 and wsb(0, H, W, G) == 0 and wsb(B, 0, W, G) == 0 and wsb(65536, H, W, G) == 0 and wsb(1, 1 << 16, 1 << 15, G) == 0
    assert wsb(1, (1 << 31) - 1, 1, G) > 0 and wsb(B, H, W, 0) == 0 and wsb(B, H, W, 12) == 0 and wsb(B, H, W, 520) == 0 and wsb(B, H, W, 512) > 0
    outs = {k: torch.full(shape, -7, dtype=dt, device=device)
            for k, shape, dt in (("state", (B, G, G), torch.int32), ("owner", (B, G, G), torch.int32), ("dist2", (B, G, G), torch.int32),
                                 ("counts", (B, 128), torch.int32), ("frame", (B, 16), torch.int64), ("answers", (B, Q, 4), torch.int32))}
    ws = torch.full((nws,), 0x55, dtype=torch.uint8, device=device)
    P, st = _native.ptr, _native.stream_ptr(device)
    import ctypes
    good_q = [(4, 0, 0, 0), (1, 3, 3, 1)]

    def call(G_=G, cell=10, h_obs=10, tau=10, min_pts=1, ub=1, qs=good_q, Q_=None, ws_=ws, nws_=nws, lab_=lab, xyz_=xyz, planes_=planes,
             B_=B, H_=H, W_=W, drop=None, null_q=False):
        hq = (ctypes.c_int32 * (4 * max(len(qs), 1)))(*[x for q in qs for x in q])
        o = {k: (None if k == drop else v) for k, v in outs.items()}
        return lib.uoc_placement(P(lab_), P(xyz_), P(planes_), B_, H_, W_, G_, cell, h_obs, tau, min_pts, ub,
                                 None if null_q else ctypes.cast(hq, ctypes.c_void_p), len(qs) if Q_ is None else Q_, P(o["state"]),
                                 P(o["owner"]), P(o["dist2"]), P(o["counts"]), P(o["frame"]), P(o["answers"]), P(ws_), nws_, st)

    for kw in (dict(G_=0), dict(G_=12), dict(G_=520), dict(G_=-8), dict(cell=0), dict(cell=1001), dict(h_obs=-1), dict(h_obs=1001),
               dict(tau=0), dict(tau=1001), dict(min_pts=0), dict(min_pts=65536), dict(ub=2), dict(ub=-1), dict(Q_=-1), dict(Q_=17),
               dict(null_q=True), dict(drop="answers"), dict(drop="state"), dict(drop="owner"), dict(drop="dist2"), dict(drop="counts"),
               dict(drop="frame"), dict(ws_=None), dict(nws_=nws - 1), dict(lab_=None), dict(xyz_=None), dict(planes_=None), dict(B_=0),
               dict(B_=65536), dict(H_=0), dict(W_=-1), dict(H_=1 << 16, W_=1 << 15), dict(qs=[(-1, 0, 0, 0)]), dict(qs=[((1 << 30) + 1, 0, 0, 0)]),
               dict(qs=[(1, 4096, 0, 1)]), dict(qs=[(1, 0, -4097, 1)]), dict(qs=[(1, 0, 0, 2)]), dict(qs=[(1, 0, 0, 0), (1, 0, 0, -1)])):
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs.values()) and bool((ws == 0x55).all())
    assert call() == 0 and call(qs=[], null_q=True, drop="answers") == 0
    torch.cuda.synchronize()
    assert int(outs["state"].min()) == 0 and int(outs["frame"][0, 13]) == 1 and torch.equal(outs["state"][0], outs["state"][1])
    plane = tuple(R.true_plane()[k] for k in ("normal", "d", "centroid", "u", "v"))
    for bad in (dict(grid=12), dict(grid=1024), dict(cell=0.0), dict(cell=1.5), dict(h_obs=-0.001), dict(tau=0.0), dict(min_pts=0),
                dict(queries=[(1, 0, 0, 2)]), dict(queries=[(1, 0, 0, 0)] * 17), dict(queries=[(1, 5000, 0, 1)])):
        with pytest.raises(ValueError):
            placement.free_space(lab, xyz, plane, **bad)
    with pytest.raises(_native.NativeError):
        placement.free_space(lab.cpu(), xyz, plane)
    with pytest.raises(_native.NativeError):
        placement.free_space(lab, xyz[:, :2], plane)
    with pytest.raises(_native.NativeError):
        placement.free_space(lab, xyz, support.fit_plane(lab[:1], xyz[:1]))      # one record for two frames


def test_helpers_round_trip(device):
    lab, xyz = scene(61, 83, 1)
    dl, dx = to_dev(device, lab, xyz)
    fitted = support.fit_plane(dl, dx)
    res = placement.free_space(dl, dx, fitted)
    st = res.state[0].cpu().numpy()
    i, j = (int(v[0]) for v in np.nonzero(st == 1))
    p = placement.cell_to_camera(res, 0, i, j)
    assert placement.camera_to_cell(res, 0, p) == (i, j)                          # a cell's centre lies in the cell
    assert abs(float(fitted.normal[0].double().cpu().numpy() @ p + float(fitted.d[0]))) < 1e-5      # and on the plane
    assert placement.camera_to_cell(res, 0, (0.0, 0.0, -1.0)) is None
    q = [placement.widest(res, 0.03), placement.nearest(res, 0.03, p)]
    assert q[0] == (16, 0, 0, 0) and q[1] == (16, i, j, 1)
    again = placement.free_space(dl, dx, fitted, queries=q)
    want = reference(lab, xyz, again, 0, PARAMS[1], q)
    check_frame(host(again, 0), want, "helpers")
    mask = placement.free_mask(again, 0.03)[0].cpu().numpy()
    assert np.array_equal(mask, (want["state"] == 1) & (want["dist2"] >= 16)) and mask.any() == bool(want["answers"][0, 3])


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_placement_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out0, ref0, objs0 = O.segment_objects(sample, net, net_crop)
    np.random.seed(3)
    qs = [(36, 0, 0, R.WIDEST)]
    out1, ref1, objs1, fitted, placed = O.segment_objects(sample, net, net_crop, placement=True, placement_args=dict(queries=qs))
    assert torch.equal(out0, out1) and ref0 is not None and torch.equal(ref0, ref1) and torch.equal(objs0.centroid, objs1.centroid)
    assert hasattr(fitted, "normal") and int(fitted.found[0]) == 1 and placed.planes.data_ptr() == fitted.records.data_ptr()
    lab, xyz = ref1[0].numpy().astype(np.int32), sample["depth"][0].numpy()
    want = reference(lab, xyz, placed, 0, PARAMS[1], qs)
    check_frame(host(placed, 0), want, "demo")
    assert (want["state"] == 1).sum() > 100 and (want["state"] == 2).any() and want["answers"][0, 0] >= 0
    np.random.seed(3)
    every = O.segment_objects(sample, net, net_crop, plane=True, relations=True, placement=True)
    assert len(every) == 6 and hasattr(every[4], "front") and torch.equal(every[5].state, placed.state)
