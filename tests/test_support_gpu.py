"""uoc_support_plane / support.fit_plane on the GPU against the numpy restatement (tests/support_reference.py).

Steps A and B are exact integers: found, candidates, inliers, hyp and the object counts are compared with np.array_equal.
Steps C and D are fp64 sums stored in fp32, compared with the tolerances of tests/test_objects_gpu.py: centroid, foot and
heights within 2e-6 m, covariances and eigenvalues within 1e-6 + 1e-5*l0, and, where the relevant eigen-gap is at least
1e-3 of the largest eigenvalue, normal / u / v / axis by dot >= 1 - 1e-5 and half / center within 1e-5 m.

Beside those, and without exemption, every found plane and every object with at least one valid point goes through the
gap-independent checker of tests/stats_cases.py (plane_metrics, plane_object_metrics): (u, v, normal) orthonormal and
right-handed with v = normal x u, d >= 0, eigenvalues descending and never negative, rms^2 against eig[2], the residual of
the normal against the reference's fp64 covariance, the centroid within half a float32 ulp plus the fp64 accumulation
bound, and d, the heights, foot, cov2, the 2x2 axis (unit, sign rule, residual), half and center against their fp64
recomputation from the stored float32 plane, with every point inside the upright box; and d, the height map, height_min,
height_max, foot and cov2 against the reference itself within half a float32 ulp plus the fp64 accumulation bound plus
what the normal's fp64 uncertainty (solver error over the eigen-gap) moves them by (plane_reference_metrics).  Each bound is
derived there.  One judgement is left open: the sign rule is checked only where the stored float32 vector decides it (a
tie of mixed signs within 2^-22 of the largest component is decided by fp64 bits the record does not hold; the exact
45-degree cases cover it), and a plane whose d is below its own uncertainty has no reference orientation.  The exact
cases are in tests/test_stats_cases_gpu.py.

The scenes are generated in the reference module (seeded) and tests/test_support_host.py asserts on the CPU that they
contain what they are used for here (tied top scores, engineered degeneracies).

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import faulthandler
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import stats_cases as S
from tests import support_reference as R
from unseenobjectclustering_amd import _native, support

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22

# (seed, tau_mm, num_hyp) per size: the whole grid {1, 2} x {3, 10} x {1, 64, 256, 1024} where the reference takes
# milliseconds, a covering subset at the two large sizes (the reference costs M * num_hyp integer dot products)
GRID = [(s, t, n) for s in (1, 2) for t in (3, 10) for n in (1, 64, 256, 1024)]
COMBOS = {(480, 640): [(1, 10, 256), (2, 3, 64), (2, 10, 1)], (224, 224): [(1, 10, 1024), (2, 3, 256), (1, 3, 1)],
          (61, 83): GRID, (24, 32): GRID, (3, 1): GRID[::3], (1, 1): GRID[::5]}
PLANE_FLOATS = ("normal", "d", "centroid", "eig", "rms", "u", "v")
OBJECT_FLOATS = ("height_min", "height_max", "foot", "cov2", "axis", "half", "center")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def noise_for(tau_mm):
    return 0.0015 if tau_mm == 3 else 0.0005


@functools.lru_cache(maxsize=None)
def scene(H, W, seed, noise):
    return R.tabletop(H, W, seed, noise=noise)


@functools.lru_cache(maxsize=None)
def scene_reference(H, W, seed, tau_mm, num_hyp):
    lab, xyz = scene(H, W, seed, noise_for(tau_mm))
    return R.fit(lab, xyz, num_hyp, tau_mm, seed, height_map=True)


def to_dev(device, lab, xyz):
    return torch.from_numpy(np.ascontiguousarray(lab)).to(device), torch.from_numpy(np.ascontiguousarray(xyz)).to(device)


def host(res, b):
    f = {k: getattr(res, k)[b].cpu().numpy() for k in support.PLANE_FIELDS + support.OBJECT_FIELDS}
    f["height"] = None if res.height is None else res.height[b].cpu().numpy()
    return f


def check_frame(got, want, where):
    """got: host(res, b); want: R.fit(...).  Returns (plane gap ok, objects present, objects with their gap ok)."""
    p = want["plane"]
    for k in support.PLANE_INT_FIELDS:
        assert int(got[k]) == p[k], (where, k, int(got[k]), p[k])
    counts = np.zeros(128, np.int64)
    for l, o in want["objects"].items():
        counts[l] = o["count"]
    assert np.array_equal(got["count"], counts), where
    if got["height"] is not None:
        assert np.array_equal(np.isnan(got["height"]), np.isnan(want["height"])), where
    if not p["found"]:
        for k in PLANE_FLOATS + OBJECT_FLOATS:
            assert not np.any(got[k]), (where, k)
        assert got["height"] is None or np.isnan(got["height"]).all(), where
        return False, 0, 0
    l0 = float(p["eig"][0])
    assert np.abs(got["centroid"] - p["centroid"]).max() <= 2e-6, where
    assert np.abs(got["eig"] - p["eig"]).max() <= 1e-6 + 1e-5 * l0, where
    assert abs(float(got["rms"]) ** 2 - p["eig"][2]) <= 1e-6 + 1e-5 * l0, where
    # whatever the eigen-gaps: the properties and derived bounds of tests/stats_cases.py
    S.assert_metrics(S.plane_metrics(got, p["points"], p), where)
    S.assert_metrics(S.plane_reference_metrics(got, want), where)      # half an ulp + gamma + the normal's fp64 uncertainty
    plane_ok = l0 > 0 and p["eig"][1] - p["eig"][2] >= 1e-3 * l0
    if plane_ok:
        for k in ("normal", "u", "v"):
            assert float(got[k].astype(np.float64) @ p[k]) >= 1 - 1e-5, (where, k, got[k], p[k])
        assert abs(float(got["d"]) - p["d"]) <= 2e-6, (where, float(got["d"]), p["d"])
    if got["height"] is not None:
        m = ~np.isnan(want["height"])
        print(where, "height err", float(np.abs(got["height"][m] - want["height"][m]).max()) if m.any() else 0.0)
        assert not m.any() or np.abs(got["height"][m] - want["height"][m]).max() <= 2e-6, where
        if m.any() and "xyz" in want:
            S.assert_metrics(S.height_metrics(got["height"][m], got, want["xyz"].reshape(3, -1).T[m.reshape(-1)]), where)
    axes_ok = 0
    for l in range(128):
        o = want["objects"].get(l)
        if o is None:
            for k in OBJECT_FLOATS:
                assert not np.any(got[k][l]), (where, l, k)
            continue
        S.assert_metrics(S.plane_object_metrics({k: got[k][l] for k in OBJECT_FLOATS}, got, o["points"]), (where, l))
        assert abs(got["height_min"][l] - o["height_min"]) <= 2e-6 and abs(got["height_max"][l] - o["height_max"]) <= 2e-6, (where, l)
        assert np.abs(got["foot"][l] - o["foot"]).max() <= 2e-6, (where, l)
        assert np.abs(got["cov2"][l] - o["cov2"]).max() <= 1e-6 + 1e-5 * o["lam0"], (where, l)
        if o["gap"] == 0:
            assert np.array_equal(got["axis"][l], [1.0, 0.0]), (where, l)
        if plane_ok and o["lam0"] > 0 and o["gap"] >= 1e-3 * o["lam0"]:
            assert float(got["axis"][l].astype(np.float64) @ o["axis"]) >= 1 - 1e-5, (where, l, got["axis"][l], o["axis"])
            assert np.abs(got["half"][l] - o["half"]).max() <= 1e-5, (where, l)
            assert np.abs(got["center"][l] - o["center"]).max() <= 1e-5, (where, l)
            axes_ok += 1
    return plane_ok, len(want["objects"]), axes_ok


@pytest.mark.parametrize("H,W", list(COMBOS))
def test_tabletop_scenes_match_reference(device, H, W):
    planes = planes_ok = objects = objects_ok = 0
    for seed, tau_mm, num_hyp in COMBOS[(H, W)]:
        lab, xyz = scene(H, W, seed, noise_for(tau_mm))
        dl, dx = to_dev(device, lab, xyz)
        res = support.fit_plane(dl, dx, num_hyp=num_hyp, tau=tau_mm / 1000.0, seed=seed, height_map=True)
        assert res.found.dtype == res.count.dtype == torch.int32 and res.normal.shape == (1, 3) and res.half.shape == (1, 128, 3)
        want = scene_reference(H, W, seed, tau_mm, num_hyp)
        ok, n, n_ok = check_frame(host(res, 0), want, (H, W, seed, tau_mm, num_hyp))
        planes += want["plane"]["found"]
        planes_ok += bool(ok)
        objects += n
        objects_ok += n_ok
    if H * W >= 24 * 32:
        assert planes >= len(COMBOS[(H, W)]) - 2 and objects > 0          # a single hypothesis may be degenerate
    else:
        assert planes == 0                                              # fewer than three candidates
    assert 2 * planes_ok >= planes and 2 * objects_ok >= objects, (planes, planes_ok, objects, objects_ok)


def test_label_dtypes_and_unbatched_input(device):
    lab, xyz = scene(61, 83, 1, 0.0005)
    dl, dx = to_dev(device, lab, xyz)
    a = support.fit_plane(dl[None], dx[None], num_hyp=64)
    for other in (support.fit_plane(dl, dx, num_hyp=64), support.fit_plane(dl.float(), dx, num_hyp=64),
                  support.fit_plane(dl.long()[None], dx.double()[None], num_hyp=64)):
        for k in support.PLANE_FIELDS + support.OBJECT_FIELDS:
            assert torch.equal(getattr(a, k), getattr(other, k)), k
    assert a.height is None


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_cases_match_reference(device, name):
    lab, xyz = R.ENGINEERED[name]()
    dl, dx = to_dev(device, lab, xyz)
    for seed, tau_mm, num_hyp in ((1, 10, 64), (2, 3, 256), (7, 10, 1)):
        res = support.fit_plane(dl, dx, num_hyp=num_hyp, tau=tau_mm / 1000.0, seed=seed, height_map=True)
        want = R.fit(lab, xyz, num_hyp, tau_mm, seed, height_map=True)
        got = host(res, 0)
        check_frame(got, want, (name, seed, tau_mm, num_hyp))
        if name in ("m0", "m2", "collinear", "coincident", "all_objects"):
            assert int(got["found"]) == 0
        if name == "origin_plane":
            assert int(got["found"]) == 1 and float(got["d"]) == 0.0 and np.array_equal(got["normal"], [1.0, 0.0, 0.0])
            assert np.array_equal(got["u"], [0.0, 1.0, 0.0]) and np.array_equal(got["v"], [0.0, 0.0, 1.0])
        if name == "nasty" and num_hyp > 1:
            assert int(got["found"]) == 1 and got["count"][50] == 1 and got["count"][51] == 0
            assert not np.any(got["half"][50]) and not np.any(got["cov2"][50]) and got["height_min"][50] == got["height_max"][50]


def test_deterministic_and_batch_independent(device):
    frames = [scene(61, 83, s, n) for s, n in ((1, 0.0005), (2, 0.0005), (1, 0.0015), (2, 0.0015))] + [R.case_all_objects(61, 83)]
    labs, xyzs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    fields = support.PLANE_FIELDS + support.OBJECT_FIELDS + ("height",)

    def same(a, b, rows_a, rows_b, where):
        for k in fields:
            x, y = getattr(a, k)[rows_a].view(torch.int32), getattr(b, k)[rows_b].view(torch.int32)      # bits: NaN == NaN
            assert torch.equal(x, y), (where, k)

    dl, dx = to_dev(device, labs, xyzs)
    kw = dict(num_hyp=256, tau=0.003, seed=5, height_map=True)
    whole = support.fit_plane(dl[:4], dx[:4], **kw)
    same(whole, support.fit_plane(dl[:4], dx[:4], **kw), slice(None), slice(None), "rerun")
    other = support.fit_plane(dl[[4, 3, 0, 1]], dx[[4, 3, 0, 1]], **kw)              # frame 0 with different mates
    same(whole, other, slice(0, 1), slice(2, 3), "mates")
    for b in range(4):
        same(whole, support.fit_plane(dl[b], dx[b], **kw), slice(b, b + 1), slice(None), ("alone", b))
    assert int(other.found[0]) == 0 and bool(torch.isnan(other.height[0]).all()) and int(whole.found.sum()) == 4


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, H, W = 1, 24, 32
    lab, xyz = to_dev(device, *scene(H, W, 1, 0.0005))
    nws = lib.uoc_plane_workspace_bytes(B, H, W, 64)
    assert nws > 0 and lib.uoc_plane_workspace_bytes(B, H, W, 0) == 0 and lib.uoc_plane_workspace_bytes(B, H, W, 1025) == 0
    assert lib.uoc_plane_workspace_bytes(0, H, W, 64) == 0 and lib.uoc_plane_workspace_bytes(B, 1 << 16, 1 << 16, 64) == 0
    planes = torch.full((B, support._PW), -7, dtype=torch.int32, device=device)
    objs = torch.full((B, 128, support._OW), -7, dtype=torch.int32, device=device)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    P, st = _native.ptr, _native.stream_ptr(device)

    def call(num_hyp=64, tau_mm=10, planes_=planes, objs_=objs, ws_=ws, nws_=nws, lab_=lab):
        return lib.uoc_support_plane(P(lab_), P(xyz), B, H, W, num_hyp, tau_mm, 1, P(planes_), P(objs_), None, P(ws_), nws_, st)

    for kw in (dict(num_hyp=0), dict(num_hyp=1025), dict(tau_mm=0), dict(tau_mm=1001), dict(nws_=nws - 1), dict(planes_=None),
               dict(objs_=None), dict(ws_=None), dict(lab_=None)):
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert bool((planes == -7).all()) and bool((objs == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(planes[0, 0]) == 1
    with pytest.raises(ValueError):
        support.fit_plane(lab, xyz, num_hyp=0)
    with pytest.raises(ValueError):
        support.fit_plane(lab, xyz, tau=0.0)
    with pytest.raises(_native.NativeError):
        support.fit_plane(lab.cpu(), xyz)


def test_standing_objects_and_drop_flat(device):
    lab, xyz = scene(61, 83, 1, 0.0005)
    lab = lab.copy()
    lab[-3:, :5] = 99                                  # a patch of the table itself: an "object" a few millimetres high
    lab[0, 0] = 128
    dl, dx = to_dev(device, lab, xyz)
    res = support.fit_plane(dl, dx, num_hyp=64)
    hmax, cnt = res.height_max[0].cpu().numpy(), res.count[0].cpu().numpy()
    assert cnt[99] > 0 and hmax[99] < 0.01 and (hmax[1:7] > 0.03).all()
    standing = support.standing_objects(res, 0.02)
    assert standing.shape == (1, 128) and standing.dtype == torch.bool
    assert np.array_equal(standing[0].cpu().numpy(), (hmax >= 0.02) & (cnt > 0))
    out = support.drop_flat(dl, res, 0.02)
    want = lab.copy()
    want[lab == 99] = 0
    assert out.device == dl.device and out.dtype == dl.dtype and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(support.drop_flat(dl[None].float(), res, 0.02).cpu().numpy(), want[None].astype(np.float32))


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_plane_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out0, ref0, objs0 = O.segment_objects(sample, net, net_crop)
    np.random.seed(3)
    out1, ref1, objs1, res = O.segment_objects(sample, net, net_crop, plane=True, plane_args=dict(height_map=True))
    assert torch.equal(out0, out1) and ref0 is not None and torch.equal(ref0, ref1)
    assert torch.equal(objs0.centroid, objs1.centroid) and torch.equal(objs0.points, objs1.points)
    lab, xyz = ref1[0].numpy().astype(np.int32), sample["depth"][0].numpy()
    want = R.fit(lab, xyz, 256, 10, 1, height_map=True)
    assert want["plane"]["found"] == 1 and len(want["objects"]) >= 1
    check_frame(host(res, 0), want, "demo")
    assert np.array_equal(np.nonzero(res.count[0].cpu().numpy())[0], objs1.label.cpu().numpy())


BASE_KEYS = {"frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
             "obb_center", "obb_half", "offsets", "points", "pixel_index", "label_map"}
PLANE_KEYS = {"plane_" + k for k in ("found", "candidates", "inliers", "hyp", "normal", "d", "centroid", "eig", "rms", "u", "v")} | \
    {"height_min", "height_max", "foot", "cov2", "upright_axis", "upright_half", "upright_center"}


def test_export_objects_plane_cli(device, golden_dir, tmp_path):
    def export(out, *flags):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_objects.py"), "--imgdir",
                            os.path.join(golden_dir, "demo"), "--out", str(out), "--max-points", "500", *flags],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.load(out / "000002_objects.npz")

    plain = export(tmp_path / "plain")
    assert set(plain.files) == BASE_KEYS
    z = export(tmp_path / "plane", "--plane", "--min-height", "0.02")
    assert set(z.files) == BASE_KEYS | PLANE_KEYS | {"standing"}
    for k in BASE_KEYS:
        assert np.array_equal(plain[k], z[k]), k
    K = len(z["label"])
    assert int(z["plane_found"]) == 1 and z["plane_normal"].shape == (3,) and z["height_max"].shape == (K,)
    assert z["upright_center"].shape == (K, 3) and np.array_equal(z["standing"], z["height_max"] >= np.float32(0.02))
    want = R.fit(z["label_map"], _demo(golden_dir)[0]["depth"][0].numpy(), 256, 10, 1)
    assert int(z["plane_hyp"]) == want["plane"]["hyp"] and int(z["plane_inliers"]) == want["plane"]["inliers"]
    for row, l in enumerate(z["label"]):
        assert abs(z["height_max"][row] - want["objects"][int(l)]["height_max"]) <= 2e-6
