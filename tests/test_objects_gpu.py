"""uoc_objects / extract_objects on the GPU against the float64 numpy restatement (tests/objects_reference.py).

Integer fields, AABBs, packed points, attributes and pixel indices are copies or order-free reductions: exact.  The float
statistics are fp64 sums stored in fp32: centroid within 2e-6 m, cov within 1e-6 m^2 + 1e-5*l0, eigenvalues within
1e-5*l0 + 1e-9, and where both eigen-gaps are >= 1e-3*l0, axes |dot| >= 1 - 1e-5 with the same sign and the OBB within 1e-5 m.

Beside those, and without exemption, every object with at least one valid point goes through the gap-independent checker
of tests/stats_cases.py (object_metrics): axes orthonormal and right-handed, eigenvalues descending and never negative,
the sign rule, the residual |C a_k - eig_k a_k| of every stored pair against the reference's fp64 covariance, centroid
and cov within half a float32 ulp plus the fp64 accumulation bound, and the box against the extents recomputed from the
stored centroid and axes, with every point inside it; each bound is derived there from n, the magnitudes and the
roundings.  One judgement is left open: the sign rule is checked only where the stored float32 vector decides it; a tie of
mixed signs within 2^-22 of the largest component is decided by fp64 bits the record does not hold, and the exact
45-degree cases cover it.  The exact cases are in tests/test_stats_cases_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import objects_reference as R
from tests import stats_cases as S
from unseenobjectclustering_amd import _native, io as uio, networks, synth
from unseenobjectclustering_amd import objects as O
from unseenobjectclustering_amd.fcn import test_dataset as TD
from unseenobjectclustering_amd.fcn.config import cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic(B, H, W, seed, ids="all", corrupt=0.05):
    """labels [B,H,W] int32 with ids 1..127 in tiles (every id for large frames, or every other id with ids='gaps'),
    2 % out-of-range ids (0, 128, -1, 1000, -7); xyz [B,3,H,W] float32 of a tilted noisy surface with `corrupt` of the z
    values set to 0, negative, NaN or inf (and a few NaN x); attrs [B,2,H,W]."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    lab = np.zeros((B, H, W), np.int32)
    xyz = np.zeros((B, 3, H, W), np.float32)
    for b in range(B):
        t = max(1, min(H, W) // 16)
        tile = (ys // t) * (W // t + 1) + xs // t + b * 5
        if ids == "gaps":
            lab[b] = (tile * 2) % 126 + 1
        else:
            lab[b] = tile % 127 + 1
        bad = rng.random((H, W)) < 0.02
        lab[b][bad] = rng.choice(np.array([0, 128, -1, 1000, -7], np.int32), size=int(bad.sum()))
        z = (0.6 + 0.3 * xs / max(W, 1) + 0.2 * ys / max(H, 1) + 0.01 * rng.standard_normal((H, W))).astype(np.float32)
        xyz[b, 0] = (xs - W / 2) * z / 600.0
        xyz[b, 1] = (ys - H / 2) * z / 600.0 + 0.001 * rng.standard_normal((H, W))
        xyz[b, 2] = z
        c = rng.random((H, W)) < corrupt
        xyz[b, 2][c] = rng.choice(np.array([0.0, -0.5, np.nan, np.inf], np.float32), size=int(c.sum()))
        xyz[b, 0][rng.random((H, W)) < 0.002] = np.nan
    attrs = rng.random((B, 2, H, W)).astype(np.float32)
    return lab, xyz, attrs


def check_against_reference(objs, lab, xyz, attrs=None, max_points=None):
    recs, pts, att, pix, offs = R.extract(lab, xyz, attrs, max_points)
    want = [(b, l) for b in range(len(recs)) for l in sorted(recs[b])]
    got = list(zip(objs.frame.cpu().tolist(), objs.label.cpu().tolist()))
    assert got == want
    K = len(want)
    f = {k: getattr(objs, k).cpu().numpy() for k in ("pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max",
                                                      "eigenvalues", "axes", "obb_center", "obb_half")}
    off = objs.offsets.cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([offs[k][1] for k in want])]).astype(np.int64))
    assert torch.equal(objs.points.cpu(), torch.from_numpy(pts))
    assert np.array_equal(objs.pixel_index.cpu().numpy(), pix)
    if attrs is not None:
        assert torch.equal(objs.attrs.cpu(), torch.from_numpy(att))
    axes_checked = 0
    for k, (b, l) in enumerate(want):
        r = recs[b][l]
        assert f["pixels"][k] == r["pixels"] and f["count"][k] == r["count"], (b, l)
        assert list(f["box"][k]) == list(r["box"]), (b, l)
        assert np.array_equal(f["aabb_min"][k], r["aabb_min"].astype(np.float32)), (b, l)
        assert np.array_equal(f["aabb_max"][k], r["aabb_max"].astype(np.float32)), (b, l)
        l0 = float(r["eig"][0])
        assert np.abs(f["centroid"][k] - r["centroid"]).max() <= 2e-6, (b, l)
        assert np.abs(f["cov"][k] - r["cov"]).max() <= 1e-6 + 1e-5 * l0, (b, l)
        assert np.abs(f["eigenvalues"][k] - r["eig"]).max() <= 1e-5 * l0 + 1e-9, (b, l)
        if r["count"] == 0:
            for name in ("centroid", "cov", "eigenvalues", "axes", "obb_center", "obb_half"):
                assert not np.any(f[name][k]), (b, l, name)
            continue
        # whatever the eigen-gaps: the properties and derived bounds of tests/stats_cases.py
        S.assert_metrics(S.object_metrics(dict(centroid=f["centroid"][k], cov=f["cov"][k], eig=f["eigenvalues"][k], axes=f["axes"][k],
                                               obb_half=f["obb_half"][k], obb_center=f["obb_center"][k]), r["points"], r), (b, l))
        if r["count"] == 1:
            assert not np.any(f["obb_half"][k]) and np.array_equal(f["obb_center"][k], f["centroid"][k])
        e = r["eig"]
        if l0 > 0 and e[0] - e[1] >= 1e-3 * l0 and e[1] - e[2] >= 1e-3 * l0:
            dots = np.sum(f["axes"][k].astype(np.float64) * r["axes"], axis=0)
            assert np.all(dots >= 1 - 1e-5), (b, l, dots)
            assert np.abs(f["obb_half"][k] - r["obb_half"]).max() <= 1e-5, (b, l)
            assert np.abs(f["obb_center"][k] - r["obb_center"]).max() <= 1e-5, (b, l)
            axes_checked += 1
    return K, axes_checked


def to_dev(device, *arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrs]


@pytest.mark.parametrize("H,W,ids", [(480, 640, "all"), (481, 643, "gaps"), (7, 13, "all"), (1, 1, "all")])
def test_synthetic_frames_match_reference(device, H, W, ids):
    lab, xyz, attrs = synthetic(2, H, W, seed=H * 7 + W, ids=ids)
    if H == 1:
        lab[:] = [[[5]], [[0]]]
        xyz[:, :, 0, 0] = [[0.1, 0.2, 0.9], [0.0, 0.0, 1.0]]
    dl, dx, da = to_dev(device, lab, xyz, attrs)
    objs = O.extract_objects(dl, dx, attrs=da, min_points=0)
    K, checked = check_against_reference(objs, lab, xyz, attrs)
    if H == 480:
        assert K == 2 * 127 and checked > 100
    # the float label maps test_sample returns, and int64 maps, give the same objects
    o2 = O.extract_objects(dl.float(), dx, min_points=0)
    o3 = O.extract_objects(dl.long(), dx, min_points=0)
    for k in ("pixels", "count", "centroid", "cov", "axes", "obb_center", "obb_half", "points", "pixel_index"):
        assert torch.equal(getattr(o2, k), getattr(objs, k)) and torch.equal(getattr(o3, k), getattr(objs, k)), k
    # min_points drops small objects and compacts the cloud accordingly
    o4 = O.extract_objects(dl, dx, min_points=50)
    cnt = objs.count.cpu()
    assert len(o4) == int((cnt >= 50).sum())
    for k in range(len(o4)):
        j = int(torch.nonzero((objs.frame == o4.frame[k]) & (objs.label == o4.label[k]))[0])
        assert torch.equal(o4.cloud(k), objs.cloud(j))


def test_deterministic_and_batch_independent(device):
    lab, xyz, attrs = synthetic(4, 480, 640, seed=11)
    dl, dx, da = to_dev(device, lab, xyz, attrs)
    a = O.object_records(dl, dx, da, 100)
    b = O.object_records(dl, dx, da, 100)
    n4 = int(a[4].cpu()[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
    for x, y in zip(a[1:4], b[1:4]):                    # rows past the total are not written
        assert torch.equal(x[:n4], y[:n4])
    rec4, pts4 = a[0].cpu().numpy(), a[1].cpu()
    off_field = O._F["offset"][0]
    for f in range(4):
        r1, p1, _, _, t1 = O.object_records(dl[f:f + 1].contiguous(), dx[f:f + 1].contiguous(), da[f:f + 1].contiguous(), 100)
        r1 = r1.cpu().numpy()
        mask = np.ones(r1.shape[-1], bool)
        mask[off_field] = False
        assert np.array_equal(r1[0][:, mask].view(np.uint32), rec4[f][:, mask].view(np.uint32))
        n = int(t1.cpu()[0])
        base = int(rec4[f, 0, off_field])              # id 0 keeps nothing: its offset is the frame's first row
        assert torch.equal(p1[:n].cpu(), pts4[base:base + n]), f


@pytest.mark.parametrize("M", [1, 100, 5000])
def test_subsampling_matches_reference(device, M):
    lab, xyz, attrs = synthetic(2, 480, 640, seed=M)
    lab[0, :200, :] = 9                                # one large object (> 5000 valid points)
    dl, dx, da = to_dev(device, lab, xyz, attrs)
    objs = O.extract_objects(dl, dx, attrs=da, max_points_per_object=M, min_points=0)
    check_against_reference(objs, lab, xyz, attrs, max_points=M)
    kept = (objs.offsets[1:] - objs.offsets[:-1]).cpu()
    assert int(kept.max()) == M and torch.all(kept <= M)


def test_capacity_is_respected(device):
    lab, xyz, _ = synthetic(1, 480, 640, seed=5)
    dl, dx = to_dev(device, lab, xyz)
    _, want, _, want_pix, _ = R.extract(lab, xyz)
    lib = _native.lib()
    cap, guard = 1000, 4096
    B, H, W = lab.shape
    pts = torch.full(((cap + guard) * 3,), -7.0, device=device)
    pix = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
    rec = torch.empty((B, 128, O._W), dtype=torch.int32, device=device)
    tot = torch.zeros(1, dtype=torch.int32, device=device)
    nws = lib.uoc_objects_workspace_bytes(B, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    _native.call("uoc_objects", device, dl, dx, None, 0, B, H, W, 0, rec, pts, None, pix, cap, tot, ws, nws)
    assert int(tot.cpu()[0]) == len(want) > cap
    p = pts.cpu().reshape(-1, 3)
    assert torch.equal(p[:cap], torch.from_numpy(want[:cap])) and bool((p[cap:] == -7.0).all())
    q = pix.cpu()
    assert np.array_equal(q[:cap].numpy(), want_pix[:cap]) and bool((q[cap:] == -7).all())


def _demo_sample(golden_dir):
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    return uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)


def test_reference_maps_on_real_depth(device, golden_dir):
    g = np.load(os.path.join(golden_dir, "demo.npz"))
    xyz = _demo_sample(golden_dir)["depth"].numpy()
    for key in ("out_label", "refined"):
        lab = np.asarray(g[key]).astype(np.int32).reshape(1, 480, 640)
        dl, dx = to_dev(device, lab, xyz)
        objs = O.extract_objects(dl, dx, min_points=0)
        K, _ = check_against_reference(objs, lab, xyz)
        assert K >= 1, key


def _nets():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def _same_objects(a, b):
    assert len(a) == len(b)
    for k in ("frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
              "obb_center", "obb_half", "offsets", "points", "pixel_index"):
        assert torch.equal(getattr(a, k).cpu(), getattr(b, k).cpu()), k


def test_segment_objects_end_to_end(device, golden_dir):
    cfg.device = device
    sample = _demo_sample(golden_dir)
    net, net_crop = _nets()
    np.random.seed(3)
    want_out, want_ref = TD.test_sample(sample, net, net_crop)
    np.random.seed(3)
    out, ref, objs = O.segment_objects(sample, net, net_crop)
    assert torch.equal(out, want_out) and ref is not None and torch.equal(ref, want_ref)
    _same_objects(objs, O.extract_objects(ref[:1].to(device), sample["depth"].to(device)))
    assert len(objs) >= 1 and set(objs.label.cpu().tolist()) <= set(np.unique(ref.numpy()).astype(int).tolist())
    np.random.seed(3)
    out2, _, objs1 = O.segment_objects(sample, net, net_crop, use_refined=False)
    assert torch.equal(out2, want_out)
    _same_objects(objs1, O.extract_objects(out2.to(device), sample["depth"].to(device)))


def test_export_objects_cli(device, golden_dir, tmp_path):
    cfg.device = device
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_objects.py"), "--imgdir",
                        os.path.join(golden_dir, "demo"), "--out", str(tmp_path), "--max-points", "500"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(os.listdir(tmp_path))
    assert files == ["000002_objects.npz"]
    z = np.load(tmp_path / files[0])
    sample = _demo_sample(golden_dir)
    net, net_crop = _nets()
    np.random.seed(cfg.RNG_SEED)
    _, ref, objs = O.segment_objects(sample, net, net_crop, max_points_per_object=500)
    assert np.array_equal(z["label_map"], ref[0].numpy().astype(np.int32))
    for k in ("frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
              "obb_center", "obb_half", "offsets", "points", "pixel_index"):
        assert np.array_equal(z[k], getattr(objs, k).cpu().numpy()), k
    assert int(np.diff(z["offsets"]).max()) <= 500
