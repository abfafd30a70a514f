"""CPU side of the support plane: the generated scenes and engineered cases contain what tests/test_support_gpu.py uses them
for, and, with the native call stubbed out, the wrapper's argument handling, standing_objects, drop_flat and the --plane
keys of tools/export_objects.py."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import support_reference as R
from unseenobjectclustering_amd import _native, support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def fitted(H, W, seed, tau_mm, num_hyp, noise):
    return R.fit(*R.tabletop(H, W, seed, noise=noise), num_hyp, tau_mm, seed)


@pytest.mark.parametrize("H,W,num_hyp", [(480, 640, 256), (61, 83, 64), (24, 32, 64)])
def test_tabletop_scenes_have_tied_winners_and_the_generating_plane(H, W, num_hyp):
    for seed in (1, 2):
        r = fitted(H, W, seed, 10, num_hyp, 0.0005)
        sc, p = r["scores"], r["plane"]
        assert (sc == sc.max()).sum() >= 2 and p["hyp"] == int(np.nonzero(sc == sc.max())[0][0])    # tied: the lowest h wins
        assert 0.7 * p["candidates"] <= p["inliers"] <= 0.9 * p["candidates"]                      # the wall stays outside
        assert np.degrees(np.arccos(min(1.0, float(p["normal"] @ R.PLANE_N)))) <= 1.0 and abs(p["d"] - R.PLANE_D) <= 0.005
        assert len(r["objects"]) >= 4
        for o in r["objects"].values():
            assert 0.03 <= o["height_max"] <= 0.16 and o["gap"] >= 1e-3 * o["lam0"]
        r3 = fitted(H, W, seed, 3, num_hyp, 0.0015)                                                 # 1.5 mm noise, 3 mm band
        assert len(set(r3["scores"].tolist())) > num_hyp // 2 and r3["plane"]["found"] == 1
        assert np.degrees(np.arccos(min(1.0, float(r3["plane"]["normal"] @ R.PLANE_N)))) <= 1.0


def test_tiny_frames_have_no_plane():
    for H, W in ((3, 1), (1, 1)):
        for seed in (1, 2):
            p = R.fit(*R.tabletop(H, W, seed), 64, 10, seed)["plane"]
            assert p["found"] == 0 and p["candidates"] < 3


def test_integer_steps_are_exact_on_known_values():
    assert R.mix(0) == 0 and R.mix(1) == 0x688990C0 and R.mix(0xDEADBEEF) == 0xE628C683 and R.mix(1 << 32 | 1) == R.mix(1)
    idx = R.sample_indices(5, 1000, 9)
    assert all(0 <= i < 1000 for i in idx) and idx == R.sample_indices(5, 1000, 9)
    q = np.array([[0, 0, 1000], [30000, 0, 1000], [0, 30000, 1000], [5, 5, 1007], [5, 5, 1008]], np.int64)
    for h in range(64):                     # whichever three of the first points a hypothesis draws: the plane z = 1000
        hyp = R.hypothesis(q[:3], h, 7, 1)
        if hyp is not None:
            n, p0, thr = hyp
            assert n[0] == n[1] == 0 and abs(n[2]) == 900000000 >> 0 and abs(n[2]) < 2 ** 30 and thr == 7 * abs(n[2])
            assert R.inlier_mask(q, hyp).tolist() == [True, True, True, True, False]       # 7 mm is in, 8 mm is out
    big = np.array([[-32767, -32767, 1], [32767, -32767, 2], [-32767, 32767, 32767]], np.int64)
    for h in range(64):
        hyp = R.hypothesis(big, h, 1000, 3)
        if hyp is not None:
            assert max(abs(v) for v in hyp[0]).bit_length() == 30 and R.inlier_mask(big, hyp).all()


def test_engineered_cases_have_the_stated_properties():
    E = {k: fn() for k, fn in R.ENGINEERED.items()}
    M = {k: len(R.candidates(*v)[1]) for k, v in E.items()}
    assert M["m0"] == 0 and M["m2"] == 2 and M["m3"] == 3 and M["all_objects"] == 0
    for k in ("m0", "m2", "collinear", "coincident", "all_objects"):
        r = R.fit(*E[k], 64, 10, 1, height_map=True)
        assert r["plane"]["found"] == 0 and (r["scores"] == -1).all() and not r["objects"] and np.isnan(r["height"]).all(), k
    assert M["collinear"] == 72 and M["coincident"] >= 3
    # m3: some hypotheses draw one candidate three times, some draw three different ones
    draws = [R.sample_indices(h, 3, 1) for h in range(64)]
    assert any(len(set(d)) == 1 for d in draws) and any(len(set(d)) == 3 for d in draws)
    r = R.fit(*E["m3"], 64, 10, 1)
    assert r["plane"]["found"] == 1 and r["plane"]["inliers"] == 3 and r["objects"][5]["count"] == 1
    # range: +-32.767 m are candidates, what lies beyond is not
    lab, xyz = E["range"]
    idx, q = R.candidates(lab, xyz)
    assert int((np.abs(q) == R.Q_MAX).any(axis=1).sum()) == 5 and np.abs(q).max() == R.Q_MAX
    flat = xyz.reshape(3, -1)
    out = np.setdiff1d(np.nonzero((lab.reshape(-1) == 0))[0], idx)
    assert len(out) in (7, 8) and (np.abs(flat[:, out]).max(axis=0) > 32.767).all()      # 32.7675 m: as fp32 rounds it
    assert {(5 + k) % 12 * 16 + 3 * (5 + k) % 16 for k in range(5)} | {11 * 16 + 1, 4} <= set(out.tolist())
    assert R.fit(lab, xyz, 64, 10, 1)["plane"]["found"] == 1
    # nasty: every kind of bad depth among candidates and objects, ids outside 1..127 as background, the two special objects
    lab, xyz = E["nasty"]
    bg = ~((lab >= 1) & (lab < 128))
    z = xyz[2]
    for sel in (bg, ~bg):
        assert np.isnan(z[sel]).any() and np.isinf(z[sel]).any() and (z[sel] == 0).any() and (z[sel] < 0).any()
    assert set(np.unique(lab[bg]).tolist()) == {0, 128, -1, 1000} and np.isnan(xyz[0]).any()
    idx, _ = R.candidates(lab, xyz)
    assert set(np.unique(lab.reshape(-1)[idx]).tolist()) == {0, 128, -1, 1000}
    r = R.fit(lab, xyz, 64, 10, 1)
    assert r["plane"]["found"] == 1 and r["objects"][50]["count"] == 1 and 51 not in r["objects"] and (lab == 51).sum() == 3
    assert r["objects"][50]["gap"] == 0 and not r["objects"][50]["half"].any()
    # origin_plane: d is exactly 0, the sign rule picks +x, u falls back to the y axis
    p = R.fit(*E["origin_plane"], 64, 10, 1)["plane"]
    assert p["found"] == 1 and p["d"] == 0.0 and p["normal"].tolist() == [1.0, 0.0, 0.0]
    assert p["u"].tolist() == [0.0, 1.0, 0.0] and p["v"].tolist() == [0.0, 0.0, 1.0]


def fake_result(B=2):
    z = lambda *s: torch.zeros(*s)                                                  # noqa: E731
    f = dict(found=torch.ones(B, dtype=torch.int32), candidates=torch.full((B,), 10, dtype=torch.int32),
             inliers=torch.full((B,), 9, dtype=torch.int32), hyp=torch.zeros(B, dtype=torch.int32), normal=z(B, 3), d=z(B),
             centroid=z(B, 3), eig=z(B, 3), rms=z(B), u=z(B, 3), v=z(B, 3), count=torch.zeros(B, 128, dtype=torch.int32),
             height_min=z(B, 128), height_max=z(B, 128), foot=z(B, 128, 2), cov2=z(B, 128, 3), axis=z(B, 128, 2),
             half=z(B, 128, 3), center=z(B, 128, 3), height=None)
    f["count"][:, [1, 2, 3]] = 5
    f["height_max"][0, [1, 2, 3]] = torch.tensor([0.10, 0.004, 0.02])
    if B > 1:
        f["height_max"][1, [1, 2, 3]] = torch.tensor([0.004, 0.10, 0.019])
    f["height_max"][:, 9] = 0.5                                                     # no valid point: never standing
    return support.PlaneResult(**f)


def test_standing_objects_and_drop_flat_on_a_fabricated_result():
    res = fake_result()
    s = support.standing_objects(res, 0.02)
    assert s.dtype == torch.bool and s.shape == (2, 128)
    assert torch.nonzero(s[0]).reshape(-1).tolist() == [1, 3] and torch.nonzero(s[1]).reshape(-1).tolist() == [2]
    lab = torch.tensor([[[1, 2, 3, 9], [0, 128, -1, 1000]], [[1, 2, 3, 9], [0, 128, -1, 1000]]], dtype=torch.int32)
    out = support.drop_flat(lab, res, 0.02)
    assert out.dtype == lab.dtype and out.tolist() == [[[1, 0, 3, 0], [0, 128, -1, 1000]], [[0, 2, 0, 0], [0, 128, -1, 1000]]]
    assert support.drop_flat(lab.float(), res, 0.02).tolist() == out.float().tolist()
    one = support.PlaneResult(**{k: (v[:1] if isinstance(v, torch.Tensor) else v) for k, v in res.__dict__.items()})
    assert support.drop_flat(lab[0], one, 0.02).tolist() == out[0].tolist()            # [H,W] is B = 1
    with pytest.raises(_native.NativeError):
        support.drop_flat(lab, one, 0.02)


def test_fit_plane_argument_handling_with_the_native_call_stubbed(monkeypatch):
    lab, xyz = torch.zeros(4, 5, dtype=torch.int64), torch.zeros(3, 4, 5, dtype=torch.float64)
    with pytest.raises(_native.NativeError):
        support.fit_plane(lab, xyz)                                                 # host tensors: no CPU fallback
    for bad in (dict(num_hyp=0), dict(num_hyp=1025), dict(tau=0.0), dict(tau=0.0004), dict(tau=1.0006)):
        with pytest.raises(ValueError):
            support.fit_plane(lab, xyz, **bad)
    calls = []

    def stub(labels, xyz_, num_hyp, tau_mm, seed, height_map=False):
        calls.append((labels, xyz_, num_hyp, tau_mm, seed, height_map))
        B, H, W = labels.shape
        return (torch.zeros(B, support._PW, dtype=torch.int32), torch.zeros(B, 128, support._OW, dtype=torch.int32),
                torch.zeros(B, H, W) if height_map else None)

    monkeypatch.setattr(_native, "on_gpu", lambda t: isinstance(t, torch.Tensor))
    monkeypatch.setattr(support, "plane_records", stub)
    res = support.fit_plane(lab, xyz, num_hyp=7, tau=0.0126, seed=-1, height_map=True)
    labels, xyz_, num_hyp, tau_mm, seed, height_map = calls[-1]
    assert labels.shape == (1, 4, 5) and labels.dtype == torch.int32 and xyz_.shape == (1, 3, 4, 5) and xyz_.dtype == torch.float32
    assert (num_hyp, tau_mm, height_map) == (7, 13, True) and res.seed == 0xFFFFFFFF and res.tau_mm == 13
    assert res.found.shape == (1,) and res.normal.shape == (1, 3) and res.d.shape == (1,) and res.count.shape == (1, 128)
    assert res.center.shape == (1, 128, 3) and res.foot.shape == (1, 128, 2) and res.height.shape == (1, 4, 5)
    assert res.found.dtype == res.count.dtype == torch.int32 and res.d.dtype == res.half.dtype == torch.float32
    assert support.fit_plane(lab, xyz).tau_mm == 10 and calls[-1][2] == 256 and calls[-1][4] == 1          # the defaults
    for l, x in ((lab, xyz[:2]), (lab, torch.zeros(3, 4, 6)), (torch.zeros(2, 4, 5), xyz), (lab[0], xyz)):
        with pytest.raises(_native.NativeError):
            support.fit_plane(l, x)


def test_record_layouts_match_the_header():
    import ctypes
    assert ctypes.sizeof(_native.UocPlane) == 4 * support._PW == 84 and ctypes.sizeof(_native.UocPlaneObject) == 4 * support._OW == 64
    header = open(os.path.join(ROOT, "include", "uoc_hip.h")).read()
    for struct, name in ((_native.UocPlane, "uoc_plane"), (_native.UocPlaneObject, "uoc_plane_object")):
        body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
        members = re.findall(r"^\s*(?:int32_t|float)\s+(\w+)", body, re.M)
        assert members == [f for f, _ in struct._fields_], name                     # same fields in the same order


def test_missing_symbol_is_a_native_error(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(_native.NativeError("libuoc_hip.so not found")))
    with pytest.raises(_native.NativeError):
        support.plane_records(torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(1, 3, 2, 2), 8, 10, 1)


def test_export_plane_keys_without_a_gpu():
    spec = importlib.util.spec_from_file_location("uoc_export_objects", os.path.join(ROOT, "tools", "export_objects.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = fake_result(1)
    ids = torch.tensor([1, 3])
    rec = mod.plane_arrays(res, ids)
    assert set(rec) == {"plane_" + k for k in support.PLANE_FIELDS} | \
        {"height_min", "height_max", "foot", "cov2", "upright_axis", "upright_half", "upright_center"}
    assert not set(rec) & set(mod.FIELDS) and "label_map" not in rec               # nothing the plain export writes is replaced
    assert rec["plane_normal"].shape == (3,) and rec["plane_found"] == 1 and rec["upright_center"].shape == (2, 3)
    assert np.allclose(rec["height_max"], [0.10, 0.02])
    rec = mod.plane_arrays(res, ids, 0.05)
    assert rec["standing"].tolist() == [True, False]
