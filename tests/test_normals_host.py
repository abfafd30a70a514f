"""The surface-normal stage without a GPU: the numpy reference against its pixel-by-pixel restatement, hand counts, the
bounds the header states, the scenes the GPU tests rely on, the wrapper's argument checks and the C entry's rejections
(every one happens before any device work, so they run without a device)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import normals_reference as R
from tests import support_reference as S13
from unseenobjectclustering_amd import _native, normals


@functools.lru_cache(maxsize=None)
def boxes(H, W, seed):
    return R.boxes_scene(H, W, seed)


@functools.lru_cache(maxsize=None)
def boxes_parts(H, W, seed):
    lab, xyz = boxes(H, W, seed)
    return R.estimate(xyz, lab, R.table_plane(), parts=True)


def same(a, b, what):
    for k in ("n", "info", "faces"):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("r,s,mp,A,angles", [(1, 0, 1, 16, (20, 20)), (2, 2, None, 5, (0, 0)), (3, 1, 9, 1, (45, 44)),
                                             (2, 1, 2, 32, (89, 0))])
def test_the_vectorised_reference_is_the_pixelwise_one(r, s, mp, A, angles):
    lab, xyz = boxes(24, 32, 1)
    kw = dict(step=r, window=s, min_pairs=mp, dirs=R.direction_table(A), jump_mm=30)
    kw["c_up"], kw["s_side"] = R.thresholds(*angles)
    same(R.estimate(xyz, lab, R.table_plane(), **kw), R.estimate_pixelwise(xyz, lab, R.table_plane(), **kw), (r, s))
    same(R.estimate(xyz, None, None, **kw), R.estimate_pixelwise(xyz, None, None, **kw), "bare")


def test_the_two_references_agree_on_the_engineered_frames():
    lab, xyz = R.case_nasty(20, 28)
    same(R.estimate(xyz, lab, R.table_plane()), R.estimate_pixelwise(xyz, lab, R.table_plane()), "nasty")
    xyz = R.case_range()
    same(R.estimate(xyz, step=1, window=1, jump_mm=1000), R.estimate_pixelwise(xyz, step=1, window=1, jump_mm=1000), "range")
    tie, plane = R.case_tie()
    kw = dict(dirs=R.direction_table(4), step=1, window=1)
    same(R.estimate(tie, None, plane, **kw), R.estimate_pixelwise(tie, None, plane, **kw), "tie")


def test_hand_count_on_the_grid_plane():
    xyz = S13._grid_plane(12, 16)              # q = 16 (4x - 32, 3y, 600 + x + 2y): TX ~ (4, 0, 1), TY ~ (0, 3, 2), TY x TX = (3, 8, -12)
    for r, s, mp in ((1, 0, 1), (2, 1, None)):
        o = R.estimate(xyz, step=r, window=s, min_pairs=mp, parts=True)
        assert int(o["has"].sum()) == 140
        n = o["n"][o["has"]]
        assert (n[:, 0] > 0).all() and np.array_equal(n[:, 1] * 3, n[:, 0] * 8) and np.array_equal(n[:, 2] * 3, n[:, 0] * -12)
        assert not o["grazing"].any() and (o["cls"] == 0).all() and (o["faces"][0, :2] == [192, 140]).all()
    o = R.estimate(xyz, step=1, window=0, min_pairs=1, parts=True)
    assert np.array_equal(np.unique(o["n"][o["has"]], axis=0), [[3072, 8192, -12288]])       # (2*16)^2 (3, 8, -12)
    assert o["has"][1:-1, 1:-1].all() and o["has"].sum() == 10 * 14


def test_a_frontal_plane_is_up_by_exact_equality():
    xyz = R.frontal(12, 16)
    plane = R.plane_dict(*R.frontal_plane_tuple())
    c_up, s_side = R.thresholds(0.0, 0.0)
    assert (c_up, s_side) == (1 << 28, 0)
    o = R.estimate(xyz, None, plane, step=1, window=1, c_up=c_up, s_side=s_side, parts=True)
    n = o["n"][o["has"]]
    assert o["has"].sum() > 0 and (n[:, :2] == 0).all() and (n[:, 2] < 0).all()
    Pq = R.frame_axes(plane)[0]
    assert Pq.tolist() == [0, 0, -16384]
    c, L = n @ Pq, -n[:, 2]
    assert np.array_equal(c * 16384, c_up * L)                      # equality, not merely >=
    assert (o["cls"][o["has"]] == R.UP).all() and (o["faces"][0, 2] == o["has"].sum())
    # one unit of 2^-14 short of the plane normal and the same frame is no longer UP
    tilted = dict(plane, normal=np.array([0.0, 0.0, -16383.0 / 16384.0], np.float32))
    assert not (R.estimate(xyz, None, tilted, step=1, window=1, c_up=c_up, s_side=s_side, parts=True)["cls"] == R.UP).any()


def test_an_in_plane_normal_at_45_degrees_takes_the_lower_bin():
    xyz, plane = R.case_tie()
    o = R.estimate(xyz, None, plane, step=1, window=1, dirs=R.direction_table(4), parts=True)
    n = o["n"][o["has"]]
    assert o["has"].sum() > 0 and (n[:, 0] > 0).all() and (n[:, 1] == 0).all() and np.array_equal(n[:, 0], -n[:, 2])
    assert (o["cls"][o["has"]] == R.SIDE).all() and (o["bin"] == 0).all()
    assert o["faces"][0, 3] == o["has"].sum() == o["faces"][0, 8] and o["faces"][0, 7] == 0
    # the same normal one bin further round is unambiguous
    o8 = R.estimate(xyz, None, plane, step=1, window=1, dirs=R.direction_table(8), parts=True)
    assert (o8["bin"][o8["has"]] == 1).all()


def test_the_stated_bounds_hold_on_the_scenes():
    for r, s, jump in ((2, 2, 30), (8, 4, 1000)):
        lab, xyz = boxes(96, 128, 2)
        o = R.estimate(xyz, lab, R.table_plane(), step=r, window=s, jump_mm=jump, parts=True)
        assert np.abs(o["q"]).max() <= R.Q_MAX
        assert np.abs(o["TX"]).max() <= 81 * 16383 and np.abs(o["TY"]).max() <= 81 * 16383
        assert np.abs(o["N"]).max() < 1 << 43 and np.abs(o["n"]).max() <= 1 << 30
        assert o["nX"].max() <= (2 * s + 1) ** 2 and o["nY"].max() <= (2 * s + 1) ** 2
        assert (o["info"] >= 0).all() and o["info"].max() < 1 << 31
        assert ((o["info"] != 0) == o["has"]).all()
        f = o["faces"]
        assert f[:, 0].sum() == 96 * 128 and (f[:, 1] == f[:, 2:6].sum(axis=1)).all() and (f[:, 3] == f[:, 8:].sum(axis=1)).all()


def test_the_shift_occurs_at_the_largest_stencil():
    o = R.estimate(S13._grid_plane(40, 48), step=8, window=4, jump_mm=1000, parts=True)
    assert o["has"].any() and o["k"][o["has"]].max() > 0
    # 81 pairs of 16 columns by 81 pairs of 16 rows: |N_z| = 81^2 * 768 * 1024, 33 bits, so k = 3
    assert int(np.abs(o["N"]).max()) == 81 * 81 * 768 * 1024 and int(np.abs(o["N"]).max()).bit_length() == 33
    assert o["k"][o["nX"] + o["nY"] == 162].tolist().count(3) == int((o["nX"] + o["nY"] == 162).sum())
    full = o["nX"] == 81
    n = o["n"][full & o["has"]]
    assert full.any() and np.abs(n).max() < 1 << 30 and np.abs(n).max() >= 1 << 29          # shifted into 30 bits


def test_the_table_normals_lie_near_the_generating_plane():
    lab, xyz = S13.tabletop(480, 640, 1)
    o = R.estimate(xyz, lab, None, step=2, window=2, jump_mm=20, min_pairs=12, parts=True)
    table = o["has"] & (lab == 0) & (xyz[2] < S13.Z_CUT)
    ang = R.angle_deg(o["n"][table], S13.PLANE_N)
    print("table pixels", int(table.sum()), "median", np.median(ang), "p99", np.percentile(ang, 99), "max", ang.max())
    assert table.sum() > 100000 and np.median(ang) < 1.5 and ang.max() < 15.0


def test_boxes_scene_holds_what_the_gpu_tests_use_it_for():
    lab, xyz = boxes(480, 640, 1)
    o = boxes_parts(480, 640, 1)
    z_mm = xyz[2].astype(np.float64) * 1000.0
    assert np.abs(z_mm - np.rint(z_mm)).max() < 1e-3                            # whole millimetres
    assert set(np.unique(lab)) == set(range(6)) and (xyz[2] == 0).mean() > 0.03
    counts = np.bincount(o["cls"].ravel(), minlength=5)
    assert (counts[1:] > 50).all(), counts                                     # UP, SIDE, OBLIQUE and DOWN
    mh, mw = R.MIRROR
    patch = np.zeros_like(o["has"])
    patch[-mh:, :mw] = True
    inner = np.zeros_like(patch)
    inner[-mh + 4:, :mw - 4] = True                                             # the pixels whose whole stencil lies in the patch
    assert o["grazing"][inner & o["has"]].all() and (o["cls"][inner & o["has"]] == R.DOWN).all() and (inner & o["has"]).sum() > 20
    assert o["grazing"][~patch].mean() < 1e-3
    f = o["faces"]
    assert (f[1:6, 3] > 1000).all()                                             # every cuboid shows side faces
    two = [a for a in range(1, 6) if any(f[a, 8 + k] >= 0.2 * f[a, 3] and f[a, 8 + (k + 4) % 16] >= 0.2 * f[a, 3] for k in range(16))]
    assert two, f[1:6, 8:24]                                                    # two azimuth peaks a quarter turn apart
    up = (o["cls"] == R.UP) & (lab == 0)
    assert np.median(R.angle_deg(o["n"][up], S13.PLANE_N)) < 1.5


def test_engineered_frames_contain_their_cases():
    lab, xyz = R.case_nasty()
    assert {0, 128, -1, 1000, 127, 50} <= set(np.unique(lab)) and (lab == 50).sum() == 1
    assert np.isnan(xyz).any() and np.isinf(xyz).any() and (xyz[2] < 0).any() and (xyz[2] == 0).any()
    o = R.estimate(xyz, lab, R.table_plane(), parts=True)
    assert o["faces"][50, 0] == 1 and o["faces"][50, 1] == 0 and o["faces"][127, 1] > 0
    assert o["faces"][0, 0] == ((lab < 1) | (lab > 127)).sum()
    lab, xyz = R.case_all_ids()
    assert set(np.unique(lab)) == set(range(1, 128))
    xyz = R.case_range()
    valid, q = R.points(xyz)
    assert q.max() == R.Q_MAX and np.abs(q).max() == R.Q_MAX and (~valid).sum() == 6
    assert valid[0, 0] and q[0, 0, 0] == 524272 and valid[4 % 12, 12 % 16] and not valid[5, 15]
    ex, d, _ = R.pairs(valid, q, R.ids(None, valid.shape), 1, 1000, 1)
    assert ex[9, 5] and d[0, 9, 5] == 16383 and not ex[9, 9] and (q[0, 9, 10] - q[0, 9, 8]) == 16384
    o = R.estimate(R.case_collinear(), step=1, window=1, jump_mm=1000, parts=True)
    assert (o["nX"] > 0).any() and (o["nY"] > 0).any() and (o["N"] == 0).all() and not o["has"].any() and (o["info"] == 0).all()
    o = R.estimate(R.case_mirrored(), step=1, window=0, min_pairs=1, parts=True)
    assert o["has"].sum() == 140 and o["grazing"][o["has"]].all() and (o["n"][o["has"]][:, 2] > 0).all()


def test_unit_normals_of_the_reference_are_unit():
    o = boxes_parts(480, 640, 1)
    u = o["unit"][:, o["has"]]
    assert np.abs((u * u).sum(axis=0) - 1).max() < 1e-12 and np.isnan(o["unit"][:, ~o["has"]]).all()


# ---- the wrapper and the C entry -----------------------------------------------------------------------------------------
def test_symbols_tables_and_thresholds():
    assert "uoc_normals" in _native.EXPORTED_SYMBOLS and "uoc_normals_workspace_bytes" in _native.EXPORTED_SYMBOLS
    lib = _native.lib()
    assert hasattr(lib, "uoc_normals") and lib.uoc_normals_workspace_bytes(3, 480, 640) >= 3 * 128 * 40 * 4
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, -1), (1, 65536, 32768)):
        assert lib.uoc_normals_workspace_bytes(*bad) == 0
    for A in (1, 4, 5, 16, 32):
        assert np.array_equal(normals.direction_table(A), R.direction_table(A))
    assert normals.direction_table(4).tolist() == [[16384, 0], [0, 16384], [-16384, 0], [0, -16384]]
    for up, side in ((20, 20), (0, 0), (45, 44), (89, 0)):
        assert normals.thresholds(up, side) == R.thresholds(up, side)
        assert normals.thresholds(up, side)[0] > normals.thresholds(up, side)[1]
    for bad in ((-1, 0), (0, -1), (45, 45), (90, 0), (float("nan"), 0)):
        with pytest.raises(ValueError):
            normals.thresholds(*bad)
    for A in (0, 33):
        with pytest.raises(ValueError):
            normals.direction_table(A)
    assert (normals.UP, normals.SIDE, normals.OBLIQUE, normals.DOWN) == (R.UP, R.SIDE, R.OBLIQUE, R.DOWN)
    assert normals.FACE_FIELDS == R.FACE_FIELDS and normals.FACE_WORDS == R.FACE_WORDS


def test_estimate_rejects_bad_arguments_before_touching_a_device():
    x = torch.zeros((3, 4, 4))
    for kw in (dict(step=0), dict(step=9), dict(window=-1), dict(window=5), dict(jump=0.0), dict(jump=1.5), dict(min_pairs=0),
               dict(window=1, min_pairs=10), dict(angles=0), dict(angles=33), dict(up_deg=50, side_deg=40), dict(up_deg=-1)):
        with pytest.raises(ValueError):
            normals.estimate(x, **kw)
    with pytest.raises(_native.NativeError):
        normals.estimate(x)                         # a CPU tensor: there is no CPU path


def raw_call(**over):
    """uoc_normals with pointers that are never dereferenced by a rejected call."""
    lib = _native.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dirs = (ctypes.c_int32 * 64)(*([16384, 0] * 32))
    a = dict(xyz=p, labels=p, planes=p, B=1, H=8, W=8, step=2, window=2, jump_mm=30, min_pairs=1, dirs=ctypes.cast(dirs, ctypes.c_void_p),
             A=16, c_up=1 << 27, s_side=1 << 26, n=p, unit=p, faces=p, ws=p, ws_bytes=1 << 20)
    a.update(over)
    rc = lib.uoc_normals(a["xyz"], a["labels"], a["planes"], a["B"], a["H"], a["W"], a["step"], a["window"], a["jump_mm"], a["min_pairs"],
                         a["dirs"], a["A"], a["c_up"], a["s_side"], a["n"], a["unit"], a["faces"], a["ws"], a["ws_bytes"], None)
    return rc, lib.uoc_last_error().decode()


def test_the_c_entry_names_what_it_rejects():
    EINVAL = -22
    bad_dirs = (ctypes.c_int32 * 4)(16384, 0, 16385, 0)
    lo_dirs = (ctypes.c_int32 * 4)(16384, 0, 0, -16385)
    cases = [(dict(xyz=None), "null"), (dict(n=None), "null"), (dict(faces=None), "null"), (dict(dirs=None), "null"), (dict(ws=None), "null"),
             (dict(B=0), "shape"), (dict(B=65536), "shape"), (dict(H=0), "shape"), (dict(H=65536, W=32768), "shape"),
             (dict(step=0), "step"), (dict(step=9), "step"), (dict(window=-1), "window"), (dict(window=5), "window"),
             (dict(jump_mm=0), "jump_mm"), (dict(jump_mm=1001), "jump_mm"), (dict(min_pairs=0), "min_pairs"), (dict(min_pairs=26), "min_pairs"),
             (dict(A=0), "directions"), (dict(A=33), "directions"), (dict(c_up=-1), "c_up"), (dict(c_up=(1 << 28) + 1), "c_up"),
             (dict(s_side=-1), "s_side"), (dict(c_up=5, s_side=5), "not above"),
             (dict(A=2, dirs=ctypes.cast(bad_dirs, ctypes.c_void_p)), "direction 1"), (dict(A=2, dirs=ctypes.cast(lo_dirs, ctypes.c_void_p)), "direction 1"),
             (dict(ws_bytes=128 * 40 * 4 - 1), "workspace")]
    for over, word in cases:
        rc, msg = raw_call(**over)
        assert rc == EINVAL and word in msg, (over, rc, msg)
    keep = (ctypes.c_int32 * 64)()
    odd = ctypes.c_void_p((ctypes.addressof(keep) + 15) // 16 * 16 + 4)
    for name, word in (("ws", "workspace not 16-byte aligned"), ("n", "n not 16-byte aligned")):
        rc, msg = raw_call(**{name: odd})
        assert rc == EINVAL and word in msg, (name, rc, msg)
