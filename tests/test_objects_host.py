"""Per-object extraction without a GPU: the numpy restatement on hand-made cases, the C ABI's argument validation and the
ctypes mirror of uoc_object against the C layout."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import objects_reference as R
from unseenobjectclustering_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(H, W, fill=0):
    return np.full((1, H, W), fill, np.int32), np.zeros((1, 3, H, W), np.float32)


def test_reference_cuboid_axes_and_extents():
    # a 5 x 3 x 2 grid of points: known covariance, axes along x, y, z, half extents
    H, W = 6, 5
    lab, xyz = _frame(H, W)
    g = (np.array([(x, y, z) for x in range(5) for y in range(3) for z in range(2)]) * [0.04, 0.02, 0.01] + [1, 2, 3]).astype(np.float32)
    lab[0].reshape(-1)[:30] = 7
    xyz[0].reshape(3, -1)[:, :30] = g.T
    recs, pts, _, pix, offs = R.extract(lab, xyz)
    r = recs[0][7]
    assert r["pixels"] == 30 and r["count"] == 30 and list(r["box"]) == [0, 0, 4, 5]
    var = np.array([np.var(np.arange(5) * 0.04), np.var(np.arange(3) * 0.02), np.var(np.arange(2) * 0.01)])
    assert np.allclose(r["cov"], np.diag(var), atol=1e-12)
    assert np.allclose(r["eig"], var, atol=1e-12)
    assert np.allclose(r["axes"], np.eye(3), atol=1e-9)
    assert np.allclose(r["obb_half"], [0.08, 0.02, 0.005], atol=1e-6)
    assert np.allclose(r["obb_center"], g.astype(np.float64).min(0) + [0.08, 0.02, 0.005], atol=1e-6)
    assert np.allclose(r["aabb_min"], g.min(0)) and np.allclose(r["aabb_max"], g.max(0))
    assert offs[(0, 7)] == (0, 30) and np.array_equal(pix, np.arange(30)) and np.array_equal(pts, g)


def test_reference_single_and_two_points():
    lab, xyz = _frame(2, 3)
    lab[0, 0, 1] = 3
    xyz[0, :, 0, 1] = [0.5, -0.25, 1.0]
    lab[0, 1, 0] = lab[0, 1, 2] = 4
    xyz[0, :, 1, 0] = [0.0, 0.0, 1.0]
    xyz[0, :, 1, 2] = [0.2, 0.0, 1.0]
    recs, pts, _, pix, offs = R.extract(lab, xyz)
    one, two = recs[0][3], recs[0][4]
    assert one["count"] == 1 and np.allclose(one["centroid"], [0.5, -0.25, 1.0])
    assert np.allclose(one["cov"], 0) and np.allclose(one["obb_half"], 0) and np.allclose(one["obb_center"], one["centroid"])
    assert two["count"] == 2 and np.allclose(two["centroid"], [0.1, 0, 1])
    assert np.allclose(two["eig"], [0.01, 0, 0], atol=1e-12)
    assert np.allclose(two["axes"][:, 0], [1, 0, 0]) and np.allclose(two["obb_half"][0], 0.1)
    assert list(pix) == [1, 3, 5] and offs[(0, 3)] == (0, 1) and offs[(0, 4)] == (1, 2)


def test_reference_invalid_depth_and_background_ids():
    lab, xyz = _frame(3, 4)
    lab[0, 0, :] = 5
    xyz[0, 2, 0, :] = [0.0, -1.0, np.nan, np.inf]      # zero, negative, NaN, inf depth: no valid point
    xyz[0, 0, 0, 1] = np.nan
    lab[0, 1, 0], lab[0, 1, 1], lab[0, 1, 2] = 0, 128, -1
    lab[0, 2, :] = 1000
    xyz[0, 2, 1:, :] = 1.0
    recs, pts, _, _, _ = R.extract(lab, xyz)
    assert set(recs[0]) == {5}
    r = recs[0][5]
    assert r["pixels"] == 4 and r["count"] == 0 and len(pts) == 0 and list(r["box"]) == [0, 0, 3, 0]
    for k in ("centroid", "cov", "aabb_min", "aabb_max", "eig", "axes", "obb_center", "obb_half"):
        assert not np.any(r[k]), k


def test_reference_sign_rule_right_handed():
    rng = np.random.default_rng(0)
    for _ in range(50):
        A = rng.normal(size=(3, 3))
        w, ax = R.eig_frame(A @ A.T)
        assert np.all(np.diff(w) <= 0)
        assert np.allclose(ax.T @ ax, np.eye(3), atol=1e-9) and np.isclose(np.linalg.det(ax), 1.0)
        for k in (0, 1):
            e = ax[:, k]
            assert e[int(np.argmax(np.abs(e)))] > 0
    # tie on magnitude: the lowest index decides
    assert list(R.sign_rule(np.array([-0.5, 0.5, 0.0]) * np.sqrt(2))) == list(np.array([0.5, -0.5, 0.0]) * np.sqrt(2))


def test_reference_subsampling_rule():
    assert list(R.subsample_ranks(10, 4)) == [0, 2, 5, 7]
    assert list(R.subsample_ranks(3, 5)) == [0, 1, 2] and list(R.subsample_ranks(7, None)) == list(range(7))
    r = R.subsample_ranks(307200, 5000)
    assert len(r) == 5000 and len(np.unique(r)) == 5000 and r[-1] < 307200
    big = R.subsample_ranks(2**31 - 5, 3)               # needs 64-bit products
    assert list(big) == [0, (2**31 - 5) // 3, 2 * (2**31 - 5) // 3]


def test_objects_symbols_and_validation():
    lib = _native.lib()
    for s in ("uoc_objects", "uoc_objects_workspace_bytes"):
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s)
    ws = lib.uoc_objects_workspace_bytes(1, 480, 640)
    assert ws > 0
    assert lib.uoc_objects_workspace_bytes(2, 480, 640) > ws
    assert lib.uoc_objects_workspace_bytes(1, 960, 640) > ws and lib.uoc_objects_workspace_bytes(1, 480, 1280) > ws
    assert lib.uoc_objects_workspace_bytes(0, 480, 640) == 0
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: validation fails before any HIP call
    args = dict(lab=fake, xyz=fake, attr=None, C=0, B=1, H=4, W=4, M=0, obj=fake, pts=None, pat=None, pix=None, cap=0, tot=fake,
                ws=fake, nws=1 << 20)

    def call(**kw):
        a = dict(args, **kw)
        return lib.uoc_objects(a["lab"], a["xyz"], a["attr"], a["C"], a["B"], a["H"], a["W"], a["M"], a["obj"], a["pts"], a["pat"],
                               a["pix"], a["cap"], a["tot"], a["ws"], a["nws"], None)
    assert call(lab=None) == -22 and b"null" in lib.uoc_last_error().lower()
    assert call(xyz=None) == -22 and call(obj=None) == -22 and call(tot=None) == -22 and call(ws=None) == -22
    assert call(C=9, attr=fake) == -22 and b"attr_ch" in lib.uoc_last_error()
    assert call(B=0) == -22 and call(B=-1) == -22 and call(H=0) == -22
    assert call(C=2, attr=None) == -22
    assert call(nws=16) == -22 and b"workspace" in lib.uoc_last_error()


def test_ctypes_struct_matches_c_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to check the uoc_object layout")
    fields = [f for f, _ in _native.UocObject._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "uoc_hip.h"\nint main(){\n  printf("%zu\\n", sizeof(uoc_object));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(uoc_object, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_native.UocObject) == _native.OBJECT_BYTES
    assert out[1:] == [getattr(_native.UocObject, f).offset for f in fields]


def test_extract_objects_refuses_cpu_tensors():
    import torch
    from unseenobjectclustering_amd import objects
    with pytest.raises(_native.NativeError):
        objects.extract_objects(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(1, 3, 4, 4))
