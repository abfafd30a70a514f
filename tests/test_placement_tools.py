"""Where users meet the placement stage: the opt-in --placement RADIUS_M / --grid / --cell-mm of tools/export_objects.py,
alone and on tracked and component-split maps (GPU: the step has no CPU path)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import placement_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_KEYS = {"frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
             "obb_center", "obb_half", "offsets", "points", "pixel_index", "label_map"}
PLACEMENT_KEYS = {"place_state", "place_dist2", "place_widest_cell", "place_widest_xyz"}
PLANE_KEYS = {"plane_" + k for k in ("found", "candidates", "inliers", "hyp", "normal", "d", "centroid", "eig", "rms", "u", "v")} \
    | {"height_min", "height_max", "foot", "cov2", "upright_axis", "upright_half", "upright_center"}
COMPONENT_KEYS = {"component_src", "component_area", "component_siblings"}


def export(golden_dir, out, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_objects.py"), "--imgdir",
                        os.path.join(golden_dir, "demo"), "--out", str(out), "--max-points", "500", *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out / "000002_objects.npz")


def demo_xyz(golden_dir):
    from unseenobjectclustering_amd import io as uio
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    return uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)["depth"][0].numpy()


def check_against_reference(z, xyz, radius_mm, G, cell_mm):
    """The plane comes from the export itself (--plane), everything after it from the reference."""
    plane = dict(found=int(z["plane_found"]), normal=z["plane_normal"], d=z["plane_d"], centroid=z["plane_centroid"], u=z["plane_u"],
                 v=z["plane_v"])
    k = -(-radius_mm // cell_mm) + 1
    want = R.free_space(z["label_map"], xyz, plane, G, cell_mm, 10, 10, 1, 1, [(k * k, 0, 0, R.WIDEST)])
    assert z["place_state"].shape == (G, G) and np.array_equal(z["place_state"], want["state"])
    assert np.array_equal(z["place_dist2"], want["dist2"]) and np.array_equal(z["place_widest_cell"], want["answers"][0])
    i, j = (int(v) for v in want["answers"][0][:2])
    assert plane["found"] == 1 and i >= 0 and want["state"][i, j] == 1
    c, u, v = (np.asarray(plane[key], np.float64) for key in ("centroid", "u", "v"))
    spot = c + (i - G // 2 + 0.5) * cell_mm / 1000.0 * u + (j - G // 2 + 0.5) * cell_mm / 1000.0 * v
    assert z["place_widest_xyz"].shape == (3,) and np.allclose(z["place_widest_xyz"], spot, rtol=0, atol=1e-9)
    return want


@pytest.mark.gpu
def test_export_objects_placement_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path / "place", "--plane", "--placement", "0.04", "--grid", "128", "--cell-mm", "20")
    assert set(z.files) == BASE_KEYS | PLANE_KEYS | PLACEMENT_KEYS
    check_against_reference(z, demo_xyz(golden_dir), 40, 128, 20)
    alone = export(golden_dir, tmp_path / "alone", "--placement", "0.04", "--grid", "128", "--cell-mm", "20")       # the plane is implied
    assert set(alone.files) == BASE_KEYS | PLACEMENT_KEYS
    for k in BASE_KEYS | PLACEMENT_KEYS:
        assert np.array_equal(alone[k], z[k]), k


@pytest.mark.gpu
def test_export_objects_placement_on_split_and_tracked_maps_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path, "--placement", "0.05", "--plane", "--components", "all", "--min-area", "20", "--track")
    assert set(z.files) == BASE_KEYS | PLANE_KEYS | PLACEMENT_KEYS | COMPONENT_KEYS | {"raw_label_map", "track_uid"}
    want = check_against_reference(z, demo_xyz(golden_dir), 50, 256, 10)
    assert (want["state"] == 2).any() and (want["state"] == 1).any()
