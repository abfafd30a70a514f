"""Where users meet the placement stage: the opt-in --placement RADIUS_M / --grid / --cell-mm of tools/export_objects.py,
alone and on tracked and component-split maps (GPU: the step has no CPU path)."""
import numpy as np
import pytest

from tests import placement_reference as R
from tests.tool_cases import BASE_KEYS, COMPONENT_KEYS, PLACEMENT_KEYS, PLANE_KEYS, demo_xyz, export


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
