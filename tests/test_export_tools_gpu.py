"""tools/export_objects.py as a composition: what a stage writes does not depend on which other stages run beside it.  The
stages on the table grid (--placement, --route, --memory, --motion, --grasp, --elevation, --putdown) share one support
plane and one grid per frame, the others (--relations, --confidence, --normals) read the label map alone or with that
plane; every tests/test_*_tools.py holds one stage against its reference, this holds them against each other."""
import numpy as np
import pytest

from tests.tool_cases import demo_frames, run_tool

pytestmark = pytest.mark.gpu

BASE = ("--max-points", "200", "--grid", "64", "--track", "--reid", "--components", "all", "--min-area", "20")
ROUTE_ID = "3"                  # any id in 1..127: the route_* arrays agree whether or not it owns a cell
GRID = ("--placement", "0.04", "--route", ROUTE_ID, "0.02", "--memory", "5", "--motion", "--grasp", "0.08", "--elevation", "0.005",
        "--putdown", "0.10", "0.05")
REST = ("--relations", "--confidence", "--normals")
STEMS = ("000002", "000003")


def export(frames, out, *flags):
    r = run_tool(frames, out, *BASE, *flags)
    assert r.returncode == 0, r.stdout + r.stderr
    return [np.load(out / f"{stem}_objects.npz") for stem in STEMS]


def same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_stage_outputs_do_not_depend_on_the_other_stages(device, golden_dir, tmp_path):
    frames = demo_frames(golden_dir, tmp_path / "frames")          # the demo frame twice
    every = export(frames, tmp_path / "all", "--plane", "--min-height", "0.02", *GRID, *REST)
    grid = export(frames, tmp_path / "grid", "--plane", *GRID)
    rest = export(frames, tmp_path / "rest", "--plane", "--min-height", "0.02", *REST)
    for a, g, r in zip(every, grid, rest):
        assert set(a.files) == set(g.files) | set(r.files)
        same(a, g, g.files)
        same(a, r, r.files)
    assert {"motion_best", "route_cost", "memory_state", "grasp_best", "top_cells", "putdown_best"} <= set(grid[1].files)
    assert {"standing", "front", "conf_map", "normal"} <= set(rest[1].files)


def test_the_plane_planes_chooses_feeds_the_shared_grid(device, golden_dir, tmp_path):
    """--placement writes the same beside --grasp, which reads the same grid, as without it."""
    frames = demo_frames(golden_dir, tmp_path / "frames")
    chosen = ("--planes", "3", "--planes-up", "0", "-1", "0", "--placement", "0.04")
    with_grasp, without = export(frames, tmp_path / "planes_grasp", *chosen, "--grasp", "0.08"), export(frames, tmp_path / "planes", *chosen)
    for a, b in zip(with_grasp, without):
        keys = [k for k in b.files if k.startswith(("place_", "plane_"))]
        assert len(keys) >= 4 + 8 and set(keys) == {k for k in a.files if k.startswith(("place_", "plane_"))}
        same(a, b, keys)
