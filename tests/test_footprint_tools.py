"""Where users meet the footprint stage: the opt-in --putdown LENGTH_M WIDTH_M / --putdown-angles of
tools/export_objects.py.  The argument wiring and the arrays the tool adds are checked on the CPU (the tool's own
putdown_arrays on a synthetic result); the command line on the GPU (the step has no CPU path):
tests/test_footprint_gpu.py holds the stage against the reference end to end, segment_objects(..., footprint=True)
included."""
import types

import numpy as np
import pytest
import torch

from tests import footprint_reference as R
from tests.tool_cases import BASE_KEYS, PLACEMENT_KEYS, demo_sample, export, tool  # noqa: F401  (tool is a fixture)

PUTDOWN_KEYS = {"putdown_fits", "putdown_count", "putdown_best", "putdown_dirs", "putdown_center", "putdown_axis"}


def test_putdown_arguments_and_arrays(tool):
    from unseenobjectclustering_amd import placement
    base = ["--imgdir", "frames", "--out", "objs"]
    a = tool.build_parser().parse_args(base)
    assert a.putdown is None and a.putdown_angles == 16
    a = tool.build_parser().parse_args(base + ["--putdown", "0.3", "0.06"])
    assert a.putdown == [0.3, 0.06] and a.placement is None and a.grasp is None and a.elevation is None and not a.plane
    a = tool.build_parser().parse_args(base + ["--putdown", "0.1", "0.05", "--putdown-angles", "8", "--grid", "128", "--placement", "0.04",
                                               "--elevation", "0.005", "--grasp", "0.08"])
    assert (a.putdown, a.putdown_angles, a.grid, a.placement, a.elevation, a.grasp) == ([0.1, 0.05], 8, 128, 0.04, 0.005, 0.08)
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(base + ["--putdown", "0.3"])
    assert set(tool.PUTDOWN_KEYS) == PUTDOWN_KEYS
    planes = torch.from_numpy(placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0]))
    fits = torch.zeros((1, 1, 16, 16), dtype=torch.int32)
    fits[0, 0, 10, 3] = 0x10
    count = torch.zeros((1, 1, 32), dtype=torch.int32)
    count[0, 0, 4] = 1
    best = torch.tensor([[[1, 10, 3, 4, 25, 109, 1, 1]]], dtype=torch.int32)
    syn = types.SimpleNamespace(fits=fits, count=count, best=best, dirs=R.direction_table(16), angles=16, planes=planes, grid=16, cell_mm=10)
    rec = tool.putdown_arrays(syn)
    assert set(rec) == PUTDOWN_KEYS
    assert rec["putdown_fits"].shape == (16, 16) and rec["putdown_fits"].dtype == np.int32 and rec["putdown_fits"][10, 3] == 16
    assert rec["putdown_count"].shape == (32,) and rec["putdown_best"].tolist() == [1, 10, 3, 4, 25, 109, 1, 1]
    assert rec["putdown_dirs"].shape == (16, 2) and rec["putdown_dirs"].dtype == np.int32
    assert np.allclose(rec["putdown_center"], [0.025, 0.045, 1.0], rtol=0, atol=1e-12)
    assert np.allclose(rec["putdown_axis"], [np.sqrt(0.5), -np.sqrt(0.5), 0.0], rtol=0, atol=1e-4)
    syn.best = torch.tensor([[list(R.NO_POSE)]], dtype=torch.int32)
    rec = tool.putdown_arrays(syn)
    assert np.isnan(rec["putdown_center"]).all() and np.isnan(rec["putdown_axis"]).all() and rec["putdown_center"].shape == (3,)


@pytest.mark.gpu
def test_export_objects_putdown_cli(device, golden_dir, tmp_path):
    plain = export(golden_dir, tmp_path / "plain")
    assert set(plain.files) == BASE_KEYS                         # without --putdown: exactly the old keys
    z = export(golden_dir, tmp_path / "both", "--putdown", "0.30", "0.06", "--putdown-angles", "8", "--placement", "0.03")
    assert set(z.files) == BASE_KEYS | PUTDOWN_KEYS | PLACEMENT_KEYS
    for k in BASE_KEYS:
        assert np.array_equal(plain[k], z[k]), k
    assert z["putdown_fits"].shape == (256, 256) and z["putdown_count"].shape == (32,) and z["putdown_best"].shape == (8,)
    assert z["putdown_dirs"].tolist() == R.direction_table(8).tolist()
    # the stage on the exported label map, with the tool's defaults, against the reference
    from unseenobjectclustering_amd import footprint, placement, support
    xyz = demo_sample(golden_dir)["depth"][0].to(device)
    lab = torch.from_numpy(z["label_map"]).to(device)
    placed = placement.free_space(lab, xyz, support.fit_plane(lab, xyz))
    assert np.array_equal(z["place_state"], placed.state[0].cpu().numpy())
    rect = footprint.rect(0.30, 0.06, 10)
    st, ow, d2, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "dist2", "frame"))
    want = R.footprint(st, ow, d2, R.direction_table(8), [rect], 1, fr)
    assert np.array_equal(z["putdown_fits"], want["fits"][0]) and np.array_equal(z["putdown_count"], want["count"][0])
    assert np.array_equal(z["putdown_best"], want["best"][0])
    if want["best"][0, 0]:
        i, j = (int(x) for x in want["best"][0, 1:3])
        assert np.allclose(z["putdown_center"], placement.cell_to_camera(placed, 0, i, j), rtol=0, atol=1e-12)
        assert abs(np.linalg.norm(z["putdown_axis"]) - 1) < 1e-12
    else:
        assert np.isnan(z["putdown_center"]).all() and np.isnan(z["putdown_axis"]).all()
