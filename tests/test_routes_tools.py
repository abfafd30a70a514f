"""Where users meet the routes stage: the opt-in --route ID RADIUS_M of tools/export_objects.py.  The argument wiring and
the arrays the tool adds are checked on the CPU (the tool's own route_arrays on a synthetic result); the command line on
the GPU (the step has no CPU path): tests/test_routes_gpu.py holds the stage against the reference end to end,
segment_objects(..., routes=True) included."""
import types

import numpy as np
import pytest
import torch

from tests import routes_reference as R
from tests.tool_cases import BASE_KEYS, PLACEMENT_KEYS, demo_sample, export, tool  # noqa: F401  (tool is a fixture)

ROUTE_KEYS = {"route_cost", "route_info", "route_path", "route_xyz", "route_length_m"}


def test_route_arguments_and_arrays(tool):
    from unseenobjectclustering_amd import placement
    base = ["--imgdir", "frames", "--out", "objs"]
    a = tool.parse_args(base)
    assert a.route is None and a.placement is None
    a = tool.parse_args(base + ["--placement", "0.04", "--route", "3", "0.05"])
    assert a.route == (3, 0.05) and a.placement == 0.04 and a.putdown is None and a.grasp is None
    for bad in (["--route", "3", "0.05"], ["--placement", "0.04", "--route", "3"], ["--placement", "0.04", "--route", "x", "0.05"],
                ["--placement", "0.04", "--route", "0", "0.05"], ["--placement", "0.04", "--route", "128", "0.05"],
                ["--placement", "0.04", "--route", "3", "-0.01"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert set(tool.ROUTE_KEYS) == ROUTE_KEYS
    planes = torch.from_numpy(placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0]))
    cost = torch.full((1, 1, 16, 16), -1, dtype=torch.int32)
    cost[0, 0, 10, 3:6] = torch.tensor([0, 5, 10], dtype=torch.int32)
    info = torch.tensor([[[1, 1, 10, 5, 10, 2, 3, 200]]], dtype=torch.int32)
    path = torch.full((1, 1, 8, 2), -1, dtype=torch.int32)
    path[0, 0, :3] = torch.tensor([[10, 5], [10, 4], [10, 3]], dtype=torch.int32)
    syn = types.SimpleNamespace(cost=cost, info=info, path=path, max_path=8, planes=planes, grid=16, cell_mm=10)
    rec = tool.route_arrays(syn)
    assert set(rec) == ROUTE_KEYS
    assert rec["route_cost"].shape == (16, 16) and rec["route_cost"].dtype == np.int32 and rec["route_cost"][10, 5] == 10
    assert rec["route_info"].tolist() == [1, 1, 10, 5, 10, 2, 3, 200]
    assert rec["route_path"].tolist() == [[10, 3], [10, 4], [10, 5]] and rec["route_path"].dtype == np.int32      # source first
    assert rec["route_xyz"].shape == (3, 3) and np.allclose(rec["route_xyz"][0], [0.025, 0.045, 1.0], rtol=0, atol=1e-12)
    assert float(rec["route_length_m"]) == 0.02
    syn.info = torch.tensor([[list(R.NO_ROUTE)]], dtype=torch.int32)
    rec = tool.route_arrays(syn)
    assert rec["route_path"].shape == (0, 2) and rec["route_xyz"].shape == (0, 3) and np.isnan(rec["route_length_m"])


@pytest.mark.gpu
def test_export_objects_route_cli(device, golden_dir, tmp_path):
    plain = export(golden_dir, tmp_path / "plain", "--placement", "0.03")
    assert set(plain.files) == BASE_KEYS | PLACEMENT_KEYS           # without --route: exactly the old keys
    a = int(plain["label"][0])
    z = export(golden_dir, tmp_path / "both", "--placement", "0.03", "--route", str(a), "0.02")
    assert set(z.files) == BASE_KEYS | PLACEMENT_KEYS | ROUTE_KEYS
    for k in BASE_KEYS | PLACEMENT_KEYS:
        assert np.array_equal(plain[k], z[k], equal_nan=k == "place_widest_xyz"), k
    assert z["route_cost"].shape == (256, 256) and z["route_info"].shape == (8,) and z["route_path"].shape[1] == 2
    # the stage on the exported label map, with the tool's defaults, against the reference
    from unseenobjectclustering_amd import placement, routes, support
    xyz = demo_sample(golden_dir)["depth"][0].to(device)
    lab = torch.from_numpy(z["label_map"]).to(device)
    fitted = support.fit_plane(lab, xyz)
    placed = placement.free_space(lab, xyz, fitted)
    assert np.array_equal(z["place_state"], placed.state[0].cpu().numpy())
    spot = tuple(int(x) for x in z["place_widest_cell"][:2])
    query = routes.of_object(placed, fitted, 0, a, spot if spot[0] >= 0 else None, radius_m=0.02)
    assert query[0] == 9 and query[5] == a
    st, ow, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "frame"))
    want = R.routes(st, ow, [query], 1, 1024, fr)
    assert np.array_equal(z["route_cost"], want["cost"][0]) and np.array_equal(z["route_info"], want["info"][0])
    n = int(want["info"][0, 5]) + 1 if want["info"][0, 2] >= 0 else 0
    assert np.array_equal(z["route_path"], want["path"][0, :n][::-1])
    if n:
        assert z["route_path"][0].tolist() == list(query[1:3]) and z["route_xyz"].shape == (n, 3)
        assert np.allclose(z["route_xyz"][-1], placement.cell_to_camera(placed, 0, *z["route_path"][-1]), rtol=0, atol=1e-12)
        assert float(z["route_length_m"]) == int(want["info"][0, 4]) * 10 / 5000.0
    else:
        assert np.isnan(z["route_length_m"])
