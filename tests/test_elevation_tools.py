"""Where users meet the elevation stage: segment_objects(..., elevation=True) and the opt-in --elevation STEP_M /
--elevation-min-pts of tools/export_objects.py.  The argument wiring and the arrays the tool adds are checked on the CPU
(the tool's own elevation_arrays on a synthetic result); the command line and segment_objects on the GPU (the step has
no CPU path): tests/test_elevation_gpu.py holds the stage against the reference end to end."""
import types

import numpy as np
import pytest
import torch

from tests import elevation_reference as R
from tests.tool_cases import BASE_KEYS, PLACEMENT_KEYS, demo_sample, export, tool  # noqa: F401  (tool is a fixture)

ELEVATION_KEYS = {"top_cells", "top_level", "top_cell", "top_clear_m", "top_height_m", "top_xyz"}


def test_elevation_arguments_and_arrays(tool):
    base = ["--imgdir", "frames", "--out", "objs"]
    a = tool.build_parser().parse_args(base)
    assert a.elevation is None and a.elevation_min_pts == 2
    a = tool.build_parser().parse_args(base + ["--elevation", "0.005"])
    assert a.elevation == 0.005 and a.placement is None and a.grasp is None and not a.plane      # placement and the plane are implied at run time
    a = tool.build_parser().parse_args(base + ["--elevation", "0.01", "--elevation-min-pts", "3", "--grid", "128", "--placement", "0.04"])
    assert (a.elevation, a.elevation_min_pts, a.grid, a.placement) == (0.01, 3, 128, 0.04)
    assert set(tool.ELEVATION_KEYS) == ELEVATION_KEYS
    tops = torch.zeros((1, 128, 8), dtype=torch.int32)
    tops[0, :, 2:4] = -1
    tops[0, 3] = torch.tensor([9, 4, 7, 9, 4, 50, 52, 50], dtype=torch.int32)
    tops[0, 5] = torch.tensor([6, 0, -1, -1, 0, 0, 31, 0], dtype=torch.int32)
    syn = types.SimpleNamespace(frame=torch.from_numpy(R.frame_record(R.flat_plane()))[None], grid=16, cell_mm=10, tops=tops)
    rec = tool.elevation_arrays(syn, [5, 3])
    assert set(rec) == ELEVATION_KEYS
    assert rec["top_cells"].tolist() == [6, 9] and rec["top_level"].tolist() == [0, 4] and rec["top_cell"].tolist() == [[-1, -1], [7, 9]]
    assert np.isnan(rec["top_clear_m"][0]) and np.isnan(rec["top_height_m"][0]) and np.isnan(rec["top_xyz"][0]).all()
    assert abs(rec["top_clear_m"][1] - 0.02) < 1e-12 and rec["top_height_m"][1] == 0.05
    assert np.allclose(rec["top_xyz"][1], [-0.005, -0.015, 0.95], rtol=0, atol=1e-12) and rec["top_xyz"].shape == (2, 3)
    assert tool.elevation_arrays(syn, [5, 3], 0.01)["top_fits"].tolist() == [False, True]        # need2 = 4
    assert tool.elevation_arrays(syn, [5, 3], 0.011)["top_fits"].tolist() == [False, False]      # need2 = 9
    assert tool.elevation_arrays(syn, [])["top_xyz"].shape == (0, 3)


def check_rows(z, fits):
    n = len(z["label"])
    assert n >= 1
    for k, shape, dt in (("top_cells", (n,), np.int32), ("top_level", (n,), np.int32), ("top_cell", (n, 2), np.int32),
                         ("top_clear_m", (n,), np.float64), ("top_height_m", (n,), np.float64), ("top_xyz", (n, 3), np.float64)):
        assert z[k].shape == shape and z[k].dtype == dt, (k, z[k].shape, z[k].dtype)
    none = z["top_level"] == 0
    assert (z["top_level"] <= z["top_cells"]).all() and (z["top_level"] >= 0).all()
    assert (z["top_cell"][none] == -1).all() and (z["top_cell"][~none] >= 0).all()
    for k in ("top_clear_m", "top_height_m"):
        assert np.isnan(z[k][none]).all() and np.isfinite(z[k][~none]).all(), k
    assert np.isnan(z["top_xyz"][none]).all() and np.isfinite(z["top_xyz"][~none]).all()
    assert (z["top_clear_m"][~none] >= 0.01).all()               # a level cell is at least one cell from a blocking one
    if fits:
        assert z["top_fits"].shape == (n,) and z["top_fits"].dtype == bool and not z["top_fits"][none].any()


@pytest.mark.gpu
def test_export_objects_elevation_cli(device, golden_dir, tmp_path):
    plain = export(golden_dir, tmp_path / "plain")
    assert set(plain.files) == BASE_KEYS                         # without --elevation: exactly the old keys
    z = both = export(golden_dir, tmp_path / "both", "--elevation", "0.005", "--elevation-min-pts", "2", "--placement", "0.03")
    assert set(both.files) == BASE_KEYS | ELEVATION_KEYS | PLACEMENT_KEYS | {"top_fits"}      # top_fits only with --placement: see the CPU test
    for k in BASE_KEYS:
        assert np.array_equal(plain[k], both[k]), k
    check_rows(both, True)
    level = both["top_level"] > 0
    assert np.array_equal(both["top_fits"][level], both["top_clear_m"][level] >= 0.04 - 1e-12)      # need2 = (3 + 1)^2 cells of 1 cm
    # top_cell agrees with tops: the stage on the exported label map, with the tool's defaults
    from unseenobjectclustering_amd import elevation, placement, support
    xyz = demo_sample(golden_dir)["depth"][0].to(device)
    lab = torch.from_numpy(z["label_map"]).to(device)
    placed = placement.free_space(lab, xyz, support.fit_plane(lab, xyz))
    res = elevation.heights(lab, xyz, placed)
    tops = res.tops[0].cpu().numpy()[z["label"].astype(np.int64)]
    assert np.array_equal(z["top_cells"], tops[:, 0]) and np.array_equal(z["top_level"], tops[:, 1]) and np.array_equal(z["top_cell"], tops[:, 2:4])
    want = R.heights(z["label_map"], xyz.cpu().numpy(), placed.frame[0].cpu().numpy(), 256, 10, 10, 5, 2)
    assert np.array_equal(res.tops[0].cpu().numpy(), want["tops"]) and want["info"][0] == 1


def _demo(golden_dir):
    from unseenobjectclustering_amd import networks, synth
    sample = demo_sample(golden_dir)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


@pytest.mark.gpu
def test_segment_objects_with_elevation_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out0, ref0, objs0 = O.segment_objects(sample, net, net_crop)
    np.random.seed(3)
    q = [(1, -1, *R.BAND)]
    out1, ref1, objs1, fitted, placed, raised = O.segment_objects(sample, net, net_crop, elevation=True, elevation_args=dict(queries=q))
    assert torch.equal(out0, out1) and ref0 is not None and torch.equal(ref0, ref1) and torch.equal(objs0.centroid, objs1.centroid)
    assert hasattr(fitted, "normal") and hasattr(placed, "state") and raised.frame.data_ptr() == placed.frame.data_ptr()
    for k, shape, dt in (("elev", (1, 256, 256), torch.int32), ("owner", (1, 256, 256), torch.int32), ("pts", (1, 256, 256), torch.int32),
                         ("near", (1, 256, 256), torch.int32), ("dist2", (1, 256, 256), torch.int32), ("tops", (1, 128, 8), torch.int32),
                         ("info", (1, 4), torch.int32), ("answers", (1, 1, 4), torch.int32), ("frame", (1, 16), torch.int64)):
        t = getattr(raised, k)
        assert tuple(t.shape) == shape and t.dtype == dt and t.device.type == "cuda", k
    assert (raised.grid, raised.cell_mm, raised.tau_mm, raised.step_mm, raised.min_pts, raised.queries) == (256, 10, 10, 5, 2, q)
    lab, xyz = ref1[0].numpy().astype(np.int32), sample["depth"][0].numpy()
    want = R.heights(lab, xyz, placed.frame[0].cpu().numpy(), 256, 10, 10, 5, 2, q)
    for k in R.FIELDS:
        assert np.array_equal(getattr(raised, k)[0].cpu().numpy(), want[k]), k
    assert want["info"][0] == 1 and want["info"][3] > 100
    np.random.seed(3)
    every = O.segment_objects(sample, net, net_crop, plane=True, relations=True, placement=True, grasp=True, elevation=True)
    assert len(every) == 8 and hasattr(every[6], "best") and torch.equal(every[7].elev, raised.elev) and torch.equal(every[5].state, placed.state)
