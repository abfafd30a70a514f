"""Where users meet the grasp stage: the opt-in --grasp MAX_OPEN_M / --grasp-angles / --grasp-offsets of
tools/export_objects.py.  The argument wiring and the arrays the tool adds are checked on the CPU (the tool's own
grasp_arrays on a synthetic result); the command line itself on the GPU (the step has no CPU path), its arrays against
each other: tests/test_grasp_gpu.py holds the stage against the reference end to end."""
import numpy as np
import pytest
import torch

from tests import grasp_reference as R
from tests.tool_cases import BASE_KEYS, export, tool  # noqa: F401  (tool is a fixture)

GRASP_KEYS = {"grasp_best", "grasp_cand", "grasp_dirs", "grasp_center", "grasp_axis", "grasp_width", "grasp_opening"}
S = 16384


def test_grasp_arguments(tool):
    base = ["--imgdir", "frames", "--out", "objs"]
    a = tool.build_parser().parse_args(base)
    assert a.grasp is None and a.placement is None and (a.grasp_angles, a.grasp_offsets, a.grid, a.cell_mm) == (16, 2, 256, 10)
    a = tool.build_parser().parse_args(base + ["--grasp", "0.085"])
    assert a.grasp == 0.085 and a.placement is None and not a.plane              # placement and the plane are implied at run time
    a = tool.build_parser().parse_args(base + ["--grasp", "0.06", "--grasp-angles", "8", "--grasp-offsets", "0", "--grid", "128",
                                               "--cell-mm", "5", "--placement", "0.04"])
    assert (a.grasp, a.grasp_angles, a.grasp_offsets, a.grid, a.cell_mm, a.placement) == (0.06, 8, 0, 128, 5, 0.04)
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(base + ["--grasp"])
    assert set(tool.GRASP_KEYS) == GRASP_KEYS and "--grasp MAX_OPEN_M" in tool.__doc__


def test_grasp_arrays_of_a_synthetic_result(tool):
    from unseenobjectclustering_amd import grasp, placement
    A, M = 4, 1
    best = torch.zeros((1, 128, 8), dtype=torch.int32)
    cand = torch.zeros((1, 128, A, 2 * M + 1, 2), dtype=torch.int32)
    best[0, 5] = torch.tensor([1, 2, 0, -1, 3, 10 * S, 12 * S + S // 2, 4])
    cand[0, 5, 2, M] = torch.tensor([3, -1])
    best[0, 9] = torch.tensor([0, -1, 0, 0, 0, 3 * S, 3 * S, 0])
    planes = torch.from_numpy(placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0]))
    res = grasp.GraspResult(cand=cand, best=best, dirs=grasp.direction_table(A), angles=A, offsets=M, max_open=8, gap=1, finger=1, pad=1,
                            unknown_blocks=True, grid=32, cell_mm=10, planes=planes)
    rec = tool.grasp_arrays(res, [9, 5])
    assert set(rec) == GRASP_KEYS
    assert rec["grasp_best"].tolist() == [best[0, 9].tolist(), best[0, 5].tolist()] and rec["grasp_cand"].shape == (2, A, 3, 2)
    assert np.array_equal(rec["grasp_cand"][1], cand[0, 5].numpy()) and np.array_equal(rec["grasp_dirs"], R.direction_table(A))
    assert np.isnan(rec["grasp_center"][0]).all() and np.isnan(rec["grasp_axis"][0]).all() and np.isnan(rec["grasp_width"][0])
    # k = 2 of 4 closes along v = -y; the middle of t = -1..1 is the anchor (10, 12.5) cells: -6 and -3.5 cells from the centre
    assert np.allclose(rec["grasp_center"][1], [-0.06, 0.035, 1.0], rtol=0, atol=1e-9)
    assert np.allclose(rec["grasp_axis"][1], [0, -1, 0], rtol=0, atol=1e-9)
    assert np.allclose([rec["grasp_width"][1], rec["grasp_opening"][1]], [0.03, 0.05], rtol=0, atol=1e-12)
    empty = tool.grasp_arrays(res, [])
    assert empty["grasp_center"].shape == (0, 3) and empty["grasp_best"].shape == (0, 8) and empty["grasp_width"].shape == (0,)


@pytest.mark.gpu
def test_export_objects_grasp_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path, "--grasp", "0.085")         # placement and the plane are implied, their arrays are not added
    assert set(z.files) == BASE_KEYS | GRASP_KEYS
    K = len(z["label"])
    assert z["grasp_best"].shape == (K, 8) and z["grasp_cand"].shape == (K, 16, 5, 2) and z["grasp_center"].shape == (K, 3)
    # the arrays against each other (tests/test_grasp_gpu.py holds the stage against the reference end to end)
    ok = z["grasp_best"][:, 0] == 1
    assert np.array_equal(np.isnan(z["grasp_width"]), ~ok) and np.array_equal(np.isnan(z["grasp_center"]).any(axis=1), ~ok)
    assert np.allclose(z["grasp_width"][ok], z["grasp_best"][ok, 4] * 0.01) and np.allclose(z["grasp_opening"][ok], (z["grasp_best"][ok, 4] + 2) * 0.01)
    assert np.allclose(np.linalg.norm(z["grasp_axis"][ok], axis=1), 1.0) and np.array_equal(z["grasp_dirs"], R.direction_table(16))
    assert np.array_equal((z["grasp_cand"][..., 0] > 0).sum(axis=(1, 2)), z["grasp_best"][:, 7])
