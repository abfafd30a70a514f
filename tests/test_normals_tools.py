"""Where users meet the surface-normal stage: the opt-in --normals of tools/export_objects.py.  The argument wiring and the
arrays the tool adds are checked on the CPU (the tool's own normals_arrays on a synthetic result); the command line on
the GPU (the stage has no CPU path): tests/test_normals_gpu.py holds the stage against the reference end to end,
segment_objects(..., normals=True) included."""
import os
import types

import numpy as np
import pytest
import torch

from tests import normals_reference as R
from tests import placement_reference as S15
from tests.tool_cases import BASE_KEYS, demo_sample, run_tool, tool  # noqa: F401  (tool is a fixture)

NORMALS_KEYS = {"normal", "normal_info", "faces"}


def test_normals_arguments_and_arrays(tool):
    base = ["--imgdir", "frames", "--out", "objs"]
    assert tool.parse_args(base).normals is False
    assert tool.parse_args(base + ["--normals"]).normals is True
    assert tool.parse_args(base + ["--normals", "--plane", "--confidence"]).normals is True
    with pytest.raises(SystemExit):
        tool.parse_args(base + ["--normals", "3"])
    assert set(tool.NORMALS_KEYS) == NORMALS_KEYS
    packed = torch.arange(2 * 3 * 4 * 4, dtype=torch.int32).reshape(2, 3, 4, 4)
    faces = torch.arange(2 * 128 * 40, dtype=torch.int32).reshape(2, 128, 40)
    syn = types.SimpleNamespace(n=packed[..., :3], info=packed[..., 3], faces=faces)
    rec = tool.normals_arrays(syn, torch.tensor([5, 2]).tolist())
    assert set(rec) == NORMALS_KEYS
    assert rec["normal"].shape == (3, 4, 3) and rec["normal"].dtype == np.int32 and rec["normal"][1, 2].tolist() == [24, 25, 26]
    assert rec["normal_info"].shape == (3, 4) and rec["normal_info"][1, 2] == 27
    assert rec["faces"].shape == (2, 40) and rec["faces"][:, 0].tolist() == [200, 80]
    assert tool.normals_arrays(syn, [])["faces"].shape == (0, 40)


@pytest.mark.gpu
def test_export_objects_normals_cli(device, golden_dir, tmp_path):
    r = run_tool(os.path.join(golden_dir, "demo"), tmp_path, "--max-points", "500", "--normals", "--plane")
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(tmp_path / "000002_objects.npz")
    assert NORMALS_KEYS <= set(z.files) and BASE_KEYS <= set(z.files)
    K = len(z["label"])
    H, W = z["label_map"].shape
    assert K >= 1 and z["normal"].shape == (H, W, 3) and z["normal_info"].shape == (H, W) and z["faces"].shape == (K, 40)
    assert all(z[k].dtype == np.int32 for k in NORMALS_KEYS)
    ids = z["label"].astype(int)
    assert np.array_equal(z["faces"][:, 0], z["pixels"])
    # the exported arrays are the reference's on the exported label map and plane; the frame's cloud comes from the tool's loader
    sample = demo_sample(golden_dir)
    plane = dict(found=int(z["plane_found"]), normal=z["plane_normal"], d=z["plane_d"], centroid=z["plane_centroid"], u=z["plane_u"],
                 v=z["plane_v"])
    assert S15.frame_record(plane)[13] == 1
    want = R.estimate(sample["depth"][0].numpy(), z["label_map"], plane)
    assert np.array_equal(z["normal"], want["n"]) and np.array_equal(z["normal_info"], want["info"])
    assert np.array_equal(z["faces"], want["faces"][ids])
    assert (z["normal_info"] & 7 == R.UP).sum() > 1000
