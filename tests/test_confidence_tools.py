"""Where users meet the confidence stage: the opt-in --confidence [WEAK] of tools/export_objects.py.  The argument wiring and
the arrays the tool adds are checked on the CPU (the tool's own confidence_arrays on a synthetic summary); the command
line on the GPU (the stage has no CPU path): tests/test_confidence_gpu.py holds the stage against the reference end to
end, segment_objects(..., confidence=True) included."""
import types

import numpy as np
import pytest
import torch

from tests import confidence_reference as R
from tests.tool_cases import BASE_KEYS, export, tool  # noqa: F401  (tool is a fixture)

CONFIDENCE_KEYS = {"conf_map", "conf_mean", "conf_min", "conf_weak_share"}


def test_confidence_arguments_and_arrays(tool):
    base = ["--imgdir", "frames", "--out", "objs"]
    assert tool.parse_args(base).confidence is None
    assert tool.parse_args(base + ["--confidence"]).confidence == 0.02
    assert tool.parse_args(base + ["--confidence", "0.1", "--plane"]).confidence == 0.1
    for bad in (["--confidence", "-0.1"], ["--confidence", "1.5"], ["--confidence", "x"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert set(tool.CONFIDENCE_KEYS) == CONFIDENCE_KEYS
    mean = np.full((1, 128), np.nan)
    mean[0, [2, 5]] = [0.25, 0.5]
    syn = types.SimpleNamespace(mean=mean, min=mean / 2, weak_share=np.where(np.isnan(mean), np.nan, 0.125))
    rec = tool.confidence_arrays(syn, torch.tensor([5, 2]), torch.full((3, 4), 0.75))
    assert set(rec) == CONFIDENCE_KEYS
    assert rec["conf_map"].shape == (3, 4) and rec["conf_map"].dtype == np.float32 and (rec["conf_map"] == 0.75).all()
    assert rec["conf_mean"].tolist() == [0.5, 0.25] and rec["conf_min"].tolist() == [0.25, 0.125]
    assert rec["conf_weak_share"].tolist() == [0.125, 0.125] and rec["conf_mean"].dtype == np.float64


@pytest.mark.gpu
def test_export_objects_confidence_cli(device, golden_dir, tmp_path):
    plain = export(golden_dir, tmp_path / "plain")
    assert set(plain.files) == BASE_KEYS                            # without --confidence: exactly the old keys
    z = export(golden_dir, tmp_path / "conf", "--confidence", "0.05")
    assert set(z.files) == BASE_KEYS | CONFIDENCE_KEYS
    for k in BASE_KEYS:
        assert np.array_equal(plain[k], z[k]), k
    K = len(z["label"])
    H, W = z["label_map"].shape
    assert K >= 1 and z["conf_map"].shape == (H, W) and z["conf_map"].dtype == np.float32
    for k in ("conf_mean", "conf_min", "conf_weak_share"):
        assert z[k].shape == (K,) and z[k].dtype == np.float64, k
    assert (z["conf_map"] >= 0).all() and (z["conf_map"] <= 1).all()
    # the per-object rows are the integer summary of (exported label map, exported margin map)
    want = R.objects(z["label_map"][None], z["conf_map"][None], 3277)[0]      # ceil(0.05 * 65536)
    ids = z["label"].astype(int)
    assert np.array_equal(want[ids, 0], z["pixels"])
    assert np.array_equal(z["conf_mean"], want[ids, 1].astype(np.float64) / want[ids, 0] / 65536)
    assert np.array_equal(z["conf_min"], want[ids, 2].astype(np.float64) / 65536)
    assert np.array_equal(z["conf_weak_share"], want[ids, 3].astype(np.float64) / want[ids, 0])
