"""Where users meet the component split: the opt-in --components / --min-area of tools/export_objects.py (GPU: the step
has no CPU path)."""
import numpy as np
import pytest

from tests import components_reference as R
from tests.tool_cases import BASE_KEYS, COMPONENT_KEYS, export


@pytest.mark.gpu
def test_export_objects_components_largest_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path, "--components", "largest", "--min-area", "20")
    assert set(z.files) == BASE_KEYS | COMPONENT_KEYS
    label_map = z["label_map"]
    _, comps = R.components(label_map, 8)
    ids = [src for _, _, src in comps]
    assert len(ids) >= 1 and len(set(ids)) == len(ids)                    # every id is one connected piece ...
    assert all(area >= 20 for _, area, _ in comps)                        # ... of at least min_area pixels
    assert sorted(z["label"].tolist()) == sorted(ids)
    assert np.array_equal(z["component_src"], z["label"]) and np.array_equal(z["component_area"], z["pixels"])
    assert (z["component_siblings"] >= 1).all()
    for lab, px in zip(z["label"], z["pixels"]):
        assert px == int((label_map == lab).sum())


@pytest.mark.gpu
def test_export_objects_components_all_with_track_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path, "--components", "all", "--min-area", "20", "--track")
    assert set(z.files) == BASE_KEYS | COMPONENT_KEYS | {"raw_label_map", "track_uid"}
    split, tracked = z["raw_label_map"], z["label_map"]                   # the tracker was fed the split map
    _, comps = R.components(split, 8)
    n = len(comps)
    assert n >= 1 and np.array_equal(np.unique(split), np.arange(n + 1))  # pieces numbered 1..n, each connected
    assert sorted(src for _, _, src in comps) == list(range(1, n + 1))
    assert np.array_equal(tracked > 0, split > 0)
    area_of = {src: area for _, area, src in comps}
    for lab, px, area, src in zip(z["label"], z["pixels"], z["component_area"], z["component_src"]):
        piece = np.unique(split[tracked == lab])
        assert len(piece) == 1 and area_of[int(piece[0])] == area == px and 1 <= src <= 127
