"""Where users meet the object relations: the opt-in --relations / --relations-gap / --relations-min-pairs of
tools/export_objects.py, alone and on tracked and component-split maps (GPU: the step has no CPU path)."""
import numpy as np
import pytest

from tests import relations_reference as R
from tests.tool_cases import BASE_KEYS, COMPONENT_KEYS, demo_xyz, export

RELATION_KEYS = {"layer", "free", "order", "n_above", "edge", "front", "touch"}


def demo_z(golden_dir):
    return demo_xyz(golden_dir)[2]


def check_against_reference(z, depth, gap_mm, min_pairs):
    want = R.relations(z["label_map"], depth, 8, gap_mm, min_pairs)
    ids = z["label"].astype(np.int64)
    K = len(ids)
    assert K >= 1 and z["front"].shape == z["touch"].shape == (K, K)
    for k in ("layer", "free", "order", "n_above", "edge"):
        assert z[k].shape == (K,) and np.array_equal(z[k], want[k][ids]), k
    assert np.array_equal(z["front"], want["front"][np.ix_(ids, ids)]) and np.array_equal(z["touch"], want["touch"][np.ix_(ids, ids)])
    assert sorted(z["order"].tolist()) == list(range(1, K + 1))           # the exported objects are the present ids


@pytest.mark.gpu
def test_export_objects_relations_cli(device, golden_dir, tmp_path):
    plain = export(golden_dir, tmp_path / "plain")
    assert set(plain.files) == BASE_KEYS
    z = export(golden_dir, tmp_path / "rel", "--relations", "--relations-gap", "0.02", "--relations-min-pairs", "5")
    assert set(z.files) == BASE_KEYS | RELATION_KEYS
    for k in BASE_KEYS:
        assert np.array_equal(plain[k], z[k]), k
    check_against_reference(z, demo_z(golden_dir), 20, 5)


@pytest.mark.gpu
def test_export_objects_relations_on_split_and_tracked_maps_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path, "--relations", "--components", "all", "--min-area", "20", "--track")
    assert set(z.files) == BASE_KEYS | RELATION_KEYS | COMPONENT_KEYS | {"raw_label_map", "track_uid"}
    check_against_reference(z, demo_z(golden_dir), 15, 8)
