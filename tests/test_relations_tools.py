"""Where users meet the object relations: the opt-in --relations / --relations-gap / --relations-min-pairs of
tools/export_objects.py, alone and on tracked and component-split maps (GPU: the step has no CPU path)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import relations_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_KEYS = {"frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
             "obb_center", "obb_half", "offsets", "points", "pixel_index", "label_map"}
RELATION_KEYS = {"layer", "free", "order", "n_above", "edge", "front", "touch"}
COMPONENT_KEYS = {"component_src", "component_area", "component_siblings"}


def export(golden_dir, out, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_objects.py"), "--imgdir",
                        os.path.join(golden_dir, "demo"), "--out", str(out), "--max-points", "500", *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out / "000002_objects.npz")


def demo_z(golden_dir):
    from unseenobjectclustering_amd import io as uio
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    return uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)["depth"][0, 2].numpy()


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
