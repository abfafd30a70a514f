"""What the tests of tools/export_objects.py (tests/test_*_tools.py, tests/test_export_tools_gpu.py) share: the tool as a
module, the tool as a command on the committed demo frame, that frame's sample, and the key sets every stage's test names."""
import importlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_KEYS = {"frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
             "obb_center", "obb_half", "offsets", "points", "pixel_index", "label_map"}
PLACEMENT_KEYS = {"place_state", "place_dist2", "place_widest_cell", "place_widest_xyz"}
PLANE_KEYS = {"plane_" + k for k in ("found", "candidates", "inliers", "hyp", "normal", "d", "centroid", "eig", "rms", "u", "v")} \
    | {"height_min", "height_max", "foot", "cov2", "upright_axis", "upright_half", "upright_center"}
COMPONENT_KEYS = {"component_src", "component_area", "component_siblings"}


@pytest.fixture(scope="module")
def tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        yield importlib.import_module("export_objects")
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))


def run_tool(imgdir, out, *flags):
    """The tool as a command on the frames of `imgdir`; the finished process, whatever its return code."""
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_objects.py"), "--imgdir", str(imgdir), "--out", str(out), *flags],
                          capture_output=True, text=True, timeout=600, cwd=ROOT)


def export(golden_dir, out, *flags):
    """The tool on the committed demo frame with 500 points per object; the file it wrote."""
    r = run_tool(os.path.join(golden_dir, "demo"), out, "--max-points", "500", *flags)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out / "000002_objects.npz")


def demo_frames(golden_dir, frames, n=2):
    """A stream in which nothing moves: the demo frame n times, as 000002, 000003, ... in the new directory `frames`."""
    frames.mkdir()
    for k in range(2, 2 + n):
        for kind in ("color", "depth"):
            shutil.copy(os.path.join(golden_dir, "demo", f"000002-{kind}.png"), frames / f"{k:06d}-{kind}.png")
    shutil.copy(os.path.join(golden_dir, "demo", "camera_params.json"), frames / "camera_params.json")
    return frames


def demo_sample(golden_dir):
    """The demo frame as the tool's loader reads it."""
    from unseenobjectclustering_amd import io as uio
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    return uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)


def demo_xyz(golden_dir):
    return demo_sample(golden_dir)["depth"][0].numpy()
