"""Where users meet the re-identification: the opt-in --reid of the ROS node (ros/segmentation_tracked.py) and of
tools/export_objects.py, both on top of --track.  A stub segmentation whose second object jumps to a place that shares no
pixel with the old one comes out with a new track slot under --track alone and with the same id under --reid (GPU: the
stages have no CPU path).  The argument errors are in tests/test_identity_host.py."""
import os

import numpy as np
import pytest
import torch

from tests import fake_ros
from tests.test_ros_node import K
from tests.test_tracking_tools import load_tracked_module, rosmod  # noqa: F401  (rosmod is a fixture)
from tests.tool_cases import run_tool
from unseenobjectclustering_amd.fcn.config import cfg

pytestmark = pytest.mark.gpu

H, W, JUMP = 48, 64, 3


def boxes(k):
    """Frame k: object A drifts one pixel per frame, object B jumps at frame JUMP."""
    return (5, 4 + k, 15, 20), ((25, 4, 12, 16) if k < JUMP else (30, 44, 12, 16))


def frame(k):
    rng = np.random.default_rng(100 + k)
    im = np.full((H, W, 3), 90, dtype=np.int64)
    for (y, x, h, w), colour in zip(boxes(k), ((40, 40, 200), (200, 60, 40))):
        im[y:y + h, x:x + w] = colour
    im = np.clip(im + rng.integers(-5, 6, size=im.shape), 0, 255).astype(np.uint8)
    return im, np.full((H, W), 1000, dtype=np.uint16)


def jumping_segment():
    calls = []

    def segment(sample, network, network_crop):
        k = len(calls)
        calls.append(sample)
        a, b = [(1, 2), (2, 1), (7, 3), (90, 127)][k % 4]              # the raw ids change with every call
        label = torch.zeros(1, H, W)
        for (y, x, h, w), rid in zip(boxes(k), (a, b)):
            label[0, y:y + h, x:x + w] = rid
        return label, label.clone()
    return segment


def expected(k, ids=(1, 2)):
    want = np.zeros((H, W), np.uint8)
    for (y, x, h, w), i in zip(boxes(k), ids):
        want[y:y + h, x:x + w] = i
    return want


def test_reid_publishes_the_same_id_after_a_jump(rosmod, device):
    cfg.device = device
    tracked = load_tracked_module()
    plain = tracked.make_node(rosmod, "net", "crop", fake_ros.make(K), segment=jumping_segment(), track=True)
    reid = tracked.make_node(rosmod, "net", "crop", fake_ros.make(K), segment=jumping_segment(), track=True,
                             reid=dict(min_sim=0.7, min_size=0.25, max_lost=300))
    assert plain.segment.identifiers == {} and set(reid.segment.identifiers) == {"seg_label", "seg_label_refined"}
    for k in range(6):
        im, dep = frame(k)
        for node in (plain, reid):
            node.on_rgbd(fake_ros.Image(im, "bgr8", "cam", stamp=float(k)), fake_ros.Image(dep, "16UC1"))
            assert node.spin_once() is True
        for topic in ("seg_label", "seg_label_refined"):
            msg = reid.pub[topic].sent[k]
            assert msg.encoding == "mono8" and msg.data.dtype == np.uint8 and msg.header.stamp == float(k)
            assert np.array_equal(msg.data, expected(k)), (topic, k)                       # B keeps id 2 across the jump
            assert np.array_equal(plain.pub[topic].sent[k].data, expected(k, (1, 2 if k < JUMP else 3))), (topic, k)
    for topic, ident in reid.segment.identifiers.items():
        rec = ident.identities()
        assert rec["entry"].tolist() == [1, 2] and rec["pid"].tolist() == [1, 2] and rec["hits"].tolist() == [6, 6], topic
        assert rec["uid"].tolist() == [1, 3] and rec["evicted"] == 0                      # the track changed, the identity did not


def test_export_objects_reid_cli(device, golden_dir, tmp_path):
    r = run_tool(os.path.join(golden_dir, "demo"), tmp_path, "--max-points", "500", "--track", "--reid")
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(tmp_path / "000002_objects.npz")
    assert {"identity", "identity_pid", "identity_map", "label_map", "raw_label_map", "track_uid"} <= set(z.files)
    tracked, who = z["label_map"], z["identity_map"]
    n = len(np.unique(tracked)) - 1
    assert n >= 1 and who.dtype == np.int32 and who.shape == tracked.shape and np.array_equal(who > 0, tracked > 0)
    assert np.array_equal(z["label"], z["track_uid"])                                      # the --track keys are as they were
    assert z["identity"].tolist() == z["label"].tolist() and z["identity_pid"].tolist() == z["label"].tolist()   # first frame
    for lab, entry in zip(z["label"], z["identity"]):
        assert (who[tracked == lab] == entry).all()
