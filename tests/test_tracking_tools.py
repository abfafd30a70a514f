"""Where users meet the tracker: the opt-in --track of the ROS node (ros/segmentation_tracked.py, which wraps the
segmentation call of the unchanged node in ros/test_images_segmentation.py) and of tools/export_objects.py.  Without the
flag the node publishes exactly what it published before (CPU); with it, a stub segmentation that re-numbers its objects
every frame comes out with constant ids (GPU: the tracker has no CPU path)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import fake_ros
from tests.test_ros_node import K, frame, load_node_module, stub_segment
from tests.tool_cases import ROOT, run_tool
from unseenobjectclustering_amd.fcn.config import cfg


def load_tracked_module():
    spec = importlib.util.spec_from_file_location("uoc_ros_tracked", os.path.join(ROOT, "ros", "segmentation_tracked.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def rosmod():
    saved = cfg.TEST.ROS_CAMERA, cfg.TEST.SCALES_BASE, cfg.INPUT, cfg.device
    cfg.TEST.SCALES_BASE, cfg.TEST.ROS_CAMERA, cfg.INPUT = (1.0,), "camera", "RGBD"
    yield load_node_module()
    cfg.TEST.ROS_CAMERA, cfg.TEST.SCALES_BASE, cfg.INPUT, cfg.device = saved


def permuting_segment(calls):
    """Two rectangles that drift one pixel per frame; their raw ids change with every call."""
    def segment(sample, network, network_crop):
        k = len(calls)
        calls.append(sample)
        a, b = [(1, 2), (2, 1), (7, 3), (90, 127)][k % 4]
        label = torch.zeros(1, 48, 64)
        label[0, 5:20, 4 + k:24 + k] = a
        label[0, 25:40, 40 - k:60 - k] = b
        refined = torch.where(label > 0, label % 100 + 20, label)     # another numbering on the refined topic
        return label, refined
    return segment


def permuting_segment_no_crop():
    inner = permuting_segment([])
    return lambda sample, network, network_crop: (inner(sample, network, network_crop)[0], None)


def expected(k):
    want = np.zeros((48, 64), np.uint8)
    want[5:20, 4 + k:24 + k] = 1
    want[25:40, 40 - k:60 - k] = 2
    return want


def test_flag_is_off_by_default_and_the_published_bytes_are_unchanged(rosmod):
    tracked = load_tracked_module()
    assert tracked.parse_args(rosmod, []).track is False
    args = tracked.parse_args(rosmod, ["--track", "--track_max_age", "2", "--gpu", "1", "--pretrained", "a.pth"])
    assert args.track is True and args.track_max_age == 2 and args.track_min_iou == 0.3
    assert args.gpu_id == 1 and args.pretrained == "a.pth" and args.network_name == "seg_resnet34_8s_embedding"
    with pytest.raises(SystemExit):
        tracked.main(["--track"], ros=fake_ros.make(K))                        # no checkpoint, no node: as the base node
    calls = []
    segment = stub_segment(calls)
    node = tracked.make_node(rosmod, "net", "crop", fake_ros.make(K), segment=segment)
    assert type(node) is rosmod.SegmentationNode and node.segment is segment   # no wrapper without the flag
    for seed in (1, 2):
        im, dep = frame(seed)
        node.on_rgbd(fake_ros.Image(im, "bgr8", "cam", stamp=float(seed)), fake_ros.Image(dep, "16UC1"))
        assert node.spin_once() is True
        z = dep.astype(np.float32) / 1000.0
        label = (z > 1.0).astype(np.uint8) + (z > 2.0).astype(np.uint8)
        lab_msg, ref_msg = node.pub["seg_label"].sent[-1], node.pub["seg_label_refined"].sent[-1]
        assert lab_msg.encoding == "mono8" and lab_msg.data.dtype == np.uint8 and np.array_equal(lab_msg.data, label)
        assert ref_msg.encoding == "mono8" and ref_msg.data.dtype == np.uint8 and np.array_equal(ref_msg.data, 2 * label)
    # the raw ids of a re-numbering segmentation go out as they are
    node = tracked.make_node(rosmod, "net", "crop", fake_ros.make(K), segment=permuting_segment([]))
    im, dep = frame(3)
    for k in range(2):
        node.on_rgbd(fake_ros.Image(im, "bgr8"), fake_ros.Image(dep, "16UC1"))
        node.spin_once()
    assert np.array_equal(node.pub["seg_label"].sent[1].data == 2, expected(1) == 1)


@pytest.mark.gpu
def test_track_publishes_constant_ids(rosmod, device):
    cfg.device = device
    tracked = load_tracked_module()
    node = tracked.make_node(rosmod, "net", "crop", fake_ros.make(K), segment=permuting_segment([]), track=True)
    trackers = node.segment.trackers
    assert set(trackers) == {"seg_label", "seg_label_refined"}
    im, dep = frame(4)
    for k in range(8):
        node.on_rgbd(fake_ros.Image(im, "bgr8", "cam", stamp=float(k)), fake_ros.Image(dep, "16UC1"))
        assert node.spin_once() is True
        for topic in ("seg_label", "seg_label_refined"):
            msg = node.pub[topic].sent[k]
            assert msg.encoding == "mono8" and msg.data.dtype == np.uint8 and msg.header.stamp == float(k)
            assert np.array_equal(msg.data, expected(k)), (topic, k)
        assert len(node.pub["seg_image"].sent) == k + 1 and len(node.pub["seg_image_refined"].sent) == k + 1
    for tr in trackers.values():
        live = tr.tracks()
        assert live["uid"].tolist() == [1, 2] and live["hits"].tolist() == [8, 8] and live["dropped"] == 0
    # without a crop network there is no refined map: nothing to track or publish on that topic
    node = tracked.make_node(rosmod, "net", None, fake_ros.make(K), segment=permuting_segment_no_crop(), track=True)
    node.on_rgbd(fake_ros.Image(im, "bgr8"), fake_ros.Image(dep, "16UC1"))
    assert node.spin_once() is True and not node.pub["seg_label_refined"].sent
    assert np.array_equal(node.pub["seg_label"].sent[0].data, expected(0))
    assert node.segment.trackers["seg_label_refined"].tracks()["step"] == 0


@pytest.mark.gpu
def test_export_objects_track_cli(device, golden_dir, tmp_path):
    r = run_tool(os.path.join(golden_dir, "demo"), tmp_path, "--max-points", "500", "--track")
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(tmp_path / "000002_objects.npz")
    raw, tracked = z["raw_label_map"], z["label_map"]
    n = len(np.unique(raw)) - 1
    assert n >= 1 and np.array_equal(np.unique(tracked), np.arange(n + 1))     # first frame: slots 1..n
    assert np.array_equal(tracked > 0, (raw >= 1) & (raw <= 127))
    for s in range(1, n + 1):                                                    # a renumbering of the raw map
        assert len(np.unique(raw[tracked == s])) == 1
    assert np.array_equal(z["label"], z["track_uid"]) and set(z["label"].tolist()) <= set(range(1, n + 1))
    for lab, px in zip(z["label"], z["pixels"]):
        assert px == int((tracked == lab).sum())
