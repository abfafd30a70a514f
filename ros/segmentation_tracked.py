#!/usr/bin/env python
"""The ROS node of ros/test_images_segmentation.py with an opt-in `--track` (no reference counterpart): the same
subscriptions, topics and encodings, but the ids published on `seg_label` / `seg_label_refined` are TRACKED — every
label map goes through a device-side tracker (unseenobjectclustering_amd/tracking.py, one per topic) and the published
value is the track slot in 1..127 that an object keeps from frame to frame and gets back after a short occlusion.
mono8 is enough for it.  The overlays are coloured by the tracked ids as well, so an object keeps its colour.

    python ros/segmentation_tracked.py --network seg_resnet34_8s_embedding --pretrained ckpt.pth \\
           [--pretrained_crop crop.pth] [--cfg <yml>] [--gpu 0] [--rand] --track [--track_min_iou 0.3] [--track_max_age 5]
           [--reid [--reid_min_sim 0.7] [--reid_min_size 0.25] [--reid_max_lost 300]]

With `--reid` on top of `--track` the published value is the IDENTITY entry in 1..127 instead of the track slot
(unseenobjectclustering_amd/identity.py, one Identifier per topic, fed with the frame's colour image and XYZ): an object
keeps it across a jump with no mask overlap and across an occlusion longer than --track_max_age.

Without `--track` this is exactly the node of ros/test_images_segmentation.py.  That file is not changed: the node
takes its segmentation call as an argument, and tracking wraps that call (`tracked_segment`)."""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from unseenobjectclustering_amd.fcn import test_dataset  # noqa: E402
from unseenobjectclustering_amd.fcn.config import cfg, cfg_from_file  # noqa: E402
from unseenobjectclustering_amd import identity  # noqa: E402
from unseenobjectclustering_amd.tracking import Tracker  # noqa: E402

TOPICS = ("seg_label", "seg_label_refined")


def load_base():
    """ros/test_images_segmentation.py as a module (the directory is not a package)."""
    spec = importlib.util.spec_from_file_location("uoc_ros_node", os.path.join(ROOT, "ros", "test_images_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tracked_segment(segment=None, min_iou=0.3, max_age=5, reid=None):
    """Wraps a segmentation call (sample, network, network_crop) -> (out_label, out_label_refined): item 0 of each map —
    the one the node publishes — is renumbered with the track slots of its topic's tracker, or, with reid = the keyword
    arguments of identity.Identifier, with the identity entries of its topic's identifier.  The trackers and identifiers
    are reachable as `.trackers` / `.identifiers` of the returned function."""
    segment = segment or test_dataset.test_sample
    trackers = {name: Tracker(min_iou=min_iou, max_age=max_age) for name in TOPICS}
    identifiers = {name: identity.Identifier(**reid) for name in TOPICS} if reid is not None else {}

    def track(topic, label_maps, sample):
        if label_maps is None:
            return None
        dev = test_dataset._device()
        out = label_maps.clone()
        ids = trackers[topic].update(label_maps[0].to(dev))
        if identifiers:
            xyz = sample["depth"][:1].to(dev) if "depth" in sample else None
            ids = identifiers[topic].update(ids, trackers[topic], identity.image_u8(sample).to(dev), xyz)
        out[0] = ids.to(device=label_maps.device, dtype=label_maps.dtype)
        return out

    def run(sample, network, network_crop):
        out_label, out_label_refined = segment(sample, network, network_crop)
        return track(TOPICS[0], out_label, sample), track(TOPICS[1], out_label_refined, sample)

    run.trackers, run.identifiers = trackers, identifiers
    return run


def make_node(base, network, network_crop, ros, segment=None, track=False, min_iou=0.3, max_age=5, reid=None):
    """base.SegmentationNode, publishing tracked ids when track is set and identities when reid is given as well."""
    if reid is not None and not track:
        raise ValueError("reid needs track (identities are kept per track)")
    if track:
        segment = tracked_segment(segment, min_iou, max_age, reid)
    return base.SegmentationNode(network, network_crop, ros, segment=segment)


def parse_args(base, argv=None):
    """The base node's arguments plus --track, --track_min_iou, --track_max_age and --reid with its three parameters."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--track", dest="track", action="store_true", help="publish tracked ids (stable across frames)")
    p.add_argument("--track_min_iou", dest="track_min_iou", default=0.3, type=float)
    p.add_argument("--track_max_age", dest="track_max_age", default=5, type=int)
    p.add_argument("--reid", dest="reid", action="store_true", help="with --track: publish identities (kept across jumps)")
    p.add_argument("--reid_min_sim", dest="reid_min_sim", default=0.7, type=float)
    p.add_argument("--reid_min_size", dest="reid_min_size", default=0.25, type=float)
    p.add_argument("--reid_max_lost", dest="reid_max_lost", default=300, type=int)
    own, rest = p.parse_known_args(sys.argv[1:] if argv is None else argv)
    if own.reid and not own.track:
        p.error("--reid needs --track (identities are kept per track)")
    args = base.parse_args(rest)
    args.track, args.track_min_iou, args.track_max_age = own.track, own.track_min_iou, own.track_max_age
    args.reid = dict(min_sim=own.reid_min_sim, min_size=own.reid_min_size, max_lost=own.reid_max_lost) if own.reid else None
    return args


def main(argv=None, ros=None):
    base = load_base()
    args = parse_args(base, argv)
    print("Called with args:")
    print(args)
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    if not args.randomize:
        np.random.seed(cfg.RNG_SEED)
    cfg.gpu_id = args.gpu_id
    cfg.device = torch.device("cuda:{:d}".format(cfg.gpu_id))
    cfg.instance_id = args.instance_id
    cfg.MODE = "TEST"
    cfg.TEST.VISUALIZE = False
    network, network_crop = base.build_networks(args)
    node = make_node(base, network, network_crop, ros or base.load_ros(), track=args.track, min_iou=args.track_min_iou,
                     max_age=args.track_max_age, reid=args.reid)
    node.spin()


if __name__ == "__main__":
    main()
