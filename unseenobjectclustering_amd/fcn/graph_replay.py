"""One frame at a time as hipGraph replays (round 6; no reference counterpart — the reference runs test_sample eagerly,
lib/fcn/test_dataset.py:232-267, and its ROS consumer calls it once per camera frame,
ros/test_images_segmentation.py:134-161).

A frame is TWO graph launches with ONE small device->host read between them:

    graph 1   (fixed shape)   network(image, depth) -> mean shift -> depth filter + ROI table -> D2H of the table
    host      waits for the table, reads K (the number of ROIs sizes every stage-2 launch), draws the K first-seed
              indices from the caller's RNG (mean_shift.py:155: 1 + K draws per frame, in the reference's order)
    graph 2[K] crop K ROIs -> network_crop -> K mean shifts -> match statistics, ROI order, renumbering, paste (device)

What is replayed is exactly the eager path's launch sequence (test_dataset._stage1_launches / _stage2_launches, the two
functions FrameGroupJob calls, run under stream capture on static buffers), so the label maps are bit-identical to the eager
job's (tests/test_graph_replay_gpu.py: torch.equal).  Graph 2 is captured
lazily per K; the first frame with a new K runs eagerly (that run is also the warm-up that sizes the workspaces and lets
the convolution tuner look its shapes up) and captures for the next time.

Why K stays a host read instead of living on the device: the ROI count sizes the stage-2 network launches
(batch K through ~150 convolution launches whose tile shapes and persistent item lists are derived from it).  A
device-resident K would need every convolution kernel to take its batch from memory; with the read in place the idle
time per frame is one event wait (~20 us) and the Python in front of a frame is two replay calls.

Constraints (checked by test_dataset._run_frame_graphed): single-image samples, SEGNET networks (a stub callable may do anything inside its
forward), one stream per device at a time — the persistent sampling kernel is launched plainly under capture (no
cooperative launch, no cross-stream event chain), so replays must not overlap other work on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from . import test_dataset as TD
from .config import cfg, uses_depth

MAX_ROIS = 127


class GraphedFrame:
    """The two graphs (graph 2 per ROI count) of one (networks, image size, configuration) combination, with the static
    buffers they read and write and the dedicated stream they are captured and replayed on."""

    def __init__(self, network, network_crop, H, W, dev, depth_threshold):
        self.network, self.network_crop = network, network_crop
        self.H, self.W, self.dev, self.thr = H, W, dev, depth_threshold
        self.S = int(cfg.TRAIN.SYN_CROP_SIZE)
        self.has_depth = uses_depth()
        self.stream = torch.cuda.Stream(dev)
        self.ready = torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            self.image = torch.zeros((1, 3, H, W), dtype=torch.float32, device=dev)
            self.depth = torch.zeros((1, 3, H, W), dtype=torch.float32, device=dev) if self.has_depth else None
            self.first1 = torch.zeros(1, dtype=torch.int32, device=dev)
            self.first2 = torch.zeros(MAX_ROIS + 1, dtype=torch.int32, device=dev)
        self.first1_h = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.first2_h = torch.zeros(MAX_ROIS + 1, dtype=torch.int32).pin_memory()
        self.table_h = torch.zeros(_native.ROI_TABLE_BYTES, dtype=torch.uint8).pin_memory()
        self._table_K = self.table_h.numpy()[:4].view(np.int32)        # uoc_roi_table.K
        self.g1 = None
        self.g2 = {}
        self.calls = 0
        with torch.cuda.stream(self.stream):
            self.status = TD._status_word(dev)      # the ordering flag of THIS stream (uoc_roi_match)

    # -- the two stage bodies: the eager path's own launch functions, on the static buffers ------------------------------
    def _body1(self):
        labels, (table,) = TD._stage1_launches(self.network, self.image, self.depth, self.first1,
                                               self.thr if self.depth is not None else None)
        if self.network_crop is not None:
            self.table_h.copy_(table, non_blocking=True)
        return labels, table

    def _body2(self, K):
        (refined,), parts = TD._stage2_launches(self.network_crop, self.image, self.depth, self.labels, [self.table], [K],
                                                self.first2[:K])
        return refined, parts

    def _capture(self, body):
        # (capture_begin / capture_end directly: the torch.cuda.graph context manager also runs gc.collect() and
        # empty_cache(), which would hand the caching allocator's blocks back in the middle of a frame sequence)
        g = torch.cuda.CUDAGraph()
        _native.GRAPHS_ALIVE += 1
        torch.cuda.synchronize(self.dev)
        assert torch.cuda.current_stream(self.dev) == self.stream
        g.capture_begin(capture_error_mode="thread_local")
        try:
            out = body()
        finally:
            g.capture_end()
        return g, out

    # -- one frame --------------------------------------------------------------------------------------------------
    def run(self, image, depth, rng):
        """image / depth: [1,3,H,W] float32 on the device (any stream).  -> (labels [1,H,W] int32, refined [1,H,W] int32
        or None, K, redo) — new tensors, the static buffers are reused by the next frame.  `redo` re-runs the ROI
        ordering on the host from this frame's crop labels (only valid until the next run)."""
        H, W, dev, S = self.H, self.W, self.dev, self.S
        draw = (rng if rng is not None else np.random).randint
        caller = torch.cuda.current_stream(dev)
        self.stream.wait_stream(caller)
        self.calls += 1
        with torch.cuda.stream(self.stream):
            self.image.copy_(image, non_blocking=True)
            if self.depth is not None:
                self.depth.copy_(depth, non_blocking=True)
            self.first1_h[0] = int(draw(0, H * W))                               # mean_shift.py:155
            self.first1.copy_(self.first1_h, non_blocking=True)
            if self.g1 is None:
                self._body1()                                                    # warm-up: workspaces, tuner lookups, attributes
                self.g1, (self.labels, self.table) = self._capture(self._body1)
            self.g1.replay()
            refined, redo, K = None, None, 0
            if self.network_crop is not None:
                self.ready.record(self.stream)
                self.ready.synchronize()                                         # the ONE host wait inside a frame
                K = int(self._table_K[0])
            if K > 0:
                for k in range(K):
                    self.first2_h[k] = int(draw(0, S * S))                       # K draws, in ROI order
                self.first2.copy_(self.first2_h, non_blocking=True)
                entry = self.g2.get(K)
                if entry is None:
                    # first frame with this K: run eagerly (= the warm-up), use that result, capture for the next time
                    refined, parts = self._body2(K)
                    g, (ref_static, parts_static) = self._capture(lambda: self._body2(K))
                    self.g2[K] = (g, ref_static, parts_static)
                else:
                    g, ref_static, parts = entry
                    g.replay()
                    refined = ref_static.clone()
                refined = refined.view(1, H, W)

                def redo(parts=parts, K=K):
                    with torch.cuda.stream(self.stream):
                        r, _ = TD._match_host_order(parts[0], parts[1], parts[2], self.table, K, H, W, dev)
                    torch.cuda.current_stream(dev).wait_stream(self.stream)
                    return r.view(1, H, W)
            labels = self.labels.clone().view(1, H, W)
        caller.wait_stream(self.stream)
        return labels, refined, K, redo


_frames = {}


def _key(network, network_crop, H, W, dev, thr):
    gen = lambda n: (id(n), getattr(n, "_native_gen", 0)) if n is not None else None
    return (gen(network), gen(network_crop), H, W, dev.type, dev.index, thr, cfg.INPUT, cfg.TRAIN.FUSION_TYPE,
            int(cfg.TRAIN.SYN_CROP_SIZE), float(cfg.TRAIN.EMBEDDING_ALPHA), str(cfg.TRAIN.EMBEDDING_METRIC))


def frame_for(network, network_crop, H, W, dev, thr):
    """The GraphedFrame of this combination; None on the FIRST call of a combination (that call runs eagerly — a one-shot
    caller never pays for a capture, and the eager frame builds the native weight copies the key's generation counts)."""
    for n in (network, network_crop):
        if n is not None:
            n._ensure_native(dev)
    key = _key(network, network_crop, H, W, dev, thr)
    gf = _frames.get(key)
    if gf is None:
        _frames[key] = False               # seen once
        return None
    if gf is False:
        if len([v for v in _frames.values() if v]) >= 8:      # a bounded cache: drop the oldest combination
            for k, v in list(_frames.items()):
                if v:
                    del _frames[k]
                    break
        gf = _frames[key] = GraphedFrame(network, network_crop, H, W, dev, thr)
    return gf


def reset():
    """Drops every captured graph (tests; after changing library state that graphs bake)."""
    _frames.clear()
