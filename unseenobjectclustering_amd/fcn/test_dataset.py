"""Host-side mirror of the reference's lib/fcn/test_dataset.py inference surface
(clustering_features :44, crop_rois :62, match_label_crop :116, filter_labels_depth :183,
test_sample :232, test_segnet :271), backed by libuoc_hip.so.

Same names, argument meaning and return conventions as the reference (labels are float32
tensors, `out_label` lives on the CPU, ROIs are [K,4] float x0,y0,x1,y1 inclusive, the global
NumPy RNG is consumed once per clustered field in the reference's order).  Internally labels stay
int32 on the device and the per-object Python loops of the reference are single batched launches.
There is no CPU fallback: inputs are moved to the ROCm device and every stage runs as HIP kernels.

The two-stage frame path is written once: _stage1_launches / _stage2_launches queue the device work of the two stages,
FrameGroupJob adds what needs the host (uploads, RNG draws, the read of the ROI counts between the stages).  test_sample,
test_segnet and the frame-parallel runner run that job; fcn/graph_replay.py replays the same two functions as hipGraphs.
"""
from __future__ import annotations

import ctypes
import os
import time

import numpy as np
import torch

from .. import _native
from ..utils.mean_shift import cluster_batch, to_planes
from .config import cfg, require_supported, uses_depth

KAPPA = 20            # test_dataset.py:51
MAX_ITERS = 10        # :56
PAD_FRACTION = 0.25   # :66
DEPTH_FILTER = 0.8    # :252
MAX_LABELS = 128

LAST_FRAME_STATS = {"rois": 0}      # number of stage-1 ROIs of the most recent frame (measurement bookkeeping)


def _device():
    if cfg.device is not None and torch.device(cfg.device).type == "cuda":
        return torch.device(cfg.device)
    if not torch.cuda.is_available():
        raise _native.NativeError("no ROCm device visible: the HIP path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# one scratch buffer per stream: two frames in flight must not share it
_ws = _native.PerStream(lambda dev, _: torch.empty(_native.lib().uoc_roi_workspace_bytes() + 256, dtype=torch.uint8, device=dev)).get


def _pixel_major(features: torch.Tensor) -> torch.Tensor:
    """[B,C,h,w] -> [B,h*w,C] contiguous; zero-copy for the channels-last view SEGNET.forward returns."""
    B, C, h, w = features.shape
    x = features.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    return x.reshape(B, h * w, C)


def _detach_keep_planes(features: torch.Tensor) -> torch.Tensor:
    """features.detach() like the reference (:247), keeping the kernel-layout buffer the 128-d 'cat' output of
    SEGNET.forward carries as `_uoc_planes` (detach() returns a new tensor object without Python attributes)."""
    planes = getattr(features, "_uoc_planes", None)
    features = features.detach()
    if planes is not None:
        features._uoc_planes = planes
    return features


def _kernel_layout(features: torch.Tensor) -> torch.Tensor:
    """[B,C,h,w] features -> the layout of cluster_batch: [B, h*w, 64], or the planes [B, 2, h*w, 64] of 128-d fields."""
    planes = getattr(features, "_uoc_planes", None)     # 128-d output of SEGNET ('cat' fusion): already in kernel layout
    if planes is not None and planes.shape[0] == features.shape[0]:
        return planes
    X = _pixel_major(features.float())
    return to_planes(X) if X.shape[-1] == 128 else X


def _cluster(features: torch.Tensor, firsts, num_seeds: int = 100):
    """Clusters the B fields of `features` [B,C,h,w] from the given first-seed indices (B ints, or an int32 device tensor
    [B]) -> int32 labels [B, h*w], seed indices [B, m], both on the device."""
    return cluster_batch(_kernel_layout(features), firsts, KAPPA, num_seeds, MAX_ITERS, 2 * cfg.TRAIN.EMBEDDING_ALPHA)


def clustering_features(features, num_seeds=100):
    """test_dataset.py:44-59 -> (out_label [B,h,w] float32 on the CPU, list of [m] int64 seed indices)."""
    require_supported()
    if not features.is_cuda:
        raise _native.NativeError("features must be on a ROCm device (no CPU fallback)")
    B, _, h, w = features.shape
    firsts = [np.random.randint(0, h * w) for _ in range(B)]       # mean_shift.py:155, one draw per field, in order
    labels, indices = _cluster(features, firsts, num_seeds)
    out_label = labels.view(B, h, w).float().cpu()
    _check_clustering(labels.device)
    return out_label, [indices[j].long().cpu() for j in range(B)]


def _labels_to_device(labels: torch.Tensor, dev) -> torch.Tensor:
    lab = labels.to(dev)
    if lab.dtype != torch.int32:
        lab = lab.round().to(torch.int32)
    lab = lab.contiguous()
    if lab.numel() and (int(lab.max()) >= MAX_LABELS or int(lab.min()) < 0):
        raise ValueError(f"label ids must be in [0, {MAX_LABELS})")
    return lab


def filter_labels_depth(labels, depth, threshold):
    """test_dataset.py:183-198.  Returns a new tensor like `labels`."""
    dev = depth.device if depth.is_cuda else _device()
    lab = _labels_to_device(labels, dev).clone()
    d = depth.to(dev).float().contiguous()
    B, H, W = lab.shape
    ws = _ws(dev)
    _native.call("uoc_filter_labels_depth", dev, lab, d.data_ptr() + 2 * H * W * 4, 3 * H * W, B, H, W, float(threshold), ws, ws.numel())
    return lab.to(labels.dtype).to(labels.device)


def _read_table(table_dev: torch.Tensor) -> _native.RoiTable:
    host = table_dev.cpu().numpy().tobytes()      # one small D2H (2.5 KB); synchronises the stream
    return _native.RoiTable.from_buffer_copy(host)


def _check_clustering(dev):
    """Raise if a clustering launch since the last check reported a timed-out grid exchange (uoc_ms_check)."""
    _native.call("uoc_ms_check", dev)


def _build_rois(lab0: torch.Tensor, z_plane_ptr, H, W, dev, threshold=DEPTH_FILTER):
    table = torch.empty(_native.ROI_TABLE_BYTES, dtype=torch.uint8, device=dev)
    ws = _ws(dev)
    _native.call("uoc_roi_build", dev, lab0, z_plane_ptr, H, W, float(threshold), PAD_FRACTION, table, ws, ws.numel())
    return table


def _crop_buffers(K, has_depth, dev):
    """(rgb_crops [K,3,S,S], mask_crops [K,S,S], depth_crops [K,3,S,S] or None), uninitialised."""
    S = cfg.TRAIN.SYN_CROP_SIZE
    return (torch.empty((K, 3, S, S), dtype=torch.float32, device=dev), torch.empty((K, S, S), dtype=torch.float32, device=dev),
            torch.empty((K, 3, S, S), dtype=torch.float32, device=dev) if has_depth else None)       # :73-76


def _crop(rgb, depth, lab0, table, K, H, W, dev, out=None):
    """The K ROI crops of one image -> (rgb_crops, mask_crops, depth_crops): new tensors, or the views `out` (same order)
    of a batch that holds the crops of several images."""
    S = cfg.TRAIN.SYN_CROP_SIZE
    rgb_crops, mask_crops, depth_crops = out = out if out is not None else _crop_buffers(K, depth is not None, dev)
    if K > 0:
        _native.call("uoc_roi_crop", dev, rgb, depth, lab0, H, W, table, K, S, rgb_crops, depth_crops, mask_crops)
    return out


def crop_rois(rgb, initial_masks, depth):
    """test_dataset.py:62-112 -> (rgb_crops [K,3,S,S], mask_crops [K,S,S], rois [K,4], depth_crops)."""
    dev = rgb.device if rgb.is_cuda else _device()
    rgb = rgb.to(dev).float().contiguous()
    depth = depth.to(dev).float().contiguous() if depth is not None else None
    N, H, W = initial_masks.shape
    lab0 = _labels_to_device(initial_masks[0], dev)
    table = _build_rois(lab0, ctypes.c_void_p(0), H, W, dev)
    t = _read_table(table)
    K = int(t.K)
    rgb_crops, mask_crops, depth_crops = _crop(rgb, depth, lab0, table, K, H, W, dev)
    rois = torch.tensor([[t.box[k][i] for i in range(4)] for k in range(K)], dtype=torch.float32, device=dev).reshape(K, 4)
    return rgb_crops, mask_crops, rois, depth_crops


def _order_and_map(keep: np.ndarray, sort_key: torch.Tensor):
    """Host part of match_label_crop: ROI paint order by mean depth, far first — or by box area, large
    first, when there is no depth (:129-151, Python's stable sort with reverse=True on the 0-dim
    tensors, NaN behaviour included) and the global renumbering of kept clusters in that order (:156-163)."""
    K = keep.shape[0]
    keys = [(i, sort_key[i]) for i in range(K)]
    order = [i for i, _ in sorted(keys, key=lambda kv: kv[1], reverse=True)]
    mapping = np.zeros((K, MAX_LABELS), dtype=np.int32)
    count = 0
    for i in order:
        for c in np.nonzero(keep[i])[0]:
            count += 1
            mapping[i, c] = count
    return np.asarray(order, dtype=np.int32), mapping


class _HostMirror:
    """Pinned host buffers of one job slot: the ROI tables of a job's frames (the one small device->host read of a frame)
    arrive here as asynchronous copies guarded by an event, so the host can queue another job's work on another stream
    while the read is in flight.  A second event marks that the job's stage 2 has run."""

    def __init__(self, frames=1):
        self.frames = frames
        self.tables = torch.empty((frames, _native.ROI_TABLE_BYTES), dtype=torch.uint8).pin_memory()
        # blocking events: a host thread that waits on one sleeps instead of spinning (the runner's core budget per rank)
        blocking = os.environ.get("UOC_PIPE_BLOCKING_EVENTS", "0") == "1"
        self.table_ready = torch.cuda.Event(blocking=blocking)
        self.stage2_done = torch.cuda.Event(blocking=blocking)


_mirror = _native.PerStream(lambda dev, frames: _HostMirror(frames), size=lambda m: m.frames).get


def _match_stats(labels_crop_i32, mask_crops, depth_crops, K, dev):
    """Overlap / mean-depth statistics of the K clustered crops (:118-148), one launch over all ROIs.
    Returns the device buffer [K*128 keep flags | K mean depths]."""
    S = cfg.TRAIN.SYN_CROP_SIZE
    ws = _ws(dev)
    # keep table and mean depths share one buffer (one D2H), paint order and id map another (one H2D)
    stats = torch.empty((K * MAX_LABELS + K,), dtype=torch.int32, device=dev)
    keep = stats[:K * MAX_LABELS].view(K, MAX_LABELS)
    meanz = stats[K * MAX_LABELS:].view(torch.float32) if depth_crops is not None else None
    _native.call("uoc_roi_match_stats", dev, labels_crop_i32, mask_crops, depth_crops, K, S, keep, meanz, ws, ws.numel())
    return stats


def _paste(labels_crop_i32, table_dev, table_host, stats_h, has_depth, K, H, W, dev):
    """Host ordering of the ROIs (:129-151) from the statistics read back, then one paste launch (:156-177)."""
    S = cfg.TRAIN.SYN_CROP_SIZE
    keep_h = stats_h[:K * MAX_LABELS].view(K, MAX_LABELS).numpy()
    if has_depth:
        sort_key = stats_h[K * MAX_LABELS:K * MAX_LABELS + K].view(torch.float32)
    else:       # :138-146 roi_size = (y_max - y_min + 1) * (x_max - x_min + 1), float32 like the reference's rois
        box = torch.tensor(np.ctypeslib.as_array(table_host.box)[:K].astype(np.float32))
        sort_key = (box[:, 3] - box[:, 1] + 1) * (box[:, 2] - box[:, 0] + 1)
    order, mapping = _order_and_map(keep_h, sort_key)
    flat = np.concatenate([order.reshape(-1), mapping.reshape(-1)]).astype(np.int32)
    plan = torch.from_numpy(flat).to(dev)
    order_d, map_d = plan[:K], plan[K:]
    refined = torch.empty((H * W,), dtype=torch.int32, device=dev)
    _native.call("uoc_roi_paste", dev, labels_crop_i32, table_dev, map_d, order_d, K, S, H, W, refined)
    return refined


# Per-stream sticky device flag of uoc_roi_match (bit 0: NaN sort keys with >= 64 ROIs — the one ordering case the device
# kernel does not restate; the caller then orders on the host).
_order_status = _native.PerStream(lambda dev, _: torch.zeros(1, dtype=torch.int32, device=dev))
_status_word = _order_status.get


def _match_device(labels_crop_i32, mask_crops, depth_crops, table, K, H, W, dev, want_keep=False):
    """match_label_crop (:116-179) with no host round trip (round 6): statistics, ROI paint order (Python's
    sorted(reverse=True) semantics restated on the device), renumbering and paste in one call (uoc_roi_match).
    -> refined int32 [H*W] (device), keep table [K,128] (device) or None."""
    S = cfg.TRAIN.SYN_CROP_SIZE
    ws = _ws(dev)
    refined = torch.empty((H * W,), dtype=torch.int32, device=dev)
    keep = torch.empty((K, MAX_LABELS), dtype=torch.int32, device=dev) if want_keep else None
    status = _status_word(dev)
    _native.call("uoc_roi_match", dev, labels_crop_i32, mask_crops, depth_crops, table, K, S, H, W, refined, keep, None, status, ws,
                 ws.numel())
    return refined, keep


def _take_order_flag(status: torch.Tensor) -> bool:
    """Reads and clears the sticky ordering flag in a stream's status word (synchronises)."""
    flagged = int(status.item()) != 0
    if flagged:
        status.zero_()
    return flagged


def _finish_block(dev):
    """End of a block of frames whose per-frame checks were deferred (the frame-parallel runner): the clustering status
    (uoc_ms_check) and the ordering flag of every stream of `dev`."""
    _check_clustering(dev)
    flags = [_take_order_flag(status) for status in _order_status.of_device(dev)]
    if any(flags):
        raise HostOrderNeeded("a frame had NaN ROI sort keys with >= 64 ROIs: re-run with the ROI ordering on the host")


def _match_host_order(labels_crop_i32, mask_crops, depth_crops, table, K, H, W, dev):
    """The same with the ROI ordering on the host (Python's own sorted on the statistics read back): the fallback for NaN
    keys with >= 64 ROIs, and the path of rounds 1-5."""
    stats = _match_stats(labels_crop_i32, mask_crops, depth_crops, K, dev)
    stats_h = stats.cpu()
    table_host = _read_table(table) if depth_crops is None else None
    refined = _paste(labels_crop_i32, table, table_host, stats_h, depth_crops is not None, K, H, W, dev)
    return refined, stats[:K * MAX_LABELS].view(K, MAX_LABELS)


def _match(labels_crop_i32, mask_crops, depth_crops, table, K, H, W, dev):
    """labels_crop_i32 [K, S*S] int32 (device) -> refined int32 [H*W] (device), keep table (device)."""
    refined, keep = _match_device(labels_crop_i32, mask_crops, depth_crops, table, K, H, W, dev, want_keep=True)
    if _take_order_flag(_status_word(dev)):
        return _match_host_order(labels_crop_i32, mask_crops, depth_crops, table, K, H, W, dev)
    return refined, keep


def match_label_crop(initial_masks, labels_crop, out_label_crop, rois, depth_crop):
    """test_dataset.py:116-179 -> (refined_masks like initial_masks (float), labels_crop with rejected = -1)."""
    dev = labels_crop.device if labels_crop.is_cuda else _device()
    K = labels_crop.shape[0]
    N, H, W = initial_masks.shape
    refined_masks = torch.zeros_like(initial_masks).float()
    if K == 0:
        return refined_masks, labels_crop
    lab = _labels_to_device(labels_crop, dev).reshape(K, -1)
    t = _native.RoiTable()
    t.K = K
    r = rois.detach().cpu().numpy().astype(np.int64)
    for k in range(K):
        for i in range(4):
            t.box[k][i] = int(r[k, i])
    table = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev)
    refined, keep = _match(lab, out_label_crop.to(dev).float().contiguous(),
                           depth_crop.to(dev).float().contiguous() if depth_crop is not None else None,
                           table, K, H, W, dev)
    refined_masks[0] = refined.view(H, W).float().to(refined_masks.device)
    kept = torch.gather(keep, 1, lab.long()) != 0
    labels_out = torch.where(kept, lab, torch.full_like(lab, -1)).view(labels_crop.shape).to(labels_crop.dtype)
    return refined_masks, labels_out.to(labels_crop.device)


def test_sample(sample, network, network_crop):
    """test_dataset.py:232-267: (out_label [B,H,W] float32 CPU, out_label_refined [B,H,W] float32 CPU — only item 0 is
    refined, the rest stays zero, as in the reference — or None)."""
    return _run_frame(sample, network, network_crop, DEPTH_FILTER)


FORCE_HOST_ORDER = os.environ.get("UOC_HOST_ORDER", "0") == "1"      # True: ROI ordering on the host (the fallback for NaN keys with >= 64 ROIs; A/B)


class HostOrderNeeded(_native.NativeError):
    """A frame of the block had NaN sort keys with >= 64 ROIs: the device ordering does not restate that case, the
    caller re-runs with FORCE_HOST_ORDER (runner.run_sharded does)."""


def _upload(samples, dev):
    """The images of `samples` as one batch on the device -> (image [N,3,H,W] float32, XYZ images [N,3,H,W] or None when the
    configuration does not use depth, :236-239).  Raw samples (uint8 BGR + uint16 depth) are prepared on the device
    (io.prepare_on_device); when all are raw and of one size, straight into the batched buffers."""
    from ..io import prepare_on_device
    if all("image_u8" in sm for sm in samples) and len({tuple(sm["depth_u16"].shape) for sm in samples}) == 1:
        Hs, Ws = samples[0]["depth_u16"].shape
        image = torch.empty((len(samples), 3, Hs, Ws), dtype=torch.float32, device=dev)
        xyz = torch.empty((len(samples), 3, Hs, Ws), dtype=torch.float32, device=dev)
        for f, sm in enumerate(samples):
            prepare_on_device(sm, dev, out=(image[f], xyz[f]))
        return image, (xyz if uses_depth() else None)
    # non_blocking is a no-op for pageable host memory (the runtime stages it synchronously) and asynchronous for
    # pinned memory; asking the tensor (`is_pinned()`) costs a driver query per call, so just always pass it
    pin = lambda t: t.to(dev, non_blocking=True)
    images, depths = [], []
    for sm in samples:
        if "image_u8" in sm:
            sm = dict(sm, **prepare_on_device(sm, dev))
        images.append(pin(sm["image_color"]).float())
        if uses_depth():
            depths.append(pin(sm["depth"]).float())
    batch = lambda ts: (torch.cat(ts) if len(ts) > 1 else ts[0]).contiguous()
    return batch(images), (batch(depths) if depths else None)


def _stage1_launches(network, image, depth, firsts, thr, label=None, refine=None):
    """Stage 1 of the N images of `image`, queued on the current stream: embed (:247), cluster from the first-seed indices
    `firsts`, depth filter (:250-252; thr None = none) — fused with the ROI table build for the first `refine` items
    (default: all), one filter-only call for the rest.  -> labels [N, H*W] int32, the ROI tables of the refined items."""
    dev = _device()
    N, _, H, W = image.shape
    R = N if refine is None else refine
    features = _detach_keep_planes(network(image, label, depth))
    labels, _ = _cluster(features, firsts)
    zptr = lambda f: ctypes.c_void_p(depth.data_ptr() + ((3 * f + 2) * H * W) * 4 if thr is not None else 0)   # z plane of item f
    tables = [_build_rois(labels[f], zptr(f), H, W, dev, thr if thr is not None else 0.0) for f in range(R)]
    if R < N and thr is not None:
        ws = _ws(dev)
        _native.call("uoc_filter_labels_depth", dev, labels[R:], zptr(R), 3 * H * W, N - R, H, W, float(thr), ws, ws.numel())
    return labels, tables


def _match_frames(parts, tables, Ks, H, W, dev, host_order=False):
    """match_label_crop of every frame with ROIs, from the clustered crop batch `parts` = (labels_crop, mask, depth_crop):
    -> per frame the refined map [H, W] int32, or None.  host_order: _match_host_order (synchronises) for _match_device."""
    match = _match_host_order if host_order else _match_device
    off = np.concatenate([[0], np.cumsum(Ks)]).astype(int)
    refined = [None] * len(Ks)
    for f, K in enumerate(Ks):
        if K > 0:
            labels_crop, mask, dep = (p[off[f]:off[f + 1]] if p is not None else None for p in parts)
            refined[f] = match(labels_crop, mask, dep, tables[f], K, H, W, dev)[0].view(H, W)
    return refined


def _stage2_launches(network_crop, image, depth, labels, tables, Ks, firsts, host_order=False):
    """Stage 2 of the frames whose ROI tables are `tables` (Ks: their ROI counts, not all 0), queued on the current stream:
    the crops of all frames as ONE batch of sum(Ks) through one network_crop forward (:259) and one clustering launch set
    (firsts: sum(Ks) first-seed indices), then match_label_crop per frame.
    -> per frame the refined map [H, W] int32 or None, and the crop batch (labels_crop, mask, depth_crop) that a redo of
    the match with the ROI ordering on the host starts from."""
    dev = _device()
    _, _, H, W = image.shape
    rgb, mask, dep = _crop_buffers(sum(Ks), depth is not None, dev)
    a = 0
    for f, K in enumerate(Ks):
        _crop(image[f], depth[f] if depth is not None else None, labels[f], tables[f], K, H, W, dev,
              out=(rgb[a:a + K], mask[a:a + K], dep[a:a + K] if dep is not None else None))
        a += K
    features_crop = _detach_keep_planes(network_crop(rgb, mask, dep))
    parts = (_cluster(features_crop, firsts)[0], mask, dep)
    return _match_frames(parts, tables, Ks, H, W, dev, host_order), parts


class FrameGroupJob:
    """Frames on their way through the two-stage path as ONE set of launches per stage, cut at the ONE point where the host
    needs a small result from the device (the ROI counts, which size the stage-2 launches):

        stage1  upload, embed, cluster, depth filter + ROI tables              -> async D2H of the tables
        stage2  (needs K) crop, embed + cluster the crops, match: statistics, ROI order + renumbering + paste (device)

    The launches themselves are _stage1_launches / _stage2_launches (fcn/graph_replay.py replays the same two functions);
    the job owns what they do not: uploads, RNG draws, the table read and its event, the results.

    `samples` is either N single-image samples, each with its own RNG (`rngs`) — the frame-parallel runner's unit of work:
    all stage-1 embeddings in one network forward (batch N), all clusterings in one launch set, and the crops of all N
    frames in one stage-2 forward (batch K_1 + ... + K_N).  Twice the pixels / Winograd tiles per launch is what the
    convolution kernels need to fill 256 CUs with full-height tiles.  Every frame keeps its own ROI table, RNG
    and output; label maps are bit-identical to one-frame-at-a-time processing (the kernels' per-output summation order
    does not depend on the batch), and do not depend on how jobs in flight interleave.
    Or it is ONE sample (`_run_frame`), possibly a batch of B images that share one RNG (rngs=None: the global NumPy RNG,
    like the reference): every item is clustered and depth-filtered, only item 0 is refined (:247-261).

    Round 6: the second cut of rounds 1-5 (statistics to the host, Python's sorted, plan back to the device) is gone —
    uoc_roi_match orders on the device.  With host_order=True (FORCE_HOST_ORDER) stage 2 orders on the host, synchronously
    (_match_host_order): a correctness fallback, not a schedule."""

    def __init__(self, samples, network, network_crop, depth_threshold, rngs=None, host_order=None):
        self.samples, self.network, self.network_crop = list(samples), network, network_crop
        self.depth_threshold = depth_threshold
        self.rngs = list(rngs) if rngs is not None else [np.random]
        self.host_order = FORCE_HOST_ORDER if host_order is None else host_order
        self.R = len(self.samples)               # refined items: every single-image frame, or item 0 of the one sample
        self.K = [0] * self.R
        self.refined = [None] * self.R

    def stage1(self):
        require_supported()
        dev = self.dev = _device()
        self.image, self.depth = image, depth = _upload(self.samples, dev)
        N, _, H, W = image.shape
        self.N, self.H, self.W = N, H, W
        assert N == self.R or self.R == 1, "several samples in one FrameGroupJob must be single-image samples"
        if len(self.rngs) == 1:
            self.rngs = self.rngs * N            # the items of one sample draw from one RNG, in item order
        thr = self.depth_threshold if depth is not None else None                                 # :250 `if depth is not None`
        label = self.samples[0]["label"].to(dev) if self.R == 1 and "label" in self.samples[0] else None
        firsts = [self.rngs[f].randint(0, H * W) for f in range(N)]          # mean_shift.py:155, one draw per field
        self.labels, self.tables = _stage1_launches(self.network, image, depth, firsts, thr, label, refine=self.R)
        if self.network_crop is not None:
            self.host = _mirror(dev, self.R)
            for f in range(self.R):
                self.host.tables[f].copy_(self.tables[f], non_blocking=True)
            self.host.table_ready.record(torch.cuda.current_stream(dev))

    def stage2(self):
        if self.network_crop is None:
            return
        S = cfg.TRAIN.SYN_CROP_SIZE
        self.host.table_ready.synchronize()
        self.K = [int(_native.RoiTable.from_buffer_copy(self.host.tables[f].numpy().tobytes()).K) for f in range(self.R)]
        if sum(self.K) == 0:
            return
        firsts = [self.rngs[f].randint(0, S * S) for f in range(self.R) for _ in range(self.K[f])]   # K_f draws per frame, in order
        self.refined, self.parts = _stage2_launches(self.network_crop, self.image, self.depth, self.labels, self.tables,
                                                    self.K, firsts, self.host_order)
        self.host.stage2_done.record(torch.cuda.current_stream(self.dev))      # the runner frees the slot only then (pending_event)

    def redo_with_host_order(self):
        """The device ordering flagged a frame (NaN keys, >= 64 ROIs): order on the host from the same crop labels."""
        self.refined = _match_frames(self.parts, self.tables, self.K, self.H, self.W, self.dev, host_order=True)

    def pending_event(self, state):
        """The event the next step waits for (state 1: the ROI tables have landed on the host; state 2: stage 2 has run),
        or None if there is nothing to wait for.
        State 2 is a wait although the device ordering needs nothing from the device any more: a stream that is handed its
        next job's stage 1 while this job's stage 2 is still queued puts that job's sampling kernel into the per-device event
        chain (csrc/meanshift.hip) AHEAD of the other streams' stage-2 sampling kernels, which then wait behind this
        stream's whole stage 2 — measured 168 -> 161 frames/s (same box, round 6)."""
        if self.network_crop is None:
            return None
        if state == 1:
            return self.host.table_ready
        return self.host.stage2_done if sum(self.K) > 0 else None

    def final_maps(self):
        """Per frame: the refined map if stage 2 produced one, else the stage-1 map ([H,W] int32, device)."""
        return [self.refined[f] if self.refined[f] is not None else self.labels[f].view(self.H, self.W) for f in range(self.R)]

    def result_device(self):
        """Of the job of one sample: (labels [B,H,W] int32, refined [B,H,W] int32 or None), on the device."""
        refined = self.refined[0]
        if refined is not None:      # match_label_crop returns zeros_like(initial_masks) with only item 0 painted (:153,:176-177)
            refined = refined.view(1, self.H, self.W)
            if self.N > 1:
                full = torch.zeros((self.N, self.H, self.W), dtype=refined.dtype, device=self.dev)
                full[0] = refined[0]
                refined = full
        return self.labels.view(self.N, self.H, self.W), refined


def _run_frame_graphed(sample, network, network_crop, depth_threshold, checked):
    """The frame as hipGraph replays (fcn/graph_replay.py) when the call qualifies — cfg.TEST.GRAPH_REPLAY, a single-image
    sample, SEGNET networks, and not the first call of this (networks, size, configuration) combination — else None and
    the caller runs the eager FrameGroupJob.  Same label maps either way (tests/test_graph_replay_gpu.py)."""
    from . import graph_replay as GR        # (it imports this module)
    if FORCE_HOST_ORDER or not getattr(cfg.TEST, "GRAPH_REPLAY", False) or "label" in sample:
        return None
    from ..networks.SEG import SEGNET
    if not isinstance(network, SEGNET) or not (network_crop is None or isinstance(network_crop, SEGNET)):
        return None
    if "image_u8" not in sample and (sample["image_color"].dim() != 4 or sample["image_color"].shape[0] != 1):
        return None
    require_supported()
    dev = _device()
    image, depth = _upload([sample], dev)
    _, _, H, W = image.shape
    gf = GR.frame_for(network, network_crop, H, W, dev, depth_threshold if depth is not None else None)
    if gf is None:
        return None
    labels, refined, K, redo = gf.run(image, depth, None)
    LAST_FRAME_STATS["rois"] = K
    if checked:
        _check_clustering(dev)              # synchronises
        if K > 0 and _take_order_flag(gf.status):
            refined = redo()
    return labels, refined


def _run_frame(sample, network, network_crop, depth_threshold, return_device=False, checked=None):
    """Per-frame body shared by test_sample (:247-261) and test_segnet (:288-321).
    depth_threshold None = no depth-coverage filter.  return_device=True keeps the int32 label
    maps on the device ([B,H,W], [1,H,W] or None).  checked (default: not return_device): synchronise and check the
    clustering status + the ordering flag before returning; the frame-parallel runner passes False and checks once per
    block (_finish_block)."""
    if checked is None:
        checked = not return_device
    graphed = _run_frame_graphed(sample, network, network_crop, depth_threshold, checked)
    if graphed is not None:
        labels, out_label_refined = graphed
    else:
        job = FrameGroupJob([sample], network, network_crop, depth_threshold)
        job.stage1()
        job.stage2()
        LAST_FRAME_STATS["rois"] = job.K[0]
        if checked:
            _check_clustering(job.dev)          # synchronises
            if job.K[0] > 0 and not job.host_order and _take_order_flag(_status_word(job.dev)):
                job.redo_with_host_order()
        labels, out_label_refined = job.result_device()
    if return_device:
        return labels, out_label_refined
    out_label = labels.float().cpu()
    if out_label_refined is not None:
        out_label_refined = out_label_refined.float().cpu()
    return out_label, out_label_refined


def _print_average(metrics_all):
    """test_dataset.py:346-357 — sum per key over the frames, divide by the frame count, print sorted."""
    result = {}
    num = len(metrics_all)
    for metrics in metrics_all:
        for k in metrics.keys():
            result[k] = result.get(k, 0) + metrics[k]
    for k in sorted(result.keys()):
        result[k] /= num
        print("%s: %f" % (k, result[k]))
    return result


def test_segnet(test_loader, network, output_dir, network_crop):
    """test_dataset.py:271-381: dataset loop around the same per-frame body; per-frame segmentation metrics of
    the stage-1 and the refined label maps against sample['label'] (multilabel_metrics, :308-329), one .mat
    per sample (labels, labels_refined, filename; :337-340) and the averaged report (:346-381).  Samples
    without a 'label' entry are segmented and saved but not scored."""
    import scipy.io
    from ..utils.evaluation import multilabel_metrics
    network.eval()
    if network_crop is not None:
        network_crop.eval()
    epoch_size = len(test_loader)
    results = []
    metrics_all, metrics_all_refined = [], []
    name = str(getattr(getattr(test_loader, "dataset", None), "name", ""))
    threshold = 0.5 if "ocid" in name else (0.8 if "osd" in name else None)      # :299-305
    for i, sample in enumerate(test_loader):
        end = time.time()
        labels_dev, refined_dev = _run_frame(sample, network, network_crop, threshold, return_device=True, checked=True)
        prediction_dev = labels_dev.reshape(labels_dev.shape[-2:]) if labels_dev.shape[0] == 1 else labels_dev[0]
        refined_2d = refined_dev[0] if refined_dev is not None else prediction_dev
        prediction = labels_dev.float().cpu().squeeze().numpy()
        prediction_refined = refined_dev.float().cpu().squeeze().numpy() if refined_dev is not None else prediction.copy()
        result = {"labels": prediction, "labels_refined": prediction_refined, "filename": sample.get("filename", "")}
        if "label" in sample:
            gt = sample["label"].squeeze()
            metrics = multilabel_metrics(prediction_dev, gt)                     # :308-312
            metrics_all.append(metrics)
            print(metrics)
            metrics_refined = multilabel_metrics(refined_2d, gt)                 # :324-329
            metrics_all_refined.append(metrics_refined)
            print(metrics_refined)
            result["metrics"], result["metrics_refined"] = metrics, metrics_refined
        if output_dir is not None:
            filename = os.path.join(output_dir, "%06d.mat" % i)
            print(filename)
            scipy.io.savemat(filename, {k: result[k] for k in ("labels", "labels_refined", "filename")},
                             do_compression=True)
        results.append(result)
        print("[%d/%d], batch time %.2f" % (i, epoch_size, time.time() - end))
    if metrics_all:
        print("========================================================")
        print("%d images" % len(metrics_all))
        print("========================================================")
        result = _print_average(metrics_all)
        for k in ("Objects Precision", "Objects Recall", "Objects F-measure", "Boundary Precision", "Boundary Recall",
                  "Boundary F-measure", "obj_detected_075_percentage"):
            print("%.6f" % (result[k]))
        print("========================================================")
        print(result)
        print("====================Refined=============================")
        print(_print_average(metrics_all_refined))
        print("========================================================")
    return results
