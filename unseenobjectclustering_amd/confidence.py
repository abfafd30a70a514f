"""How sure is a label: assignment margins per pixel and per object, on the device (uoc_ms_confidence, uoc_conf_paste,
uoc_conf_objects, include/uoc_hip.h).

    labels, margin, second, Z, seed_labels = cluster_with_confidence(X, firsts, 20.0, 100, 10, 0.04)
    res = assign_confidence(X, Z, seed_labels)                   # the same from given seeds: res.margin, res.second, res.rival
    out, refined, conf = segment_confidence(sample, net, net_crop)
    conf.margin                                                  # [H,W] float32: 0 = a coin toss, 1 = no other label in sight
    conf.per_object.mean[3], conf.per_object.weak_share[3]       # object 3: mean margin, share of its pixels below `weak`
    summarize(labels, anything, weak=0.02)                       # the per-id summary of any (label map, value map) pair

The nearest-seed assignment picks per pixel the seed of smallest cosine distance; the margin is how far the nearest seed
of ANOTHER seed component lies behind it, `second` the label the pixel would carry then.  The per-id summary is integer
arithmetic on q = floor(margin * 65536): defined exactly, independent of launch order and batch.  Cosine metric only.
No CPU fallback."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native

NUM_IDS = 128
ONE = _native.CONF_ONE
STAT_FIELDS = ("pixels", "sum_q", "min_q", "weak")


class AssignConfidence(_native.Fields):
    """Device tensors of one uoc_ms_confidence call over B fields of n pixels: labels [B,n] int32 (what the clustering's
    assignment writes, bit for bit), margin [B,n] float32, second [B,n] int32 (-1: every seed carries the pixel's label),
    closest and rival [B,n] int32 (seed indices; rival -1 likewise)."""


class ConfidenceSummary(_native.Fields):
    """Per id 0..127 of every frame (row 0: the background), host numpy arrays [B,128]: pixels, min (the smallest q /
    65536), weak (pixels with q < weak_q), mean = sum_q / pixels / 65536 and weak_share = weak / pixels as float64 (NaN
    for an id without pixels); stats: the raw table [B,128,4] int64 (STAT_FIELDS) on the device; weak_q: the threshold."""


class FrameConfidence(_native.Fields):
    """segment_confidence's third item.  margin1 [B,H,W] float32 and second1 [B,H,W] int32: stage 1 (second1 in the
    numbering of the clustering, before the depth filter); margin [H,W] float32: the final map of item 0; per_object: the
    ConfidenceSummary of (final label map, margin); rois: the number of stage-1 ROIs; stage2: None without ROIs, else what
    the final map was pasted from: margin_crop [K,S*S] float32, labels_crop [K,S*S] int32, table (the uoc_roi_table bytes),
    plan [K + K*128] int32 and labels1 [H*W] int32, the filtered stage-1 map of item 0.  Device tensors but for
    per_object's host arrays."""


def _device_f32(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _native.NativeError(f"confidence: {what} must be a tensor on the GPU (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"confidence: {what} must be float32, got {t.dtype}")
    return t.contiguous()


def weak_to_q(weak: float) -> int:
    """The threshold `weak` on a margin as the integer the device compares q = floor(margin * 65536) with."""
    if not 0.0 <= float(weak) <= 1.0:
        raise ValueError(f"weak = {weak} outside [0, 1]")
    return min(ONE - 1, int(np.ceil(float(weak) * ONE)))


def assign_confidence(X, Z, seed_labels, num_unique=None) -> AssignConfidence:
    """X [B,n,64] float32 unit rows (or the planes [B,2,n,64] of 128-d fields), Z [B,m,64] ([B,2,m,64]) and seed_labels
    [B,m] int32 as cluster_batch(return_parts=True) returns them; num_unique [B] int32 defaults to the number of distinct
    seed labels of every field, counted on the device.  No copy to the host, nothing synchronises."""
    X, Z = _device_f32(X, "X"), _device_f32(Z, "Z")
    if X.dim() not in (3, 4) or Z.dim() != X.dim() or X.shape[-1] != 64 or Z.shape[-1] != 64 or Z.shape[:-2] != X.shape[:-2] \
            or Z.device != X.device:
        raise _native.NativeError(f"confidence: X {tuple(X.shape)} and Z {tuple(Z.shape)} are not [B,n,64] and [B,m,64] (or "
                                  "[B,2,n,64] and [B,2,m,64]) on one device")
    halves = 1 if X.dim() == 3 else int(X.shape[1])
    B, n, m = int(X.shape[0]), int(X.shape[-2]), int(Z.shape[-2])
    dev = X.device
    if not isinstance(seed_labels, torch.Tensor) or seed_labels.device != dev or tuple(seed_labels.shape) != (B, m):
        raise _native.NativeError(f"confidence: seed_labels must be a [{B},{m}] tensor on {dev}")
    sl = seed_labels.to(torch.int32).contiguous()
    if num_unique is None:
        ordered = torch.sort(sl, dim=1).values
        nu = (1 + (ordered[:, 1:] != ordered[:, :-1]).sum(dim=1)).to(torch.int32)
    else:
        nu = torch.as_tensor(num_unique, dtype=torch.int32, device=dev).reshape(B).contiguous()
    L = _native.lib()
    labels, second, closest, rival = (torch.empty((B, n), dtype=torch.int32, device=dev) for _ in range(4))
    margin = torch.empty((B, n), dtype=torch.float32, device=dev)
    nws = L.uoc_ms_confidence_workspace_bytes(B, n, m, halves)
    ws = _native.workspace("uoc_ms_confidence_workspace_bytes", dev, B, n, m, halves, who="confidence", hint=f"B={B} n={n} m={m}", floor=16)
    _native.call("uoc_ms_confidence", dev, X, halves, B, n, Z, sl, nu, m, _native.METRIC_COSINE, labels, margin, second, closest,
                 rival, ws, nws)
    return AssignConfidence(labels=labels, margin=margin, second=second, closest=closest, rival=rival)


def cluster_with_confidence(X, first_index, kappa=20.0, num_seeds=100, max_iters=10, epsilon=None):
    """cluster_batch(..., return_parts=True, metric='cosine') followed by assign_confidence on its seeds ->
    (labels [B,n] int32, margin [B,n] float32, second [B,n] int32, Z, seed_labels).  `labels` are the confidence call's:
    equal to cluster_batch's bit for bit."""
    from .utils.mean_shift import cluster_batch
    _, _, Z, seed_labels = cluster_batch(X, first_index, kappa, num_seeds, max_iters, epsilon, return_parts=True, metric="cosine")
    res = assign_confidence(X, Z, seed_labels)
    return res.labels, res.margin, res.second, Z, seed_labels


def object_stats(labels, conf, weak_q: int):
    """The raw uoc_conf_objects call: labels [B,H,W] int32 and conf [B,H,W] float32 contiguous on one GPU -> the table
    [B,128,4] int64 on the device.  No synchronisation."""
    B, H, W = labels.shape
    dev = labels.device
    stats = torch.empty((B, NUM_IDS, 4), dtype=torch.int64, device=dev)
    _native.call("uoc_conf_objects", dev, labels, conf, B, H, W, int(weak_q), stats)
    return stats


def summarize(labels, conf, weak=0.02) -> ConfidenceSummary:
    """The per-id summary of a (label map, value map) pair: labels [B,H,W] or [H,W] of int32 / int64 / float ids (the maps
    test_sample returns are float32), conf of the same shape, float32.  A pixel counts as weak when its q =
    floor(conf * 65536) is below ceil(weak * 65536).  One small read of the table (synchronises)."""
    lab = _native.label_input("summarize", labels)
    if not _native.on_gpu(conf):
        raise _native.NativeError("summarize: conf must be a tensor on the GPU (there is no CPU fallback)")
    if lab.dim() == 2:
        lab, conf = lab[None], conf[None] if conf.dim() == 2 else conf
    if lab.dim() != 3 or tuple(conf.shape) != tuple(lab.shape) or conf.device != lab.device:
        raise _native.NativeError(f"summarize: labels {tuple(lab.shape)} and conf {tuple(conf.shape)} do not match ([B,H,W])")
    weak_q = weak_to_q(weak)
    stats = object_stats(lab, conf.to(torch.float32).contiguous(), weak_q)
    h = stats.cpu().numpy()
    pixels = h[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = h[..., 1].astype(np.float64) / pixels / ONE
        share = h[..., 3].astype(np.float64) / pixels
    return ConfidenceSummary(pixels=pixels.copy(), mean=mean, min=h[..., 2].astype(np.float64) / ONE, weak=h[..., 3].copy(),
                             weak_share=share, stats=stats, weak_q=weak_q)


def paste_values(values_crop, labels_crop, table, plan, K, H, W, out):
    """The raw uoc_conf_paste call: the crop-level values [K,S*S] float32 into `out` [H*W] float32 (pre-filled by the
    caller) along the paint plan [K + K*128] int32 of uoc_roi_match.  No synchronisation."""
    S = int(round(values_crop.shape[-1] ** 0.5)) if values_crop.dim() == 2 else int(values_crop.shape[-1])
    dev = out.device
    _native.call("uoc_conf_paste", dev, values_crop, labels_crop, table, plan, int(K), S, int(H), int(W), out)
    return out


def final_margin(refined, labels1, margin1, margin_crop, labels_crop, table, plan, K, H, W):
    """The margin of the final map of one frame (device tensors; refined, labels1 [H*W] int32 — labels1 the FILTERED
    stage-1 map — margin1 [H*W] float32, margin_crop [K,S*S] float32): a pixel with refined != 0 carries the margin of the
    crop pixel that painted it; one with refined == 0 and stage-1 label 0 keeps its stage-1 margin; one with refined ==
    0 and a stage-1 label != 0 gets 0.0, the two stages disagree."""
    out = torch.where(labels1 == 0, margin1, torch.zeros_like(margin1)).contiguous()
    return paste_values(margin_crop, labels_crop, table, plan, K, H, W, out)


def segment_confidence(sample, network, network_crop, return_device=False, weak=0.02):
    """One frame through the two-stage path (fcn/test_dataset.py's helpers, the draws of the global NumPy RNG in
    FrameGroupJob's order: one randint(0, H*W) per item, then K draws of randint(0, S*S)) with the margins alongside ->
    (out_label, out_label_refined, conf): the two maps exactly as test_sample returns them under the same np.random.seed
    (float32, host; with return_device int32 on the device, [B,H,W] and [1,H,W] or None), conf a FrameConfidence.
    The margin of the final map follows final_margin; with no ROI, or network_crop None, margin = margin1[0] and per_object
    is taken over the stage-1 map.  When the device ordering of the ROIs flags NaN sort keys with >= 64 ROIs this raises
    HostOrderNeeded: that case is not covered (test_sample orders on the host then).
    Cosine metric only: with cfg.TRAIN.EMBEDDING_METRIC = 'euclidean' test_sample clusters with the euclidean metric, for
    which no margin is built, so this raises NotImplementedError before anything is drawn from the RNG rather than
    segment the frame with another metric.
    Host traffic: the ROI-count read between the stages, the clustering status and the ordering flag at the end, and the
    summary's small table; each of them synchronises."""
    from .fcn import test_dataset as TD
    from .fcn.config import cfg, require_supported
    from .utils.mean_shift import cluster_batch
    require_supported()
    if cfg.TRAIN.EMBEDDING_METRIC != "cosine":
        raise NotImplementedError("segment_confidence: cfg.TRAIN.EMBEDDING_METRIC = %r; the assignment margin is built for the "
                                  "cosine metric only, and the frame is not re-segmented with another metric"
                                  % (cfg.TRAIN.EMBEDDING_METRIC,))
    dev = TD._device()
    image, depth = TD._upload([sample], dev)
    N, _, H, W = image.shape
    thr = TD.DEPTH_FILTER if depth is not None else None
    label = sample["label"].to(dev) if "label" in sample else None
    firsts = [np.random.randint(0, H * W) for _ in range(N)]
    eps = 2 * cfg.TRAIN.EMBEDDING_ALPHA
    X = TD._kernel_layout(TD._detach_keep_planes(network(image, label, depth)))
    labels, _, Z, seed_labels = cluster_batch(X, firsts, TD.KAPPA, 100, TD.MAX_ITERS, eps, return_parts=True, metric="cosine")
    res1 = assign_confidence(X, Z, seed_labels)
    margin1, second1 = res1.margin.view(N, H, W), res1.second.view(N, H, W)
    zptr = lambda f: ctypes.c_void_p(depth.data_ptr() + ((3 * f + 2) * H * W) * 4 if thr is not None else 0)
    table = TD._build_rois(labels[0], zptr(0), H, W, dev, thr if thr is not None else 0.0)       # filters item 0 in place
    if N > 1 and thr is not None:
        ws = TD._ws(dev)
        _native.call("uoc_filter_labels_depth", dev, labels[1:], zptr(1), 3 * H * W, N - 1, H, W, float(thr), ws, ws.numel())
    refined = margin = stage2 = None
    K = 0
    if network_crop is not None:
        K = int(TD._read_table(table).K)             # the small read between the stages (synchronises)
    TD.LAST_FRAME_STATS["rois"] = K
    if K > 0:
        S = cfg.TRAIN.SYN_CROP_SIZE
        firsts2 = [np.random.randint(0, S * S) for _ in range(K)]
        rgb, mask, dep = TD._crop(image[0], depth[0] if depth is not None else None, labels[0], table, K, H, W, dev)
        X2 = TD._kernel_layout(TD._detach_keep_planes(network_crop(rgb, mask, dep)))
        labels_crop, _, Z2, sl2 = cluster_batch(X2, firsts2, TD.KAPPA, 100, TD.MAX_ITERS, eps, return_parts=True, metric="cosine")
        res2 = assign_confidence(X2, Z2, sl2)
        plan = torch.empty((K + K * NUM_IDS,), dtype=torch.int32, device=dev)
        refined = torch.empty((H * W,), dtype=torch.int32, device=dev)
        status, ws = TD._status_word(dev), TD._ws(dev)
        _native.call("uoc_roi_match", dev, labels_crop, mask, dep, table, K, S, H, W, refined, None, plan, status, ws, ws.numel())
        margin = final_margin(refined, labels[0], res1.margin[0], res2.margin, labels_crop, table, plan, K, H, W).view(H, W)
        stage2 = dict(margin_crop=res2.margin, labels_crop=labels_crop, table=table, plan=plan, labels1=labels[0])
    TD._check_clustering(dev)                         # synchronises
    if K > 0 and TD._take_order_flag(TD._status_word(dev)):
        raise TD.HostOrderNeeded("segment_confidence: NaN ROI sort keys with >= 64 ROIs; the paint plan of the host ordering is "
                                 "not covered")
    labels = labels.view(N, H, W)
    if refined is not None:
        final = refined.view(1, H, W)
        if N > 1:       # match_label_crop paints item 0 only, the rest stays zero (FrameGroupJob.result_device)
            refined = torch.zeros((N, H, W), dtype=torch.int32, device=dev)
            refined[0] = final[0]
        else:
            refined = final
        per_object = summarize(final, margin[None], weak)
    else:
        margin = margin1[0]
        per_object = summarize(labels, margin1, weak)
    conf = FrameConfidence(margin1=margin1, second1=second1, margin=margin, per_object=per_object, rois=K, stage2=stage2)
    if return_device:
        return labels, refined, conf
    return labels.float().cpu(), (refined.float().cpu() if refined is not None else None), conf
