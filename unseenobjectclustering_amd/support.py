"""The surface the objects stand on, and every object's height above it, on the device (uoc_support_plane,
include/uoc_hip.h).

    res = fit_plane(refined, xyz)                     # labels [B,H,W] / [H,W] on the GPU, xyz = sample['depth'] [B,3,H,W]
    res.normal[b], res.d[b]                           # normal.p + d = 0, the camera on the positive side
    res.height_max[b, k], res.center[b, k]            # object k: height above the plane, upright box
    labels = drop_flat(refined, res, 0.01)            # ids lower than 1 cm (a patch of tablecloth) become background

The background pixels of the label map (every id outside 1..127) with a valid point are the plane candidates; `num_hyp`
three-point hypotheses are scored in exact integer arithmetic on millimetre coordinates (inliers within `tau`), the winner
(ties: the lowest hypothesis index) is refined once in fp64 over its inliers, and every id is measured against the refined
plane.  Everything is computed by HIP kernels in a fixed order: bitwise reproducible and independent of the batch.
`fit_plane` neither copies to the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

import torch

from . import _native

NUM_IDS = 128


def _layout(struct):
    return {name: (getattr(struct, name).offset // 4, getattr(struct, name).size // 4) for name, _ in struct._fields_}


_PLANE = _layout(_native.UocPlane)
_OBJECT = _layout(_native.UocPlaneObject)
_PW = sum(n for _, n in _PLANE.values())
_OW = sum(n for _, n in _OBJECT.values())
PLANE_INT_FIELDS = ("found", "candidates", "inliers", "hyp")
PLANE_FIELDS = tuple(_PLANE)
OBJECT_FIELDS = tuple(_OBJECT)


class PlaneResult:
    """Device tensors.  Per frame: found, candidates, inliers, hyp [B] int32; normal, centroid, eig, u, v [B,3]; d, rms [B].
    Per (frame, id): count [B,128] int32; height_min, height_max [B,128]; foot, axis [B,128,2]; cov2, half, center
    [B,128,3].  height: [B,H,W] (NaN where there is no valid point) with height_map=True, else None.  records: the
    uoc_plane records themselves, [B,21] int32 (what placement.free_space reads in place)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _view(rec, layout, name, integer):
    o, n = layout[name]
    v = rec[..., o:o + n]
    v = v if integer else v.view(torch.float32)
    return v[..., 0] if n == 1 else v


def _on_gpu(t):
    return isinstance(t, torch.Tensor) and t.device.type == "cuda"


def plane_records(labels, xyz, num_hyp, tau_mm, seed, height_map=False):
    """The raw uoc_support_plane call: (planes [B,21] int32 holding uoc_plane, objects [B,128,16] int32 holding
    uoc_plane_object, height [B,H,W] float32 or None), on the device, no synchronisation.  labels int32 [B,H,W] and xyz
    float32 [B,3,H,W] contiguous on one GPU."""
    B, H, W = (int(v) for v in labels.shape)
    dev = labels.device
    lib = _native.lib()
    nws = lib.uoc_plane_workspace_bytes(B, H, W, int(num_hyp))
    if nws == 0:
        raise _native.NativeError(f"fit_plane: bad shape B={B} H={H} W={W} or num_hyp={num_hyp} (1..{_native.PLANE_MAX_HYP})")
    planes = torch.empty((B, _PW), dtype=torch.int32, device=dev)
    objs = torch.empty((B, NUM_IDS, _OW), dtype=torch.int32, device=dev)
    height = torch.empty((B, H, W), dtype=torch.float32, device=dev) if height_map else None
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)      # from torch's stream-ordered cache: no allocation in steady state
    with torch.cuda.device(dev):
        rc = lib.uoc_support_plane(_native.ptr(labels), _native.ptr(xyz), B, H, W, int(num_hyp), int(tau_mm),
                                   int(seed) & 0xFFFFFFFF, _native.ptr(planes), _native.ptr(objs), _native.ptr(height),
                                   _native.ptr(ws), nws, _native.stream_ptr(dev))
    _native.check(rc, "uoc_support_plane")
    return planes, objs, height


def fit_plane(labels, xyz, num_hyp=256, tau=0.010, seed=1, height_map=False) -> PlaneResult:
    """labels: device tensor [B,H,W] or [H,W] of int32 / int64 / float ids; xyz: [B,3,H,W] or [3,H,W] float metres
    (sample['depth']).  num_hyp in 1..1024 hypotheses; tau = inlier distance in metres, used in whole millimetres
    (int(round(tau*1000)) in 1..1000); seed picks the hypotheses.  Returns a PlaneResult."""
    if not 1 <= int(num_hyp) <= _native.PLANE_MAX_HYP:
        raise ValueError(f"num_hyp = {num_hyp} outside 1..{_native.PLANE_MAX_HYP}")
    tau_mm = int(round(float(tau) * 1000))
    if not 1 <= tau_mm <= _native.PLANE_MAX_TAU_MM:
        raise ValueError(f"tau = {tau} m is {tau_mm} mm, outside 1..{_native.PLANE_MAX_TAU_MM} mm")
    for t, what in ((labels, "labels"), (xyz, "xyz")):
        if not _on_gpu(t):
            raise _native.NativeError(f"fit_plane: {what} must be a tensor on the GPU (there is no CPU fallback)")
    if labels.dim() == 2:
        labels = labels[None]
    if xyz.dim() == 3:
        xyz = xyz[None]
    if labels.dim() != 3 or xyz.dim() != 4 or xyz.shape[1] != 3 or xyz.shape[0] != labels.shape[0] \
            or tuple(xyz.shape[2:]) != tuple(labels.shape[1:]):
        raise _native.NativeError(f"fit_plane: labels {tuple(labels.shape)} and xyz {tuple(xyz.shape)} do not match "
                                  "([B,H,W] and [B,3,H,W])")
    if xyz.device != labels.device:
        raise _native.NativeError("fit_plane: labels and xyz are on different devices")
    lab = (labels if labels.dtype == torch.int32 else labels.to(torch.int32)).contiguous()
    planes, objs, height = plane_records(lab, xyz.to(torch.float32).contiguous(), num_hyp, tau_mm, seed, height_map)
    fields = {k: _view(planes, _PLANE, k, k in PLANE_INT_FIELDS) for k in PLANE_FIELDS}
    fields.update({k: _view(objs, _OBJECT, k, k == "count") for k in OBJECT_FIELDS})
    return PlaneResult(height=height, num_hyp=int(num_hyp), tau_mm=tau_mm, seed=int(seed) & 0xFFFFFFFF, records=planes,
                       **fields)


def standing_objects(result, min_height):
    """[B,128] bool: the ids with a valid point whose top is at least min_height metres above the plane."""
    return (result.height_max >= float(min_height)) & (result.count > 0)


def drop_flat(labels, result, min_height):
    """The label map with every id 1..127 that is not standing (standing_objects) set to 0; other values pass through.
    A gather through a [B,128] table: it stays on the device.  labels [B,H,W] or [H,W] (B = 1), any integer or float dtype."""
    keep = standing_objects(result, min_height)
    lab3 = labels[None] if labels.dim() == 2 else labels
    if lab3.dim() != 3 or lab3.shape[0] != keep.shape[0]:
        raise _native.NativeError(f"drop_flat: labels {tuple(labels.shape)} do not match the result's {keep.shape[0]} frames")
    ids = lab3.to(torch.int64)
    obj = (ids >= 1) & (ids < NUM_IDS)
    kept = torch.gather(keep, 1, ids.clamp(0, NUM_IDS - 1).reshape(keep.shape[0], -1)).reshape(ids.shape)
    out = torch.where(obj & ~kept, torch.zeros_like(lab3), lab3)
    return out.reshape(labels.shape)
