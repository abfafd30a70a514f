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
`fit_plane` neither copies to the host nor synchronises.  No CPU fallback.

Several planes (uoc_support_planes): shelves, walls and the plane the objects stand on.

    res = fit_planes(refined, xyz, max_planes=4)      # the same scheme repeated on what the earlier planes left
    res.count[b], res.normal[b, k], res.cos0[b, k]    # planes found; plane k; its cosine with plane 0
    k = choose_support(res, up=(0.0, -1.0, 0.0))      # [B]: the plane most objects stand on among those facing `up`
    placed = placement.free_space(refined, xyz, res.plane(k))      # every stage that takes `fitted` takes res.plane(k)"""
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


class PlaneResult(_native.Fields):
    """Device tensors.  Per frame: found, candidates, inliers, hyp [B] int32; normal, centroid, eig, u, v [B,3]; d, rms [B].
    Per (frame, id): count [B,128] int32; height_min, height_max [B,128]; foot, axis [B,128,2]; cov2, half, center
    [B,128,3].  height: [B,H,W] (NaN where there is no valid point) with height_map=True, else None.  records: the
    uoc_plane records themselves, [B,21] int32 (what placement.free_space reads in place)."""


def _view(rec, layout, name, integer):
    o, n = layout[name]
    v = rec[..., o:o + n]
    v = v if integer else v.view(torch.float32)
    return v[..., 0] if n == 1 else v


def plane_records(labels, xyz, num_hyp, tau_mm, seed, height_map=False):
    """The raw uoc_support_plane call: (planes [B,21] int32 holding uoc_plane, objects [B,128,16] int32 holding
    uoc_plane_object, height [B,H,W] float32 or None), on the device, no synchronisation.  labels int32 [B,H,W] and xyz
    float32 [B,3,H,W] contiguous on one GPU."""
    B, H, W = (int(v) for v in labels.shape)
    dev = labels.device
    ws = _native.workspace("uoc_plane_workspace_bytes", dev, B, H, W, int(num_hyp), who="fit_plane",
                           hint=f"B={B} H={H} W={W} or num_hyp={num_hyp} (1..{_native.PLANE_MAX_HYP})")
    planes = torch.empty((B, _PW), dtype=torch.int32, device=dev)
    objs = torch.empty((B, NUM_IDS, _OW), dtype=torch.int32, device=dev)
    height = torch.empty((B, H, W), dtype=torch.float32, device=dev) if height_map else None
    _native.call("uoc_support_plane", dev, labels, xyz, B, H, W, int(num_hyp), int(tau_mm), int(seed) & 0xFFFFFFFF, planes, objs,
                 height, ws, ws.numel())
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
    lab, xyz = _native.frame_inputs("fit_plane", labels, xyz)
    planes, objs, height = plane_records(lab, xyz, num_hyp, tau_mm, seed, height_map)
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


# ---- several planes (uoc_support_planes) ------------------------------------------------------------
_INFO = _layout(_native.UocPlaneInfo)
_IW = sum(n for _, n in _INFO.values())
INFO_INT_FIELDS = ("round_candidates", "removed")
INFO_FIELDS = tuple(_INFO)


class PlanesResult(_native.Fields):
    """Device tensors.  count [B] int32: the planes found.  Per (frame, plane): every uoc_plane field as in PlaneResult
    with a plane axis ([B,K] / [B,K,3]); round_candidates, removed [B,K] int32; cos0, offset0 [B,K]; extent [B,K,4].  Per
    (frame, plane, id): every uoc_plane_object field, [B,K,128,...] (zeros with objects=False); its point count is named
    obj_count here, count being the number of planes.  index [B,H,W] int32: -2
    not a candidate, k an inlier of plane k, 16 + k the removal fringe of plane k, -1 a candidate no plane took.
    records [B,K,21] int32, the uoc_plane records themselves."""

    def plane(self, k) -> PlaneResult:
        """Plane k of every frame as a PlaneResult (contiguous [B,21] records, the object fields, height=None): what every
        stage that takes `fitted` takes.  k: an int, or a [B] int64 device tensor (one plane per frame), gathered on the
        device without a host read."""
        B, K = int(self.records.shape[0]), int(self.records.shape[1])
        if isinstance(k, torch.Tensor):
            if k.dim() != 1 or int(k.shape[0]) != B or k.device != self.records.device:
                raise _native.NativeError(f"PlanesResult.plane: k must be a [B] = [{B}] tensor on the result's device")
            kk = k.to(torch.int64).clamp(0, K - 1)
            rows = torch.arange(B, device=kk.device)
            planes, objs = self.records[rows, kk].contiguous(), self._objs[rows, kk].contiguous()
        else:
            if not 0 <= int(k) < K:
                raise ValueError(f"PlanesResult.plane: k = {k} outside 0..{K - 1}")
            planes, objs = self.records[:, int(k)].contiguous(), self._objs[:, int(k)].contiguous()
        fields = {f: _view(planes, _PLANE, f, f in PLANE_INT_FIELDS) for f in PLANE_FIELDS}
        fields.update({f: _view(objs, _OBJECT, f, f == "count") for f in OBJECT_FIELDS})
        return PlaneResult(height=None, num_hyp=self.num_hyp, tau_mm=self.tau_mm, seed=self.seed, records=planes, **fields)


def planes_records(labels, xyz, max_planes, num_hyp, tau_mm, rem_mm, min_inliers, seed, objects=True):
    """The raw uoc_support_planes call: (count [B], planes [B,K,21], info [B,K,8], index [B,H,W], objects [B,K,128,16] or
    None), int32 on the device, no synchronisation.  labels int32 [B,H,W] and xyz float32 [B,3,H,W] contiguous on one GPU."""
    B, H, W = (int(v) for v in labels.shape)
    K = int(max_planes)
    dev = labels.device
    ws = _native.workspace("uoc_planes_workspace_bytes", dev, B, H, W, int(num_hyp), K, who="fit_planes",
                           hint=f"B={B} H={H} W={W}, num_hyp={num_hyp} (1..{_native.PLANE_MAX_HYP}), "
                                f"max_planes={K} (1..{_native.PLANES_MAX}) or B * max_planes above 65535")
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    planes = torch.empty((B, K, _PW), dtype=torch.int32, device=dev)
    info = torch.empty((B, K, _IW), dtype=torch.int32, device=dev)
    index = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    objs = torch.empty((B, K, NUM_IDS, _OW), dtype=torch.int32, device=dev) if objects else None
    _native.call("uoc_support_planes", dev, labels, xyz, B, H, W, K, int(num_hyp), int(tau_mm), int(rem_mm), int(min_inliers),
                 int(seed) & 0xFFFFFFFF, count, planes, info, index, objs, ws, ws.numel())
    return count, planes, info, index, objs


def fit_planes(labels, xyz, max_planes=4, num_hyp=256, tau=0.010, remove=None, min_inliers=None, seed=1,
               objects=True) -> PlanesResult:
    """Up to max_planes (1..8) planes of the background, extracted one after the other: labels, xyz, num_hyp, tau and seed
    as in fit_plane.  A plane's inliers lie within tau of it; every candidate within `remove` metres (default 2*tau, at
    least tau, used in whole millimetres) is taken out before the next round, so that the fringe of a plane cannot seed a
    copy of it.  A round whose best hypothesis has fewer than min_inliers (default max(3, H*W // 50)) inliers ends the
    extraction.  Plane 0 is fit_plane's plane bit for bit.  objects=False skips the per-plane object tables (all zero)."""
    if not 1 <= int(max_planes) <= _native.PLANES_MAX:
        raise ValueError(f"max_planes = {max_planes} outside 1..{_native.PLANES_MAX}")
    if not 1 <= int(num_hyp) <= _native.PLANE_MAX_HYP:
        raise ValueError(f"num_hyp = {num_hyp} outside 1..{_native.PLANE_MAX_HYP}")
    tau_mm = int(round(float(tau) * 1000))
    if not 1 <= tau_mm <= _native.PLANE_MAX_TAU_MM:
        raise ValueError(f"tau = {tau} m is {tau_mm} mm, outside 1..{_native.PLANE_MAX_TAU_MM} mm")
    rem_mm = 2 * tau_mm if remove is None else int(round(float(remove) * 1000))
    if remove is None:
        rem_mm = min(rem_mm, _native.PLANE_MAX_TAU_MM)
    if not tau_mm <= rem_mm <= _native.PLANE_MAX_TAU_MM:
        raise ValueError(f"remove = {remove} m is {rem_mm} mm, outside tau = {tau_mm}..{_native.PLANE_MAX_TAU_MM} mm")
    if min_inliers is not None and int(min_inliers) < 3:
        raise ValueError(f"min_inliers = {min_inliers} below 3")
    lab, xyz = _native.frame_inputs("fit_planes", labels, xyz)
    B, H, W = (int(v) for v in lab.shape)
    mi = max(3, H * W // 50) if min_inliers is None else int(min_inliers)
    count, planes, info, index, objs = planes_records(lab, xyz, max_planes, num_hyp, tau_mm,
                                                      rem_mm, mi, seed, objects)
    if objs is None:
        objs = torch.zeros((B, int(max_planes), NUM_IDS, _OW), dtype=torch.int32, device=lab.device)
    fields = {k: _view(planes, _PLANE, k, k in PLANE_INT_FIELDS) for k in PLANE_FIELDS}
    fields.update({k: _view(info, _INFO, k, k in INFO_INT_FIELDS) for k in INFO_FIELDS})
    fields["obj_count"] = _view(objs, _OBJECT, "count", True)
    fields.update({k: _view(objs, _OBJECT, k, False) for k in OBJECT_FIELDS if k != "count"})
    return PlanesResult(count=count, index=index, records=planes, info=info, _objs=objs, max_planes=int(max_planes),
                        num_hyp=int(num_hyp), tau_mm=tau_mm, rem_mm=rem_mm, min_inliers=mi, seed=int(seed) & 0xFFFFFFFF,
                        **fields)


def _found(res):
    K = int(res.records.shape[1])
    return torch.arange(K, device=res.count.device)[None, :] < res.count[:, None].to(torch.int64)


def planes_like(res, like, par_deg=15.0):
    """[B,K] bool: the found planes whose normal lies within par_deg degrees of a reference direction, by signed cosine
    (a plane facing the other way is not alike).  like: a plane index (the direction is that plane's normal, per frame;
    a frame that has not found it has no plane alike), or an `up` vector of 3 numbers in camera coordinates (a tensor
    [3] or [B,3] on the device works too).  Torch ops on the tables: no kernel of its own, no synchronisation."""
    import math
    normal = res.normal                                                     # [B,K,3]
    if isinstance(like, int):
        if not 0 <= like < int(normal.shape[1]):
            raise ValueError(f"planes_like: plane {like} outside 0..{int(normal.shape[1]) - 1}")
        ref = normal[:, like]
    else:
        ref = torch.as_tensor(like, dtype=torch.float32, device=normal.device)
        if ref.shape[-1] != 3 or ref.dim() > 2:
            raise ValueError("planes_like: `like` is a plane index or a direction of 3 numbers")
        ref = ref.expand(normal.shape[0], 3) if ref.dim() == 1 else ref
        ref = ref / ref.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    cos = (normal * ref[:, None, :]).sum(-1)
    return _found(res) & (cos >= math.cos(math.radians(float(par_deg))))


def standing_on(res, like=0, tol=0.02, par_deg=15.0):
    """[B,128] int64: per id with points, the plane it stands on: among the planes alike `like` (planes_like) those the
    id does not reach below (height_min >= -tol metres), and of these the one with the smallest height_min, ties to the
    lowest k; -1 for an id without points or without such a plane.  The contact of an object is usually not visible from
    above, so "stands on" means "the nearest plane of the class below its lowest visible point"."""
    K = int(res.records.shape[1])
    cls = planes_like(res, like, par_deg)                                   # [B,K]
    hm = res.height_min                                                     # [B,K,128]
    ok = cls[:, :, None] & (res.obj_count > 0) & (hm >= -float(tol))
    val = torch.where(ok, hm, torch.full_like(hm, float("inf")))
    best = val.amin(dim=1, keepdim=True)
    ks = torch.arange(K, device=hm.device)[None, :, None].expand_as(hm)
    first = torch.where(ok & (val == best), ks, torch.full_like(ks, K)).amin(dim=1)
    return torch.where(first < K, first, torch.full_like(first, -1))


def choose_support(res, up=None, tol=0.02, par_deg=15.0):
    """[B] int64: the support plane of every frame: among the planes alike `up` (planes_like; up=None takes plane 0's
    normal, which is fit_plane's behaviour whenever plane 0 is the table) the one most ids stand on (standing_on), ties to
    the lowest k; 0 for a frame without a plane of the class.  The limit: without a gravity hint a frame dominated by a
    wall has the wall as plane 0, and then only `up` (camera coordinates, pointing away from the floor) finds the table."""
    K = int(res.records.shape[1])
    like = 0 if up is None else up
    cls = planes_like(res, like, par_deg)
    on = standing_on(res, like, tol, par_deg)[:, 1:]                        # [B,127]
    ks = torch.arange(K, device=on.device)
    votes = (on[:, None, :] == ks[None, :, None]).sum(-1)                   # [B,K]
    votes = torch.where(cls, votes, torch.full_like(votes, -1))
    best = votes.amax(dim=1, keepdim=True)
    first = torch.where(cls & (votes == best), ks[None, :].expand_as(votes), torch.full_like(votes, K)).amin(dim=1)
    return torch.where(first < K, first, torch.zeros_like(first))
