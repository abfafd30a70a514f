"""Per-object point clouds and 3D statistics from label maps, on the device (uoc_objects, include/uoc_hip.h).

    objs = extract_objects(labels, xyz)               # labels [B,H,W] / [H,W] on the GPU, xyz = sample['depth'] [B,3,H,W]
    objs.centroid[k], objs.obb_center[k], objs.cloud(k)

A pixel of object l has label l in [1, 127]; a valid point is such a pixel with finite x, y, z and z > 0.  The records
and the packed clouds are computed by HIP kernels in a fixed summation order (bitwise reproducible, independent of the
batch); the only host traffic is one small read of the per-object counts that sizes the result.  No CPU fallback.
"""
from __future__ import annotations


import torch

from . import _native

NUM_IDS = 128
_W = _native.OBJECT_BYTES // 4          # 4-byte words per record
_F = {name: (getattr(_native.UocObject, name).offset // 4, getattr(_native.UocObject, name).size // 4)
      for name, _ in _native.UocObject._fields_}
_COV_INDEX = [0, 1, 2, 1, 3, 4, 2, 4, 5]   # xx, xy, xz, yy, yz, zz -> 3x3


class ObjectSet(_native.Fields):
    """Objects of the (frame, id) pairs with pixels > 0 and count >= min_points, in ascending (frame, id) order.
    Every tensor lives on the device of the inputs; K = len(self).

    frame, label, pixels, count [K] int32; box [K,4] int32 (x0, y0, x1, y1 inclusive); centroid, aabb_min, aabb_max,
    eigenvalues (descending), obb_center, obb_half [K,3]; cov, axes [K,3,3] (column k of axes = e_k);
    points [P,3]; pixel_index [P] int32 (raster index y*W + x in its frame); attrs [P,C] or None; offsets [K+1] int64:
    the rows of object k are points[offsets[k]:offsets[k+1]]."""

    def __len__(self):
        return int(self.frame.shape[0])

    def cloud(self, k):
        """Points of object k, [n,3]."""
        return self.points[self._offsets_host[k]:self._offsets_host[k + 1]]


def _workspace(dev, B, H, W):
    return _native.workspace("uoc_objects_workspace_bytes", dev, B, H, W, who="extract_objects", hint=f"B={B} H={H} W={W}", floor=1)


def object_records(labels, xyz, attrs=None, max_points_per_object=None, capacity=None, want_points=True):
    """The raw uoc_objects call: (records [B,128,41] int32 holding uoc_object, points [cap,3], point_attr [cap,C] or None,
    pixel_index [cap], total [1] int32), all on the device, no synchronisation.  labels int32 [B,H,W] and xyz float32
    [B,3,H,W] contiguous on one GPU; capacity defaults to B*H*W (always enough)."""
    B, H, W = labels.shape
    dev = labels.device
    C = 0 if attrs is None else int(attrs.shape[1])
    lib = _native.lib()
    cap = B * H * W if capacity is None else int(capacity)
    rec = torch.empty((B, NUM_IDS, _W), dtype=torch.int32, device=dev)
    pts = torch.empty((cap, 3), dtype=torch.float32, device=dev) if want_points else None
    pat = torch.empty((cap, C), dtype=torch.float32, device=dev) if (want_points and C) else None
    pix = torch.empty((cap,), dtype=torch.int32, device=dev) if want_points else None
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    nws = lib.uoc_objects_workspace_bytes(B, H, W)
    ws = _workspace(dev, B, H, W)
    M = 0 if max_points_per_object is None else int(max_points_per_object)
    _native.call("uoc_objects", dev, labels, xyz, attrs, C, B, H, W, M, rec, pts, pat, pix, cap, total, ws, nws)
    return rec, pts, pat, pix, total


def _field(rec, name, dtype=torch.float32):
    o, n = _F[name]
    v = rec[..., o:o + n]
    return v.view(torch.float32) if dtype == torch.float32 else v


def extract_objects(labels, xyz, attrs=None, max_points_per_object=None, min_points=1) -> ObjectSet:
    """labels: device tensor [B,H,W] or [H,W] of int32 / int64 / float ids (test_sample's maps are float32);
    xyz: [B,3,H,W] or [3,H,W] float metres (sample['depth']); attrs: optional [B,C,H,W] / [C,H,W], C <= 8, gathered
    verbatim per point.  max_points_per_object = M keeps the points of in-object rank floor(j*count/M), j < M, of an
    object with count > M.  Objects with pixels > 0 and count >= min_points are returned."""
    lab, xyz = _native.frame_inputs("extract_objects", labels, xyz)
    dev = lab.device
    if attrs is not None:
        if not _native.on_gpu(attrs):
            raise _native.NativeError("extract_objects: attrs must be a tensor on the GPU (there is no CPU fallback)")
        if attrs.dim() == 3:
            attrs = attrs[None]
        if attrs.dim() != 4 or attrs.shape[0] != lab.shape[0] or tuple(attrs.shape[2:]) != tuple(lab.shape[1:]) \
                or not 1 <= attrs.shape[1] <= _native.OBJECTS_MAX_ATTR or attrs.device != dev:
            raise _native.NativeError(f"extract_objects: attrs {tuple(attrs.shape)} must be [B,C,H,W] with 1 <= C <= 8")
        attrs = attrs.to(torch.float32).contiguous()
    rec, pts, pat, pix, total = object_records(lab, xyz, attrs, max_points_per_object)

    head = torch.cat([_field(rec, "pixels", torch.int32), _field(rec, "count", torch.int32), _field(rec, "offset", torch.int32),
                      _field(rec, "kept", torch.int32)], dim=-1).reshape(-1, 4).cpu()       # the one D2H read
    keep = (head[:, 0] > 0) & (head[:, 1] >= min_points)
    sel = torch.nonzero(keep).reshape(-1)
    kept = head[sel, 3].to(torch.int64)
    offsets_host = [0] + torch.cumsum(kept, 0).tolist()
    n_out = offsets_host[-1]
    starts = head[sel, 2].to(torch.int64)
    sel_d = sel.to(dev)
    flat = rec.reshape(-1, _W)[sel_d]
    if n_out == int(head[:, 3].sum()):          # every kept row belongs to a returned object: already packed in order
        rows = None
    else:
        base = starts - torch.tensor(offsets_host[:-1], dtype=torch.int64)
        rows = (torch.repeat_interleave(base, kept) + torch.arange(n_out, dtype=torch.int64)).to(dev)

    def take(t):
        if t is None:
            return None
        return t[:n_out] if rows is None else t[rows]

    K = int(sel.numel())
    return ObjectSet(
        frame=(sel_d // NUM_IDS).to(torch.int32), label=(sel_d % NUM_IDS).to(torch.int32),
        pixels=_field(flat, "pixels", torch.int32)[:, 0].clone(), count=_field(flat, "count", torch.int32)[:, 0].clone(),
        box=_field(flat, "box", torch.int32).clone(), centroid=_field(flat, "centroid").clone(),
        cov=_field(flat, "cov")[:, _COV_INDEX].reshape(K, 3, 3), aabb_min=_field(flat, "aabb_min").clone(),
        aabb_max=_field(flat, "aabb_max").clone(), eigenvalues=_field(flat, "eig").clone(),
        axes=_field(flat, "axes").reshape(K, 3, 3).clone(), obb_center=_field(flat, "obb_center").clone(),
        obb_half=_field(flat, "obb_half").clone(), points=take(pts), attrs=take(pat), pixel_index=take(pix),
        offsets=torch.tensor(offsets_host, dtype=torch.int64, device=dev), _offsets_host=offsets_host,
        image_size=(int(lab.shape[1]), int(lab.shape[2])))


def segment_objects(sample, network, network_crop, use_refined=True, plane=False, plane_args=None, relations=False,
                    relations_args=None, placement=False, placement_args=None, grasp=False, grasp_args=None, elevation=False,
                    elevation_args=None, footprint=False, footprint_args=None, routes=False, routes_args=None, confidence=False,
                    confidence_args=None, normals=False, normals_args=None, planes=False, planes_args=None, memory=None, memory_args=None,
                    **kw):
    """One frame through the two-stage path (test_dataset._run_frame, device label maps), then extract_objects on the
    refined map (item 0, as the reference refines only item 0) where there is one and use_refined, else on the stage-1
    maps.  Returns (out_label, out_label_refined, objects): the label maps exactly as test_sample returns them (float32,
    host), copied only after the extraction was enqueued.  kw goes to extract_objects.  With plane=True the support
    plane of the same maps (support.fit_plane, plane_args = its keyword arguments) is returned as a fourth item; with
    relations=True the objects' relations on the same maps (relations.relate, relations_args = its keyword arguments)
    come as a further item after it.  placement=True implies plane=True and adds, as the last item, the free space on
    that plane (placement.free_space, placement_args = its keyword arguments).  grasp=True implies placement=True and
    adds, after it, the grasp candidates of the objects on that grid (grasp.candidates, grasp_args = its keyword
    arguments).  elevation=True implies placement=True and adds, as the last item, the elevation map on that grid
    (elevation.heights, elevation_args = its keyword arguments).  footprint=True implies placement=True and adds, after
    the elevation item, the oriented put-down poses of the rectangles footprint_args["rects"] on that grid
    (footprint.fit, footprint_args = its keyword arguments, `rects` among them).  routes=True implies placement=True and
    adds, as the last item, the slide paths of the queries routes_args["queries"] on that grid (routes.plan, routes_args =
    its keyword arguments, `queries` among them).  confidence=True takes the frame through confidence.segment_confidence
    instead (the same label maps, with the assignment margins alongside; confidence_args = its keyword arguments) and
    adds its FrameConfidence as a further item; cosine metric only (NotImplementedError under the euclidean opt-in).
    normals=True implies plane=True and adds, as the last item of all, the surface normals and object faces of the same
    maps against that plane (normals.estimate, normals_args = its keyword arguments).  planes=True adds, as the last
    item of all, the several planes of the same maps (support.fit_planes; planes_args = its keyword arguments, and `up`,
    `tol`, `par_deg` of support.choose_support among them).  With it the plane of plane=True (and so of placement=True
    and every switch that implies it) is not fit_plane's but res.plane(choose_support(res, ...)), the plane most objects
    stand on, chosen on the device; plane_args is then not used.  memory=a scene.Memory implies placement=True, fuses this
    frame's free space into that memory (Memory.update, memory_args = its keyword arguments) and adds the SceneResult as
    the last item of all; the placement item and the stages on it stay those of this frame alone."""
    if footprint and "rects" not in (footprint_args or {}):
        raise ValueError("segment_objects: footprint=True needs footprint_args with `rects`")
    if routes and "queries" not in (routes_args or {}):
        raise ValueError("segment_objects: routes=True needs routes_args with `queries`")
    from . import io as uio
    from .fcn import test_dataset as TD
    dev = TD._device()
    if "depth" not in sample and "depth_u16" in sample:       # raw sample (io.read_sample_raw): prepare it on the device
        sample = uio.prepare_on_device(sample, dev)
    if sample.get("depth") is None:
        raise _native.NativeError("segment_objects needs the XYZ planes (sample['depth'])")
    if confidence:
        from .confidence import segment_confidence
        labels, refined, conf = segment_confidence(sample, network, network_crop, return_device=True, **(confidence_args or {}))
    else:
        labels, refined = TD._run_frame(sample, network, network_crop, TD.DEPTH_FILTER, return_device=True, checked=True)
    xyz = sample["depth"].to(dev)
    src, src_xyz = (refined[:1], xyz[:1]) if use_refined and refined is not None else (labels, xyz)
    objs = extract_objects(src, src_xyz, **kw)
    placement = placement or grasp or elevation or footprint or routes or memory is not None
    plane = plane or placement or normals
    if planes:
        from .support import choose_support, fit_planes
        pa = dict(planes_args or {})
        choose = {k: pa.pop(k) for k in ("up", "tol", "par_deg") if k in pa}
        several = fit_planes(src, src_xyz, **pa)
        if plane:
            fitted = several.plane(choose_support(several, **choose))
    elif plane:
        from .support import fit_plane
        fitted = fit_plane(src, src_xyz, **(plane_args or {}))
    if relations:
        from .relations import relate
        related = relate(src, src_xyz, **(relations_args or {}))
    if placement:
        from .placement import free_space
        placed = free_space(src, src_xyz, fitted, **(placement_args or {}))
    if grasp:
        from .grasp import candidates
        grasped = candidates(placed, **(grasp_args or {}))
    if elevation:
        from .elevation import heights
        raised = heights(src, src_xyz, placed, **(elevation_args or {}))
    if footprint:
        from .footprint import fit
        fitting = fit(placed, **footprint_args)
    if routes:
        from .routes import plan
        routed = plan(placed, **routes_args)
    if normals:
        from .normals import estimate
        estimated = estimate(src_xyz, src, fitted, **(normals_args or {}))
    if memory is not None:
        remembered = memory.update(placed, **(memory_args or {}))
    out_label = labels.float().cpu()
    out_refined = refined.float().cpu() if refined is not None else None
    return (out_label, out_refined, objs) + ((fitted,) if plane else ()) + ((related,) if relations else ()) \
        + ((placed,) if placement else ()) + ((grasped,) if grasp else ()) + ((raised,) if elevation else ()) \
        + ((fitting,) if footprint else ()) + ((routed,) if routes else ()) + ((conf,) if confidence else ()) \
        + ((estimated,) if normals else ()) + ((several,) if planes else ()) + ((remembered,) if memory is not None else ())
