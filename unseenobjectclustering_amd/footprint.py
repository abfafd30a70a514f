"""Where an elongated object can be put down, and turned which way: oriented rectangles on the table grid, on the device
(uoc_footprint, include/uoc_hip.h).

    placed = placement.free_space(refined, xyz, fitted)          # the top-down grid of §15, on the GPU
    box = rect(0.30, 0.06, placed.cell_mm)                       # a 30 cm x 6 cm footprint, inflated to be conservative
    res = fit(placed, [box, of_object(fitted, 0, 3, placed.cell_mm)])   # 16 orientations over half a turn
    res.fits[b, f]                                               # [G,G] int32: bit k = it fits there along direction k
    res.count[b, f, k], res.best[b, f]                           # cells per direction; (ok, i, j, k, dist2, da, poses, cells)
    fits_mask(res, 0)                                            # [B,G,G] bool on the device: in any orientation
    pose(res, 0, 0)                                              # centre and long axis in camera coordinates

A rectangle fits at a cell along direction k when every cell whose centre lies inside it, turned to that direction and
centred on the cell, is free: table, unknown when `unknown_blocks` is off, or part of the object `ignore` (the object
being moved does not block itself).  Integer arithmetic in HIP kernels: defined exactly, independent of launch order and
batch.  `fit` neither copies to the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _native, placement
from .grasp import direction_table

ROOMIEST, NEAREST = _native.FOOT_ROOMIEST, _native.FOOT_NEAREST
BEST_FIELDS = ("ok", "i", "j", "k", "dist2", "da", "poses", "cells")
INFLATE = 184                     # 0.71875 cell in units of 1/256: half a cell's diagonal (0.7072) and the table's rounding (66/16384)
FootprintPose = namedtuple("FootprintPose", "center axis k angle cell dist2")


class FootprintResult(_native.Fields):
    """Device tensors.  fits [B,F,G,G] int32: bit k of a word is set when rectangle f fits at the cell along direction k;
    count [B,F,32] int32: the cells per direction; best [B,F,8] int32: BEST_FIELDS per rectangle.  dirs: the direction
    table [A,2] and rects: the records [F,8] (host, numpy).  grid, cell_mm, planes: of the placement result the grids came
    from."""


def _radius(HL, HW):
    q, R = HL * HL + HW * HW, 0
    while (256 * R) ** 2 < q:
        R += 1
    return R


def _check_rects(rects):
    r = np.asarray(rects, dtype=np.int64)
    if r.ndim == 1 and r.size == 8:
        r = r[None]
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"rects has shape {r.shape}, not [F,8]")
    if not 1 <= len(r) <= _native.FOOT_MAX_RECTS:
        raise ValueError(f"{len(r)} rectangles, outside 1..{_native.FOOT_MAX_RECTS}")
    lim, anchor = _native.FOOT_MAX_HALF, _native.PLACE_MAX_ANCHOR
    for f, (HL, HW, ignore, mode, ai, aj, z6, z7) in enumerate(r.tolist()):
        if not (0 <= HL <= lim and 0 <= HW <= lim and HL * HL + HW * HW <= lim * lim):
            raise ValueError(f"rectangle {f}: half extents ({HL}, {HW}) outside 0..{lim} or longer than {lim} together")
        if not (0 <= ignore < 128 and mode in (ROOMIEST, NEAREST) and -anchor <= ai < anchor and -anchor <= aj < anchor and z6 == 0 and z7 == 0):
            raise ValueError(f"rectangle {f}: (ignore in 0..127, mode 0 or 1, ai, aj in -{anchor}..{anchor - 1}, two zero words), "
                             f"not {(ignore, mode, ai, aj, z6, z7)}")
    return np.ascontiguousarray(r.astype(np.int32))


def footprint_records(state, owner, dist2, frame, dirs, rects, unknown_blocks):
    """The raw uoc_footprint call on bare grids: (fits [B,F,G,G], count [B,F,32], best [B,F,8]) int32 on the device, no
    synchronisation.  state, owner, dist2: device tensors [B,G,G] or [G,G] of any integer type and layout (they are made
    int32 and contiguous); frame: [B,16] int64 on the device, or None; dirs: [A,2] integers in -S..S; rects: [F,8]."""
    if not _native.on_gpu(dist2):
        raise _native.NativeError("footprint: dist2 must be a tensor on the GPU (there is no CPU fallback)")
    st, ow = _native.grid_inputs("footprint", state, owner)
    d2 = _native.as_labels(dist2[None] if dist2.dim() == 2 else dist2)
    if tuple(d2.shape) != tuple(st.shape) or d2.device != st.device:
        raise _native.NativeError(f"footprint: state {tuple(st.shape)}, owner {tuple(ow.shape)} and dist2 {tuple(d2.shape)} "
                                  "are not three [B,G,G] grids on one device")
    B, G = int(st.shape[0]), int(st.shape[1])
    dev = st.device
    if frame is not None:
        if not (isinstance(frame, torch.Tensor) and frame.device == dev and frame.dtype == torch.int64 and tuple(frame.shape) == (B, 16)):
            raise _native.NativeError(f"footprint: the frame records do not match the {B} frames on {dev}")
        frame = frame.contiguous()
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.int64))
    if d.ndim != 2 or d.shape[1] != 2:
        raise ValueError(f"dirs has shape {d.shape}, not [A,2]")
    A = int(d.shape[0])
    if not 1 <= A <= _native.GRASP_MAX_DIRS:
        raise ValueError(f"angles = {A} outside 1..{_native.GRASP_MAX_DIRS}")
    if np.abs(d).max() > _native.GRASP_SCALE:
        raise ValueError(f"dirs has a component outside -{_native.GRASP_SCALE}..{_native.GRASP_SCALE}")
    r = _check_rects(rects)
    F = len(r)
    ws = _native.workspace("uoc_footprint_workspace_bytes", dev, B, G, A, F, who="footprint", hint=f"B={B} or {placement.grid_hint(G)}")
    fits = torch.empty((B, F, G, G), dtype=torch.int32, device=dev)
    count = torch.empty((B, F, 32), dtype=torch.int32, device=dev)
    best = torch.empty((B, F, 8), dtype=torch.int32, device=dev)
    _native.call("uoc_footprint", dev, st, ow, d2, frame, B, G, _native.host_words(d, 2), A, _native.host_words(r, 8), F,
                 1 if unknown_blocks else 0, fits, count, best, ws, ws.numel())
    return fits, count, best


def rect(length, width, cell_mm, ignore=0, near=None, conservative=True):
    """A rectangle record (HL, HW, ignore, mode, ai, aj, 0, 0).  length, width: metres, used as whole millimetres; HL =
    ceil(length_mm * 128 / cell_mm) in units of 1/256 cell, HW likewise.  conservative=True adds 184 (0.71875 cell) to
    both: every cell the real rectangle touches then has its centre inside the inflated one.  ignore: the id that does
    not block the rectangle (0: none).  near=(i, j) asks for the fitting cell nearest to that cell instead of the
    roomiest one.  ValueError outside the ranges."""
    c = int(cell_mm)
    if c < 1:
        raise ValueError(f"cell_mm = {cell_mm} below 1")
    mm = [int(round(float(v) * 1000)) for v in (length, width)]
    if min(mm) < 0:
        raise ValueError(f"rect: length {length} m or width {width} m is negative")
    HL, HW = (-(-(v * 128) // c) + (INFLATE if conservative else 0) for v in mm)
    ai, aj = (0, 0) if near is None else (int(near[0]), int(near[1]))
    rec = (HL, HW, int(ignore), ROOMIEST if near is None else NEAREST, ai, aj, 0, 0)
    _check_rects([rec])
    return rec


def of_object(fitted, b, a, cell_mm, margin=0.0, **kw):
    """The rectangle of object a in frame b of a support.fit_plane result: its two in-plane half extents (half[b, a, :2],
    the longer one as the length) plus `margin` metres on every side, and ignore = a, so that the object does not block
    its own footprint.  One small host read.  kw goes to rect."""
    h = [float(x) for x in fitted.half[b, a, :2].cpu().tolist()]
    if not all(np.isfinite(h)):
        raise ValueError(f"of_object: object {a} of frame {b} has no extents")
    return rect(2 * max(h) + 2 * float(margin), 2 * min(h) + 2 * float(margin), cell_mm, ignore=int(a), **kw)


def fit(placed, rects, angles=16, unknown_blocks=None) -> FootprintResult:
    """placed: the result of placement.free_space.  rects: one record or a sequence of up to 8 from rect() / of_object().
    angles: orientations over half a turn, 1..32.  unknown_blocks: whether an unknown cell blocks a footprint; None takes
    placed.unknown_blocks.  Returns a FootprintResult."""
    dirs = direction_table(angles)
    r = _check_rects(rects)
    ub = bool(placed.unknown_blocks if unknown_blocks is None else unknown_blocks)
    fits, count, best = footprint_records(placed.state, placed.owner, placed.dist2, getattr(placed, "frame", None), dirs, r, ub)
    return FootprintResult(fits=fits, count=count, best=best, dirs=dirs, rects=r, angles=len(dirs), unknown_blocks=ub,
                           grid=placed.grid, cell_mm=placed.cell_mm, planes=placed.planes)


# ---- host helpers -----------------------------------------------------------------------------------------------------
def fits_mask(result, f, k=None):
    """[B,G,G] bool on the device: the cells where rectangle f fits along direction k, or along any when k is None."""
    w = result.fits[:, f]
    if k is None:
        return w != 0
    if not 0 <= int(k) < result.angles:
        raise ValueError(f"fits_mask: direction {k} outside 0..{result.angles - 1}")
    return (w >> int(k)) & 1 != 0


def pose(result, b, f):
    """The best pose of rectangle f in frame b as a FootprintPose: `center`, the winning cell's centre on the plane, and
    `axis`, the rectangle's long axis as a unit vector, both in camera coordinates (float64 on the host from the plane
    record, like placement.cell_to_camera and grasp.pose); `k` and `angle` = pi k / A; `cell` (i, j) and `dist2`.  None
    without a pose."""
    rec = [int(x) for x in result.best[b, f].cpu().tolist()]
    if not rec[0]:
        return None
    i, j, k = rec[1:4]
    cx, cy = (float(x) for x in result.dirs[k])
    n, c, u, v = placement.plane_axes(result.planes, b)
    center = placement.grid_point(c, u, v, result.grid, result.cell_mm, i + 0.5, j + 0.5)
    axis = cx * u + cy * v
    n = n / np.linalg.norm(n)
    axis = axis - (axis @ n) * n                                               # the record is float32: u.n is not exactly 0
    axis = axis / np.linalg.norm(axis)
    return FootprintPose(center, axis, k, np.pi * k / result.angles, (i, j), rec[4])


def mask_offsets(dirs, k, HL, HW):
    """The offsets (di, dj) of the mask M of a rectangle with half extents HL, HW (1/256 cell) along direction k of
    `dirs`: the cells, relative to the centre, that have to be free.  An [n,2] int32 array in row-major order."""
    cx, cy = int(dirs[k][0]), int(dirs[k][1])
    HL, HW = int(HL), int(HW)
    w = _radius(HL, HW) + 1
    di, dj = np.meshgrid(np.arange(-w, w + 1, dtype=np.int64), np.arange(-w, w + 1, dtype=np.int64), indexing="ij")
    keep = (np.abs(di * cx + dj * cy) <= 64 * HL) & (np.abs(-di * cy + dj * cx) <= 64 * HW)
    return np.stack([di[keep], dj[keep]], axis=1).astype(np.int32)
