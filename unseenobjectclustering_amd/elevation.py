"""How high the scene is, cell by cell: object tops and stacking spots on the table grid, on the device (uoc_elevation,
include/uoc_hip.h).

    placed = placement.free_space(refined, xyz, fitted)        # the grid of §15: 256 x 256 cells of 1 cm
    res = heights(refined, xyz, placed)                        # the same cells: placed.frame, grid, cell_mm, tau_mm
    res.elev[b], res.owner[b]                                  # mm above the plane of the highest point (ELEV_NONE: no point); its id
    res.dist2[b]                                               # clearance^2 in cells to the nearest cell that is not level
    res.tops[b, a]                                             # (cells, level, i, j, dist2, elev_at, elev_max, elev_mean) of id a
    q = [on_top(res, 0.03), on_top(res, 0.03, id=2, hmin=0.05)]
    res = heights(refined, xyz, placed, queries=q)             # res.answers[b, k] = (i, j, dist2, ok)
    spot(res, 0, 2)                                            # the widest level spot on object 2: cell, clearance, height, xyz

Every valid point is projected into the plane's integer frame as in §15 and lands in one cell; a cell's elevation is the
height of its highest point in whole millimetres and its owner that point's id (0: the table and whatever is
unlabelled).  A cell is solid when `min_pts` of its points lie within `step` of its top (a lone mixed pixel above a
surface makes no top), and level when it and its four edge neighbours are solid, have one owner and differ by at most
`step` in elevation.  dist2 is the exact squared Euclidean distance, in cells, to the nearest cell that is not level.
Integer arithmetic in HIP kernels: defined exactly, independent of launch order and batch.  `heights` neither copies to
the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _native, placement

NUM_IDS = 128
ELEV_NONE = _native.ELEV_NONE
ANY_OBJECT = -1
TOPS_FIELDS = ("cells", "level", "i", "j", "dist2", "elev_at", "elev_max", "elev_mean")
INFO_FIELDS = ("found", "outside", "known", "solid")
_BAND = (-32768, 32767)

Spot = collections.namedtuple("Spot", "cell clearance_m height_m xyz")


class ElevationResult(_native.Fields):
    """Device tensors.  elev, owner, pts, near, dist2: [B,G,G] int32; tops [B,128,8] int32 (TOPS_FIELDS per id); info [B,4]
    int32 (INFO_FIELDS); answers [B,Q,4] int32, one (i, j, dist2, ok) per query, (-1, -1, 0, 0) without a candidate; frame
    [B,16] int64, the integer frame records used (placement.FRAME_FIELDS)."""


def elevation_records(labels, xyz, frame, grid, cell_mm, tau_mm, step_mm, min_pts, queries=()):
    """The raw uoc_elevation call: (elev, owner, pts, near, dist2 [B,G,G] int32, tops [B,128,8] int32, info [B,4] int32,
    answers [B,Q,4] int32), on the device, no synchronisation.  labels int32 [B,H,W], xyz float32 [B,3,H,W], frame int64
    [B,16] contiguous on one GPU; queries: a sequence of (need2, id, hmin_mm, hmax_mm) integers."""
    B, H, W = (int(v) for v in labels.shape)
    G, Q = int(grid), len(queries)
    dev = labels.device
    ws = _native.workspace("uoc_elevation_workspace_bytes", dev, B, H, W, G, who="heights", hint=f"B={B} H={H} W={W} or {placement.grid_hint(G)}")
    elev, owner, pts, near, dist2 = (torch.empty((B, G, G), dtype=torch.int32, device=dev) for _ in range(5))
    tops = torch.empty((B, NUM_IDS, 8), dtype=torch.int32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    answers = torch.empty((B, Q, 4), dtype=torch.int32, device=dev)
    _native.call("uoc_elevation", dev, labels, xyz, frame, B, H, W, G, int(cell_mm), int(tau_mm), int(step_mm), int(min_pts),
                 _native.host_words(queries, 4) if Q else None, Q, elev, owner, pts, near, dist2, tops, info,
                 answers if Q else None, ws, ws.numel())
    return elev, owner, pts, near, dist2, tops, info, answers


def _check_queries(queries):
    qs = [tuple(int(x) for x in q) for q in (queries or ())]
    if len(qs) > _native.ELEV_MAX_QUERIES:
        raise ValueError(f"{len(qs)} queries, at most {_native.ELEV_MAX_QUERIES}")
    for q in qs:
        if len(q) != 4 or not 0 <= q[0] <= 1 << 30 or not -1 <= q[1] < NUM_IDS \
                or not all(_BAND[0] <= h <= _BAND[1] for h in q[2:4]):
            raise ValueError(f"query {q}: (need2 in 0..2^30, id in -1..127, hmin_mm, hmax_mm in -32768..32767)")
    return qs


def heights(labels, xyz, placed, step=0.005, min_pts=2, queries=None) -> ElevationResult:
    """labels: device tensor [B,H,W] or [H,W] of int32 / int64 / float ids; xyz: [B,3,H,W] or [3,H,W] float metres
    (sample['depth']).  placed: the result of placement.free_space on the same frames; its frame records (read in place
    on the device), grid, cell_mm and tau_mm are used, so that the two grids coincide cell for cell.  step: metres, used
    in whole millimetres (1..1000); min_pts in 1..65535; queries: up to 16 (need2, id, hmin_mm, hmax_mm) from on_top().
    Returns an ElevationResult."""
    step_mm = placement.millimetres(step, "step")
    placement.check_min_pts(min_pts)
    qs = _check_queries(queries)
    G, cell_mm, tau_mm = placement.check_grid(int(placed.grid)), int(placed.cell_mm), int(placed.tau_mm)
    for mm, name in ((cell_mm, "cell_mm"), (tau_mm, "tau_mm")):
        if not 1 <= mm <= _native.PLACE_MAX_MM:
            raise ValueError(f"{name} = {mm} outside 1..{_native.PLACE_MAX_MM} mm")
    labels, xyz = _native.frame_inputs("heights", labels, xyz)
    B = int(labels.shape[0])
    frame = getattr(placed, "frame", None)
    if not _native.on_gpu(frame) or frame.device != labels.device or frame.dtype != torch.int64 or tuple(frame.shape) != (B, 16):
        raise _native.NativeError(f"heights: the frame records of `placed` do not match the {B} frames on {labels.device}")
    frame = frame.contiguous()
    elev, owner, pts, near, dist2, tops, info, answers = elevation_records(
        labels, xyz, frame, G, cell_mm, tau_mm, step_mm, int(min_pts), qs)
    return ElevationResult(elev=elev, owner=owner, pts=pts, near=near, dist2=dist2, tops=tops, info=info, answers=answers,
                           frame=frame, queries=qs, grid=G, cell_mm=cell_mm, tau_mm=tau_mm, step_mm=step_mm, min_pts=int(min_pts))


# ---- host helpers -----------------------------------------------------------------------------------------------------
def _band_mm(value, default, name):
    if value is None:
        return default
    mm = int(round(float(value) * 1000))
    if not _BAND[0] <= mm <= _BAND[1]:
        raise ValueError(f"on_top: {name} = {value} m is {mm} mm, outside {_BAND[0]}..{_BAND[1]} mm")
    return mm


def on_top(result, radius, id=ANY_OBJECT, hmin=None, hmax=None):
    """The query "the level cell with the most room on object `id`" (-1: on any object, never the table; 0: the table),
    with its elevation in hmin..hmax metres (None: no bound), ok when a disc of `radius` metres fits there."""
    a = int(id)
    if not -1 <= a < NUM_IDS:
        raise ValueError(f"on_top: id = {id} outside -1..{NUM_IDS - 1}")
    return (placement.need2(radius, result.cell_mm / 1000.0), a, _band_mm(hmin, _BAND[0], "hmin"), _band_mm(hmax, _BAND[1], "hmax"))


def cell_to_camera(result, b, i, j, h_mm=0):
    """The centre of cell (i, j) of frame b lifted h_mm millimetres off the plane along its normal, in camera coordinates
    (metres): qc + a U + b V + h N, float64 on the host from the integer frame record."""
    F = np.asarray(result.frame[b].cpu().tolist(), np.float64)
    S = float(_native.PLACE_SCALE)
    n, u, v, c = F[0:3] / S, F[4:7] / S, F[7:10] / S, F[10:13] / 1000.0
    n = n / np.linalg.norm(n)
    return placement.grid_point(c, u, v, result.grid, result.cell_mm, int(i) + 0.5, int(j) + 0.5) + float(h_mm) / 1000.0 * n


def spot(result, b, a):
    """The widest level spot on top of id a in frame b as a Spot: `cell` (i, j), `clearance_m` (the distance to the
    nearest cell that is not level), `height_m` (the elevation there) and `xyz`, the cell's centre lifted by that
    elevation along the normal, camera coordinates; None when the id has no level cell."""
    row = [int(x) for x in result.tops[b, a].cpu().tolist()]
    if row[1] == 0:
        return None
    cell = result.cell_mm / 1000.0
    return Spot((row[2], row[3]), float(np.sqrt(row[4])) * cell, row[5] / 1000.0, cell_to_camera(result, b, row[2], row[3], row[5]))


def level_mask(result, radius):
    """[B,G,G] bool on the device: the level cells where a disc of `radius` metres fits."""
    return result.dist2 >= max(1, placement.need2(radius, result.cell_mm / 1000.0))
