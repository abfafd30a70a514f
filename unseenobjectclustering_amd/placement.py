"""Where an object can be put down: the free space on the support plane, on the device (uoc_placement,
include/uoc_hip.h).

    fitted = support.fit_plane(refined, xyz)          # labels [B,H,W] / [H,W] on the GPU, xyz = sample['depth'] [B,3,H,W]
    res = free_space(refined, xyz, fitted)            # a 256 x 256 grid of 1 cm cells in the plane's axes u, v
    res.state[b], res.owner[b], res.dist2[b]          # 0 unknown / 1 table / 2 obstacle; the obstacle's id; clearance^2 in cells
    q = [widest(res, 0.05), nearest(res, 0.05, fitted.center[0, 3].tolist())]
    res = free_space(refined, xyz, fitted, queries=q) # res.answers[b, k] = (i, j, dist2, ok)
    cell_to_camera(res, 0, i, j)                      # the cell's centre on the plane, camera coordinates, metres

Every valid point is projected into the plane's frame in integers (millimetres, the plane's vectors in units of 2^-14)
and lands in one cell: labelled points and points higher than `h_obs` above the plane are obstacles, points within
`tau` of the plane are table, points more than `tau` below it (the floor past the table's edge) are ignored.  A cell
with `min_pts` obstacle points is an obstacle, else with `min_pts` table points table, else unknown (an occlusion
shadow, a depth hole, past the edge).  dist2 is the exact squared Euclidean distance, in cells, to the nearest blocking
cell: an obstacle, an unknown cell when `unknown_blocks`, or anything outside the grid.  Integer arithmetic in HIP
kernels: defined exactly, independent of launch order and batch.  `free_space` neither copies to the host nor
synchronises.  No CPU fallback."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native

NUM_IDS = 128
WIDEST, NEAREST = _native.PLACE_WIDEST, _native.PLACE_NEAREST
_PLANE_WORDS = ctypes.sizeof(_native.UocPlane) // 4
_OFF = {name: getattr(_native.UocPlane, name).offset // 4 for name, _ in _native.UocPlane._fields_}
FRAME_FIELDS = {"N": slice(0, 3), "D": 3, "U": slice(4, 7), "V": slice(7, 10), "qc": slice(10, 13), "found": 13}


class PlacementResult(_native.Fields):
    """Device tensors.  state, owner, dist2: [B,G,G] int32; cells [B,128] int32 (obstacle cells per owner id 1..127; word 0
    is the frame's `outside` counter); outside [B] int32; frame [B,16] int64 (FRAME_FIELDS); answers [B,Q,4] int32, one
    (i, j, dist2, ok) per query, (-1, -1, 0, 0) without a candidate; planes [B,21] int32, the uoc_plane records used."""


def pack_planes(normal, d, centroid, u, v, frames=None):
    """uoc_plane records [B,21] int32 (host) with found = 1 from the plane normal.p + d = 0, a point `centroid` on it and
    the in-plane axes u, v; arrays [B,3] / [3] and d [B] / scalar, metres, rounded to float32."""
    vec = [np.asarray(torch.as_tensor(a).detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).reshape(-1, 3)
           for a in (normal, centroid, u, v)]
    dd = np.asarray(d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else d, np.float32).reshape(-1)
    B = frames if frames is not None else max(len(a) for a in vec + [dd])
    rec = np.zeros((B, _PLANE_WORDS), np.float32)
    for name, a in zip(("normal", "centroid", "u", "v"), vec):
        if len(a) not in (1, B):
            raise ValueError(f"plane {name}: {len(a)} rows for {B} frames")
        rec[:, _OFF[name]:_OFF[name] + 3] = a
    if len(dd) not in (1, B):
        raise ValueError(f"plane d: {len(dd)} values for {B} frames")
    rec[:, _OFF["d"]] = dd
    out = rec.view(np.int32)
    out[:, _OFF["found"]] = 1
    return out


def placement_records(labels, xyz, planes, grid, cell_mm, h_obs_mm, tau_mm, min_pts, unknown_blocks, queries=()):
    """The raw uoc_placement call: (state, owner, dist2 [B,G,G] int32, counts [B,128] int32, frame [B,16] int64, answers
    [B,Q,4] int32), on the device, no synchronisation.  labels int32 [B,H,W], xyz float32 [B,3,H,W], planes int32 [B,21]
    contiguous on one GPU; queries: a sequence of (need2, ai, aj, mode) integers."""
    B, H, W = (int(v) for v in labels.shape)
    G, Q = int(grid), len(queries)
    dev = labels.device
    ws = _native.workspace("uoc_placement_workspace_bytes", dev, B, H, W, G, who="free_space", hint=f"B={B} H={H} W={W} or {grid_hint(G)}")
    state, owner, dist2 = (torch.empty((B, G, G), dtype=torch.int32, device=dev) for _ in range(3))
    counts = torch.empty((B, NUM_IDS), dtype=torch.int32, device=dev)
    frame = torch.empty((B, 16), dtype=torch.int64, device=dev)
    answers = torch.empty((B, Q, 4), dtype=torch.int32, device=dev)
    _native.call("uoc_placement", dev, labels, xyz, planes, B, H, W, G, int(cell_mm), int(h_obs_mm), int(tau_mm), int(min_pts),
                 int(unknown_blocks), _native.host_words(queries, 4) if Q else None, Q, state, owner, dist2, counts, frame,
                 answers if Q else None, ws, ws.numel())
    return state, owner, dist2, counts, frame, answers


# ---- the range checks every table-grid stage shares -----------------------------------------------------------------
def check_grid(grid) -> int:
    G = int(grid)
    if not (8 <= G <= _native.PLACE_MAX_GRID and G % 8 == 0):
        raise ValueError(f"grid = {grid} is not a multiple of 8 in 8..{_native.PLACE_MAX_GRID}")
    return G


def grid_hint(G) -> str:
    """How a *_workspace_bytes of 0 names the grid in the stage's NativeError."""
    return f"grid={G} (a multiple of 8 in 8..{_native.PLACE_MAX_GRID})"


def check_min_pts(min_pts) -> int:
    if not 1 <= int(min_pts) <= _native.PLACE_MAX_MIN_PTS:
        raise ValueError(f"min_pts = {min_pts} outside 1..{_native.PLACE_MAX_MIN_PTS}")
    return int(min_pts)


def millimetres(value, name, lo=1, hi=_native.PLACE_MAX_MM) -> int:
    """Metres -> whole millimetres in lo..hi."""
    mm = int(round(float(value) * 1000))
    if not lo <= mm <= hi:
        raise ValueError(f"{name} = {value} m is {mm} mm, outside {lo}..{hi} mm")
    return mm


def _check_queries(queries):
    qs = [tuple(int(x) for x in q) for q in (queries or ())]
    if len(qs) > _native.PLACE_MAX_QUERIES:
        raise ValueError(f"{len(qs)} queries, at most {_native.PLACE_MAX_QUERIES}")
    for q in qs:
        if len(q) != 4 or not 0 <= q[0] <= 1 << 30 or q[3] not in (WIDEST, NEAREST) \
                or not all(-_native.PLACE_MAX_ANCHOR <= a < _native.PLACE_MAX_ANCHOR for a in q[1:3]):
            raise ValueError(f"query {q}: (need2 in 0..2^30, ai, aj in -4096..4095, mode 0 or 1)")
    return qs


def free_space(labels, xyz, plane, grid=256, cell=0.010, h_obs=0.010, tau=0.010, min_pts=1, unknown_blocks=True,
               queries=None) -> PlacementResult:
    """labels: device tensor [B,H,W] or [H,W] of int32 / int64 / float ids; xyz: [B,3,H,W] or [3,H,W] float metres
    (sample['depth']).  plane: the result of support.fit_plane on the same frames (its device records are read in place),
    or a tuple (normal, d, centroid, u, v) that is packed into records.  grid: cells per side, a multiple of 8 in 8..512;
    cell, h_obs, tau: metres, used in whole millimetres (cell, tau in 1..1000, h_obs in 0..1000); min_pts in 1..65535;
    queries: up to 16 (need2, ai, aj, mode) from widest() / nearest().  Returns a PlacementResult."""
    G = check_grid(grid)
    cell_mm, h_obs_mm, tau_mm = millimetres(cell, "cell"), millimetres(h_obs, "h_obs", 0), millimetres(tau, "tau")
    check_min_pts(min_pts)
    qs = _check_queries(queries)
    labels, xyz = _native.frame_inputs("free_space", labels, xyz)
    B = int(labels.shape[0])
    if isinstance(plane, (tuple, list)):
        planes = torch.from_numpy(pack_planes(*plane, frames=B)).to(labels.device)
    else:
        planes = getattr(plane, "records", None)
        if planes is None:
            raise _native.NativeError("free_space: plane is neither a fit_plane result nor (normal, d, centroid, u, v)")
    if not _native.on_gpu(planes) or planes.device != labels.device or planes.dtype != torch.int32 \
            or tuple(planes.shape) != (B, _PLANE_WORDS):
        raise _native.NativeError(f"free_space: the plane records do not match the {B} frames on {labels.device}")
    state, owner, dist2, counts, frame, answers = placement_records(
        labels, xyz, planes.contiguous(), G, cell_mm, h_obs_mm, tau_mm, int(min_pts),
        1 if unknown_blocks else 0, qs)
    return PlacementResult(state=state, owner=owner, dist2=dist2, cells=counts, outside=counts[:, 0], frame=frame,
                           answers=answers, planes=planes, queries=qs, grid=G, cell_mm=cell_mm, h_obs_mm=h_obs_mm,
                           tau_mm=tau_mm, min_pts=int(min_pts), unknown_blocks=bool(unknown_blocks))


# ---- host helpers -----------------------------------------------------------------------------------------------------
def need2(radius_m, cell_m):
    """The squared clearance, in cells, that a disc of `radius_m` metres needs on a grid of `cell_m` cells: k*k with
    k = ceil(radius / cell) + 1 in whole millimetres.  Conservative: what makes a cell blocking lies within 0.71 cells of
    its centre."""
    r_mm, c_mm = int(round(float(radius_m) * 1000)), int(round(float(cell_m) * 1000))
    if r_mm < 0 or c_mm < 1:
        raise ValueError(f"need2: radius {radius_m} m, cell {cell_m} m")
    k = -(-r_mm // c_mm) + 1
    return k * k


def widest(result, radius):
    """The query "the table cell with the most room", ok when a disc of `radius` metres fits there."""
    return (need2(radius, result.cell_mm / 1000.0), 0, 0, WIDEST)


def nearest(result, radius, anchor_xyz, b=0):
    """The query "the table cell nearest to `anchor_xyz` (camera coordinates, metres; for instance an object's
    `center`) where a disc of `radius` metres fits", in frame b's grid."""
    cell = camera_to_cell(result, b, anchor_xyz)
    if cell is None:
        raise ValueError(f"nearest: frame {b} has no plane, or the anchor is not a valid point")
    lim = _native.PLACE_MAX_ANCHOR
    if not all(-lim <= c < lim for c in cell):
        raise ValueError(f"nearest: the anchor's cell {cell} lies outside -{lim}..{lim - 1}")
    return (need2(radius, result.cell_mm / 1000.0), cell[0], cell[1], NEAREST)


def camera_to_cell(result, b, xyz):
    """The cell (i, j) of a camera-frame point by the integer rule of the kernels (it may lie outside the grid), or None
    when frame b has no plane or the point is not a valid one (not finite, z <= 0 or beyond 32.767 m)."""
    F = [int(x) for x in result.frame[b].cpu().tolist()]
    p = np.asarray(xyz, np.float32).reshape(3)
    if not F[FRAME_FIELDS["found"]] or not np.isfinite(p).all() or not p[2] > 0:
        return None
    q = [int(x) for x in np.rint(p * np.float32(1000.0))]
    if max(abs(x) for x in q) > 32767:
        return None
    div = result.cell_mm * _native.PLACE_SCALE
    a = sum(F[4 + k] * (q[k] - F[10 + k]) for k in range(3))
    bv = sum(F[7 + k] * (q[k] - F[10 + k]) for k in range(3))
    return a // div + result.grid // 2, bv // div + result.grid // 2


def plane_axes(planes, b):
    """(normal, centroid, u, v) of frame b: float64 [3] each on the host, from uoc_plane records [B,21] int32 (a tensor on
    any device or a numpy array).  One small host read."""
    rec = planes[b]
    rec = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    p = np.ascontiguousarray(rec).view(np.float32).astype(np.float64)
    return tuple(p[_OFF[k]:_OFF[k] + 3] for k in ("normal", "centroid", "u", "v"))


def grid_point(origin, u, v, grid, cell_mm, a, b):
    """The point of the plane at the grid coordinates (a, b), in cells and fractions of one: origin + (a - G/2) cell u +
    (b - G/2) cell v.  Cell (i, j) spans [i, i+1) x [j, j+1): its centre is (i + 0.5, j + 0.5)."""
    cell = cell_mm / 1000.0
    return origin + (a - grid // 2) * cell * u + (b - grid // 2) * cell * v


def cell_to_camera(result, b, i, j):
    """The centre of cell (i, j) of frame b on the plane, in camera coordinates (metres): centroid + a u + b v, float64
    on the host from the plane record."""
    _, c, u, v = plane_axes(result.planes, b)
    return grid_point(c, u, v, result.grid, result.cell_mm, int(i) + 0.5, int(j) + 0.5)


def free_mask(result, radius):
    """[B,G,G] bool on the device: the table cells where a disc of `radius` metres fits."""
    return (result.state == 1) & (result.dist2 >= need2(radius, result.cell_mm / 1000.0))
