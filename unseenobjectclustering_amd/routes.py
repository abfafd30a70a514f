"""Can it get from here to there without being lifted over its neighbours, and along which cells: shortest slide paths
of a disc on the table grid, on the device (uoc_routes, include/uoc_hip.h).

    placed = placement.free_space(refined, xyz, fitted)          # the top-down grid of §15, on the GPU
    q = query(0.04, (120, 40), (60, 200), placed.cell_mm)        # a 4 cm disc from cell (120, 40) to cell (60, 200)
    res = plan(placed, [q, of_object(placed, fitted, 0, 3, (60, 200))])
    res.cost[b, q]                                               # [G,G] int32: the least cost from the source, -1: not reached
    res.info[b, q]                                               # (src_ok, ok, ci, cj, cost, steps, reached, passable)
    reachable_mask(res, 0)                                       # [B,G,G] bool on the device
    waypoints(res, 0, 0), length_m(res, 0, 0)                    # the cells from source to goal; the path's length in metres
    path_to_camera(res, 0, 0)                                    # [n,3] float64, camera coordinates

A cell is passable when the disc, centred on it, lies wholly on free cells: table, unknown when `unknown_blocks` is off,
or part of the object `ignore` (the object being moved does not block itself).  Moves go to the eight neighbours, 5 per
orthogonal and 7 per diagonal step, never across a blocked corner; a cost is a chamfer length: cost / 5 cells is 0.99 to
1.08 times the Euclidean length.  Integer arithmetic in HIP kernels: defined exactly, independent of launch order and
batch.  `plan` neither copies to the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _native
from . import placement as _placement

INFO_FIELDS = ("src_ok", "ok", "ci", "cj", "cost", "steps", "reached", "passable")
COST_ORTH, COST_DIAG = 5, 7
Waypoints = namedtuple("Waypoints", "cells truncated reached_target cost")


class RoutesResult(_native.Fields):
    """Device tensors.  cost [B,Q,G,G] int32: the least cost from the source of query q, -1 where the cell is not passable
    or not reached; info [B,Q,8] int32: INFO_FIELDS per query; path [B,Q,max_path,2] int32: the cells from the
    closest-approach cell back to the source, (-1, -1) past the end.  queries: the records [Q,8] (host, numpy).  grid,
    cell_mm, planes: of the placement result the grids came from."""


def _check_queries(queries, G=None):
    q = np.asarray(queries, dtype=np.int64)
    if q.ndim == 1 and q.size == 8:
        q = q[None]
    if q.ndim != 2 or q.shape[1] != 8:
        raise ValueError(f"queries has shape {q.shape}, not [Q,8]")
    if not 1 <= len(q) <= _native.ROUTES_MAX_QUERIES:
        raise ValueError(f"{len(q)} queries, outside 1..{_native.ROUTES_MAX_QUERIES}")
    lim = _native.PLACE_MAX_GRID if G is None else G
    for n, (need2, si, sj, ti, tj, ignore, z6, z7) in enumerate(q.tolist()):
        if not 0 <= need2 <= _native.ROUTES_MAX_NEED2:
            raise ValueError(f"query {n}: need2 = {need2} outside 0..{_native.ROUTES_MAX_NEED2}")
        if not (0 <= si < lim and 0 <= sj < lim):
            raise ValueError(f"query {n}: the source {(si, sj)} lies outside the grid of {lim} cells")
        if not ((ti, tj) == (-1, -1) or (0 <= ti < lim and 0 <= tj < lim)):
            raise ValueError(f"query {n}: the target {(ti, tj)} is neither inside the grid of {lim} cells nor (-1, -1)")
        if not (0 <= ignore < 128 and z6 == 0 and z7 == 0):
            raise ValueError(f"query {n}: (ignore in 0..127, two zero words), not {(ignore, z6, z7)}")
    return np.ascontiguousarray(q.astype(np.int32))


def _call(state, owner, frame, queries, unknown_blocks, max_path):
    """uoc_routes; returns (cost, info, path, workspace).  The workspace's first B*Q int32 words are the sweeps taken."""
    st, ow = _native.grid_inputs("routes", state, owner)
    B, G = int(st.shape[0]), int(st.shape[1])
    dev = st.device
    if frame is not None:
        if not (isinstance(frame, torch.Tensor) and frame.device == dev and frame.dtype == torch.int64 and tuple(frame.shape) == (B, 16)):
            raise _native.NativeError(f"routes: the frame records do not match the {B} frames on {dev}")
        frame = frame.contiguous()
    P = int(max_path)
    if not 1 <= P <= _native.ROUTES_MAX_PATH:
        raise ValueError(f"max_path = {max_path} outside 1..{_native.ROUTES_MAX_PATH}")
    _native.workspace("uoc_routes_workspace_bytes", dev, B, G, 1, who="routes", hint=f"B={B} or {_placement.grid_hint(G)}")    # the shape, before the queries
    q = _check_queries(queries, G)
    Q = len(q)
    ws = _native.workspace("uoc_routes_workspace_bytes", dev, B, G, Q, who="routes", hint=f"B={B} or {_placement.grid_hint(G)}")
    cost = torch.empty((B, Q, G, G), dtype=torch.int32, device=dev)
    info = torch.empty((B, Q, 8), dtype=torch.int32, device=dev)
    path = torch.empty((B, Q, P, 2), dtype=torch.int32, device=dev)
    _native.call("uoc_routes", dev, st, ow, frame, B, G, _native.host_words(q, 8), Q, 1 if unknown_blocks else 0, P, cost, info, path,
                 ws, ws.numel())
    return cost, info, path, ws


def routes_records(state, owner, frame, queries, unknown_blocks, max_path=1024):
    """The raw uoc_routes call on bare grids: (cost [B,Q,G,G], info [B,Q,8], path [B,Q,max_path,2]) int32 on the device, no
    synchronisation.  state, owner: device tensors [B,G,G] or [G,G] of any integer type and layout (they are made int32 and
    contiguous); frame: [B,16] int64 on the device, or None; queries: [Q,8] records."""
    return _call(state, owner, frame, queries, unknown_blocks, max_path)[:3]


def query(radius_m, src, dst, cell_mm, ignore=0):
    """A query record (need2, si, sj, ti, tj, ignore, 0, 0).  radius_m: the travelling disc's radius in metres, need2 by
    the rule of placement.need2; src = (i, j), the source cell; dst = (i, j), the target cell, or None for the whole field
    without a target; ignore: the id that does not block (0: none).  ValueError outside the ranges."""
    c = int(cell_mm)
    if c < 1:
        raise ValueError(f"cell_mm = {cell_mm} below 1")
    n2 = _placement.need2(radius_m, c / 1000.0)
    ti, tj = (-1, -1) if dst is None else (int(dst[0]), int(dst[1]))
    if dst is not None and (ti < 0 or tj < 0):
        raise ValueError(f"query: the target {(ti, tj)} lies outside the grid")
    rec = (n2, int(src[0]), int(src[1]), ti, tj, int(ignore), 0, 0)
    _check_queries([rec])
    return rec


def plan(placed, queries, unknown_blocks=None, max_path=1024) -> RoutesResult:
    """placed: the result of placement.free_space.  queries: one record or a sequence of up to 8 from query() /
    of_object().  unknown_blocks: whether an unknown cell blocks the way; None takes placed.unknown_blocks.  max_path: the
    cells kept per path, 1..4096.  Returns a RoutesResult."""
    q = _check_queries(queries, int(placed.grid))
    ub = bool(placed.unknown_blocks if unknown_blocks is None else unknown_blocks)
    cost, info, path = routes_records(placed.state, placed.owner, getattr(placed, "frame", None), q, ub, max_path)
    return RoutesResult(cost=cost, info=info, path=path, queries=q, unknown_blocks=ub, max_path=int(max_path), grid=placed.grid,
                        cell_mm=placed.cell_mm, planes=placed.planes)


def of_object(placed, fitted, b, a, dst, radius_m=None, margin=0.0):
    """The query that slides object a of frame b to the cell dst (None: no target): the source is the cell of the object's
    centre (fitted.center, through placement.camera_to_cell), the radius half the object's longer in-plane extent plus
    `margin` metres unless radius_m is given, and ignore = a.  One small host read."""
    rec = [float(x) for x in torch.cat([fitted.center[b, a], fitted.half[b, a, :2]]).cpu().tolist()]
    if not all(np.isfinite(rec)):
        raise ValueError(f"of_object: object {a} of frame {b} has no extents")
    cell = _placement.camera_to_cell(placed, b, rec[:3])
    if cell is None or not all(0 <= c < placed.grid for c in cell):
        raise ValueError(f"of_object: the centre of object {a} of frame {b} has no cell on the grid ({cell})")
    r = max(rec[3:]) + float(margin) if radius_m is None else float(radius_m)
    return query(r, cell, dst, placed.cell_mm, ignore=int(a))


# ---- host helpers -----------------------------------------------------------------------------------------------------
def reachable_mask(result, q):
    """[B,G,G] bool on the device: the cells the disc of query q can reach from its source."""
    return result.cost[:, q] >= 0


def waypoints(result, b, q):
    """The path of query q in frame b as Waypoints: `cells`, an [n,2] int32 array from the source to the goal (the
    closest-approach cell; the device order flipped); `truncated`, set when steps >= max_path, in which case the cells
    nearest to the source are missing; `reached_target` and the goal's `cost`.  None without a path.  One host read."""
    rec = [int(x) for x in result.info[b, q].cpu().tolist()]
    if not rec[0] or rec[2] < 0:
        return None
    steps = rec[5]
    n = min(steps, result.max_path - 1) + 1
    cells = result.path[b, q, :n].cpu().numpy()[::-1].copy()
    return Waypoints(cells, steps >= result.max_path, bool(rec[1]), rec[4])


def length_m(result, b, q):
    """The chamfer length in metres of the path of query q in frame b: cost * cell_mm / 5000.  None without a path."""
    rec = [int(x) for x in result.info[b, q].cpu().tolist()]
    if not rec[0] or rec[2] < 0:
        return None
    return rec[4] * result.cell_mm / (COST_ORTH * 1000.0)


def path_to_camera(result, b, q):
    """[n,3] float64: the centres of the waypoints' cells on the plane, camera coordinates, through
    placement.cell_to_camera.  None without a path."""
    w = waypoints(result, b, q)
    if w is None:
        return None
    _, c, u, v = _placement.plane_axes(result.planes, b)
    return np.array([_placement.grid_point(c, u, v, result.grid, result.cell_mm, i + 0.5, j + 0.5) for i, j in w.cells.tolist()],
                    np.float64).reshape(len(w.cells), 3)
