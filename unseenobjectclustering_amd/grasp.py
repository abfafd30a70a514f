"""How to take hold of an object: parallel-jaw grasp candidates on the table grid, on the device (uoc_grasp,
include/uoc_hip.h).

    placed = placement.free_space(refined, xyz, fitted)          # the top-down grid of §15, on the GPU
    res = candidates(placed)                                     # 16 closing directions x 5 lateral offsets per object
    res.best[b, a]                                               # (ok, k, m, tlo, w, ax, ay, n_ok) of id a
    res.cand[b, a, k, m + res.offsets]                           # (code, tlo): w > 0, or MISS / WIDE / PINCHED / BLOCKED
    graspable(res)                                               # [B,128] bool on the device
    pose(res, 0, a)                                              # centre, closing axis, width and opening in metres

A top-down grasp closes along a direction in the plane.  For every object the strip under the gripper's pads is sampled
through the object's centroid (and `offsets` cells to either side of it) along `angles` directions: how wide the object is
there (`w` cells), whether another object or the grid's border lies between the fingers (PINCHED), whether both fingers,
`finger` thick and `gap` away from the object, land on free table (else BLOCKED), whether the opening `max_open` suffices
(else WIDE).  Integer arithmetic in HIP kernels: defined exactly, independent of launch order and batch.  `candidates`
neither copies to the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _native, placement

NUM_IDS = 128
MISS, WIDE, PINCHED, BLOCKED = _native.GRASP_MISS, _native.GRASP_WIDE, _native.GRASP_PINCHED, _native.GRASP_BLOCKED
BEST_FIELDS = ("ok", "k", "m", "tlo", "w", "ax", "ay", "n_ok")
GraspPose = namedtuple("GraspPose", "center axis width_m opening_m k m")


class GraspResult(_native.Fields):
    """Device tensors.  cand [B,128,A,2M+1,2] int32: (code, tlo) per id, direction k and offset m (index m + M); best
    [B,128,8] int32: BEST_FIELDS per id.  dirs: the direction table [A,2] (host, numpy).  angles, offsets, max_open, gap,
    finger, pad: A, M, Wmax, gap, F, Hp in cells; grid, cell_mm, planes: of the placement result the grids came from."""


def direction_table(angles):
    """The closing directions [A,2] int32: (rint(cos(pi k / A) S), rint(sin(pi k / A) S)), S = 16384, in float64."""
    A = int(angles)
    if not 1 <= A <= _native.GRASP_MAX_DIRS:
        raise ValueError(f"angles = {angles} outside 1..{_native.GRASP_MAX_DIRS}")
    k = np.arange(A, dtype=np.float64)
    S = float(_native.GRASP_SCALE)
    return np.stack([np.rint(np.cos(np.pi * k / A) * S), np.rint(np.sin(np.pi * k / A) * S)], axis=1).astype(np.int32)


def cells_from_metres(cell_mm, max_open, gap, finger, pad):
    """(Wmax, gap, F, Hp) in cells from metres, used as whole millimetres: Wmax = max_open_mm // cell_mm, gap and F =
    ceil(. / cell_mm), Hp = pad_mm // (2 cell_mm).  ValueError when one falls outside its range."""
    c = int(cell_mm)
    if c < 1:
        raise ValueError(f"cell_mm = {cell_mm} below 1")
    mm = {name: int(round(float(v) * 1000)) for name, v in (("max_open", max_open), ("gap", gap), ("finger", finger), ("pad", pad))}
    for name, v in mm.items():
        if v < 0:
            raise ValueError(f"{name} = {v} mm is negative")
    cells = {"max_open": mm["max_open"] // c, "gap": -(-mm["gap"] // c), "finger": -(-mm["finger"] // c), "pad": mm["pad"] // (2 * c)}
    limits = {"max_open": (1, _native.GRASP_MAX_OPEN), "gap": (0, _native.GRASP_MAX_GAP), "finger": (1, _native.GRASP_MAX_FINGER),
              "pad": (0, _native.GRASP_MAX_PAD)}
    for name, (lo, hi) in limits.items():
        if not lo <= cells[name] <= hi:
            raise ValueError(f"{name} = {mm[name]} mm is {cells[name]} cells of {c} mm, outside {lo}..{hi} cells")
    return cells["max_open"], cells["gap"], cells["finger"], cells["pad"]


def _check_cells(A, M, Wmax, gap, F, Hp):
    for name, v, lo, hi in (("angles", A, 1, _native.GRASP_MAX_DIRS), ("offsets", M, 0, _native.GRASP_MAX_OFFSETS),
                            ("max_open", Wmax, 1, _native.GRASP_MAX_OPEN), ("gap", gap, 0, _native.GRASP_MAX_GAP),
                            ("finger", F, 1, _native.GRASP_MAX_FINGER), ("pad", Hp, 0, _native.GRASP_MAX_PAD)):
        if not lo <= v <= hi:
            raise ValueError(f"{name} = {v} outside {lo}..{hi}")


def grasp_records(state, owner, dirs, offsets, max_open, gap, finger, pad, unknown_blocks):
    """The raw uoc_grasp call on bare grids: (cand [B,128,A,2M+1,2], best [B,128,8]) int32 on the device, no
    synchronisation.  state, owner: device tensors [B,G,G] or [G,G] of any integer type and layout (they are made int32
    and contiguous); dirs: [A,2] integers in -S..S; the other parameters in cells."""
    st, ow = _native.grid_inputs("grasp", state, owner)
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.int64))
    if d.ndim != 2 or d.shape[1] != 2:
        raise ValueError(f"dirs has shape {d.shape}, not [A,2]")
    A, M, Wmax, gap, F, Hp = int(d.shape[0]), int(offsets), int(max_open), int(gap), int(finger), int(pad)
    _check_cells(A, M, Wmax, gap, F, Hp)
    if np.abs(d).max() > _native.GRASP_SCALE:
        raise ValueError(f"dirs has a component outside -{_native.GRASP_SCALE}..{_native.GRASP_SCALE}")
    B, G = int(st.shape[0]), int(st.shape[1])
    dev = st.device
    ws = _native.workspace("uoc_grasp_workspace_bytes", dev, B, G, A, M, who="grasp", hint=f"B={B} or {placement.grid_hint(G)}")
    cand = torch.empty((B, NUM_IDS, A, 2 * M + 1, 2), dtype=torch.int32, device=dev)
    best = torch.empty((B, NUM_IDS, 8), dtype=torch.int32, device=dev)
    _native.call("uoc_grasp", dev, st, ow, B, G, _native.host_words(d, 2), A, M, Wmax, gap, F, Hp, 1 if unknown_blocks else 0,
                 cand, best, ws, ws.numel())
    return cand, best


def candidates(placed, angles=16, offsets=2, max_open=0.085, gap=0.005, finger=0.010, pad=0.020, unknown_blocks=None) -> GraspResult:
    """placed: the result of placement.free_space.  angles: closing directions over half a turn, 1..32; offsets: lateral
    offsets to either side of the centroid, in cells, 0..8; max_open, gap, finger, pad: the gripper's largest opening,
    the clearance between a finger and the object, the finger's thickness along the closing direction and the pad's
    length across it, metres (cells_from_metres turns them into cells of placed.cell_mm).  unknown_blocks: whether a
    finger may land on an unknown cell; None takes placed.unknown_blocks.  Returns a GraspResult."""
    dirs = direction_table(angles)
    M = int(offsets)
    if not 0 <= M <= _native.GRASP_MAX_OFFSETS:
        raise ValueError(f"offsets = {offsets} outside 0..{_native.GRASP_MAX_OFFSETS}")
    Wmax, g, F, Hp = cells_from_metres(placed.cell_mm, max_open, gap, finger, pad)
    ub = bool(placed.unknown_blocks if unknown_blocks is None else unknown_blocks)
    cand, best = grasp_records(placed.state, placed.owner, dirs, M, Wmax, g, F, Hp, ub)
    return GraspResult(cand=cand, best=best, dirs=dirs, angles=len(dirs), offsets=M, max_open=Wmax, gap=g, finger=F, pad=Hp,
                       unknown_blocks=ub, grid=placed.grid, cell_mm=placed.cell_mm, planes=placed.planes)


# ---- host helpers -----------------------------------------------------------------------------------------------------
def graspable(result):
    """[B,128] bool on the device: the ids with at least one candidate of positive code."""
    return result.best[:, :, 0] != 0


def pose(result, b, a, k=None, m=None):
    """The grasp of id a in frame b as a GraspPose: `center`, the midpoint between the fingers on the plane, and `axis`,
    the closing direction as a unit vector, both in camera coordinates (float64 on the host from the plane record, like
    placement.cell_to_camera); `width_m`, the object's width between the fingers; `opening_m` = (w + 2 gap) cells, what
    the gripper has to open to.  The best candidate, or candidate (k, m) when both are given.  None when the id has no
    candidate of positive code (or (k, m) is none)."""
    rec = [int(x) for x in result.best[b, a].cpu().tolist()]
    if (k is None) != (m is None):
        raise ValueError("pose: give both k and m, or neither")
    if k is None:
        if not rec[0]:
            return None
        k, m, tlo, w = rec[1:5]
    else:
        k, m = int(k), int(m)
        if not (0 <= k < result.angles and -result.offsets <= m <= result.offsets):
            raise ValueError(f"pose: candidate ({k}, {m}) outside 0..{result.angles - 1}, -{result.offsets}..{result.offsets}")
        w, tlo = (int(x) for x in result.cand[b, a, k, m + result.offsets].cpu().tolist())
        if w <= 0:
            return None
    S = float(_native.GRASP_SCALE)
    cx, cy = (float(x) for x in result.dirs[k])
    mid = tlo + (w - 1) / 2.0
    X, Y = rec[5] + mid * cx - m * cy, rec[6] + mid * cy + m * cx             # units of 1/S cell; cell i spans [i, i+1)
    n, c, u, v = placement.plane_axes(result.planes, b)
    cell = result.cell_mm / 1000.0
    center = placement.grid_point(c, u, v, result.grid, result.cell_mm, X / S, Y / S)
    axis = cx * u + cy * v
    n = n / np.linalg.norm(n)
    axis = axis - (axis @ n) * n                                               # the record is float32: u.n is not exactly 0
    axis = axis / np.linalg.norm(axis)
    return GraspPose(center, axis, w * cell, (w + 2 * result.gap) * cell, k, m)
