"""How an object moved on the table between two frames: a rotation about the plane normal and an in-plane shift, by an
exhaustive integer search on the table grid, on the device (uoc_motion, include/uoc_hip.h).

    before = placement.free_space(labels0, xyz0, fitted)         # the top-down grids of §15, both in ONE plane frame
    after = placement.free_space(labels1, xyz1, fitted)
    res = register(before, after, [(5, 5)])                       # 32 rotations over a full turn, shifts up to 8 cells
    res.best[b, p]                                                # BEST_FIELDS: status, k, si, sj, cost, n_a, n_b, still, ...
    res.rot[b, p, k]                                              # (cost, si, sj, 0): the best shift per rotation
    transform(res, 0, 0)                                          # angle, travel in metres, the 4x4 in camera coordinates
    moved(res), ambiguous(res, 10)                                # [B,P] bool on the device

The object of a pair is the set of obstacle cells its id owns.  The two masks are aligned at their rounded centroids
(the pivots); every rotation of the table and every shift within `radius` cells is scored by the cells the turned and
shifted "before" mask and the "after" mask do not share, counted both ways, and the least (cost, shift, turn) wins, so a
symmetric object gets its smaller rotation.  Both grids must come from the same plane record: the camera does not move
between the two frames and the plane is fitted once (`Follower` keeps it).  Integer arithmetic in HIP kernels: defined
exactly, independent of launch order and batch.  `register` with explicit pairs neither copies to the host nor
synchronises.  No CPU fallback."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _native, placement

BEST_FIELDS = ("status", "k", "si", "sj", "cost", "n_a", "n_b", "still", "pi", "pj", "qi", "qj", "ti", "tj", "second", "zero")
EVALUATED, NO_FRAME, EMPTY, TOO_LARGE = 1, 0, 2, 3          # best[..., 0]
MotionTransform = namedtuple("MotionTransform", "angle k shift_uv shift_xyz T cost still")


class MotionResult(_native.Fields):
    """Device tensors.  rot [B,P,64,4] int32: (cost, si, sj, 0) per rotation, (-1, 0, 0, 0) past the table's end and for
    a pair that was not evaluated; best [B,P,16] int32: BEST_FIELDS per pair.  table: the rotation table [A,2] and pairs
    [P,2] (host, numpy).  angles, radius; grid, cell_mm, planes: of the placement results the grids came from."""


def rotation_table(A):
    """[A,2] int64: (rint(cos(2 pi k / A) S), rint(sin(2 pi k / A) S)), S = 16384, a full turn in A steps."""
    A = int(A)
    if not 1 <= A <= _native.MOTION_MAX_ROT:
        raise ValueError(f"angles = {A} outside 1..{_native.MOTION_MAX_ROT}")
    t = 2.0 * np.pi * np.arange(A, dtype=np.float64) / A
    return np.stack([np.rint(np.cos(t) * _native.MOTION_SCALE), np.rint(np.sin(t) * _native.MOTION_SCALE)], axis=1).astype(np.int64)


def same_ids(ids):
    """The pairs (a, a) of the ids."""
    return [(int(a), int(a)) for a in ids]


def _check_pairs(pairs):
    p = np.asarray(pairs, dtype=np.int64)
    if p.ndim == 1 and p.size == 2:
        p = p[None]
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pairs has shape {p.shape}, not [P,2]")
    if not 1 <= len(p) <= _native.MOTION_MAX_PAIRS:
        raise ValueError(f"{len(p)} pairs, outside 1..{_native.MOTION_MAX_PAIRS}")
    if p.min() < 1 or p.max() > 127:
        raise ValueError("pairs has an id outside 1..127")
    return np.ascontiguousarray(p.astype(np.int32))


def motion_records(state_a, owner_a, frame_a, state_b, owner_b, frame_b, table, radius, pairs):
    """The raw uoc_motion call on bare grids: (rot [B,P,64,4], best [B,P,16]) int32 on the device, no synchronisation.
    state_x, owner_x: device tensors [B,G,G] or [G,G] of any integer type and layout (they are made int32 and
    contiguous); frame_x: [B,16] int64 on the device, or both None; table: [A,2] integers in -S..S; pairs: [P,2]."""
    sa, oa = _native.grid_inputs("motion", state_a, owner_a)
    sb, ob = _native.grid_inputs("motion", state_b, owner_b)
    if tuple(sa.shape) != tuple(sb.shape) or sa.device != sb.device:
        raise _native.NativeError(f"motion: the grids before {tuple(sa.shape)} and after {tuple(sb.shape)} are not of one shape on one device")
    B, G = int(sa.shape[0]), int(sa.shape[1])
    dev = sa.device
    if (frame_a is None) != (frame_b is None):
        raise _native.NativeError("motion: one of the two frame records is None and the other is not")
    frames = []
    for fr in (frame_a, frame_b):
        if fr is not None:
            if not (isinstance(fr, torch.Tensor) and fr.device == dev and fr.dtype == torch.int64 and tuple(fr.shape) == (B, 16)):
                raise _native.NativeError(f"motion: the frame records do not match the {B} frames on {dev}")
            fr = fr.contiguous()
        frames.append(fr)
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int64))
    if t.ndim != 2 or t.shape[1] != 2:
        raise ValueError(f"table has shape {t.shape}, not [A,2]")
    A = int(t.shape[0])
    if not 1 <= A <= _native.MOTION_MAX_ROT:
        raise ValueError(f"angles = {A} outside 1..{_native.MOTION_MAX_ROT}")
    if np.abs(t).max() > _native.MOTION_SCALE:
        raise ValueError(f"table has a word outside -{_native.MOTION_SCALE}..{_native.MOTION_SCALE}")
    R = int(radius)
    if not 0 <= R <= _native.MOTION_MAX_RADIUS:
        raise ValueError(f"radius = {radius} outside 0..{_native.MOTION_MAX_RADIUS}")
    pr = _check_pairs(pairs)
    P = len(pr)
    ws = _native.workspace("uoc_motion_workspace_bytes", dev, B, G, A, P, who="motion", hint=f"B={B} or {placement.grid_hint(G)}")
    rot = torch.empty((B, P, _native.MOTION_MAX_ROT, _native.MOTION_ROT_WORDS), dtype=torch.int32, device=dev)
    best = torch.empty((B, P, _native.MOTION_BEST_WORDS), dtype=torch.int32, device=dev)
    _native.call("uoc_motion", dev, sa, oa, frames[0], sb, ob, frames[1], B, G, _native.host_words(t, 2), A, R,
                 _native.host_words(pr, 2), P, rot, best, ws, ws.numel())
    return rot, best


def register(before, after, pairs="same", angles=32, radius=8) -> MotionResult:
    """before, after: two placement.free_space results of the same frames, of equal grid, cell and device, rasterised in
    the same plane.  pairs: up to 16 (id_before, id_after), for instance from same_ids(ids) or, across a re-labelling,
    from the tracker; "same" takes (a, a) for every id that owns cells in both results (one small host read; ValueError
    when there are none or more than 16).  angles: rotations over a full turn, 1..64; radius: the largest shift of the
    pivot past the centroids' own travel, 0..16 cells.  Returns a MotionResult."""
    if (before.grid, before.cell_mm) != (after.grid, after.cell_mm):
        raise ValueError(f"register: grid {before.grid} of {before.cell_mm} mm before, grid {after.grid} of {after.cell_mm} mm after")
    if before.state.device != after.state.device or tuple(before.state.shape) != tuple(after.state.shape):
        raise ValueError("register: the two results are not of the same frames on one device")
    table = rotation_table(angles)
    if isinstance(pairs, str):
        if pairs != "same":
            raise ValueError(f"register: pairs = {pairs!r} is neither 'same' nor a list of pairs")
        both = ((before.cells[:, 1:] > 0) & (after.cells[:, 1:] > 0)).any(0).cpu().numpy()
        pairs = same_ids(np.nonzero(both)[0] + 1)
        if not 1 <= len(pairs) <= _native.MOTION_MAX_PAIRS:
            raise ValueError(f"register: {len(pairs)} ids own cells before and after; pass 1..{_native.MOTION_MAX_PAIRS} pairs")
    pr = _check_pairs(pairs)
    rot, best = motion_records(before.state, before.owner, getattr(before, "frame", None), after.state, after.owner,
                               getattr(after, "frame", None), table, radius, pr)
    return MotionResult(rot=rot, best=best, table=table, pairs=pr, angles=len(table), radius=int(radius), grid=before.grid,
                        cell_mm=before.cell_mm, planes=before.planes)


# ---- host helpers -----------------------------------------------------------------------------------------------------
def _axes(planes, b):
    """(centroid, u, v, n) of frame b, orthonormal: the record is float32, so u.n is not exactly 0."""
    n, c, u, v = placement.plane_axes(planes, b)
    n = n / np.linalg.norm(n)
    u = u - (u @ n) * n
    u = u / np.linalg.norm(u)
    v = v - (v @ n) * n - (v @ u) * u
    return c, u, v / np.linalg.norm(v), n


def transform(result, b, p):
    """The motion of pair p in frame b as a MotionTransform, None unless it was evaluated.  `angle` = 2 pi k / A in
    (-pi, pi], about the plane normal from u towards v; `shift_uv`, the pivot's travel along u and v in metres, and
    `shift_xyz`, the same in camera coordinates; `T`, the 4x4 x -> Rot (x - P_a) + P_b in camera coordinates with Rot =
    cos (u u' + v v') + sin (v u' - u v') + n n' and P_a, P_b the centres of the pivot cell before and of where it went
    (placement.cell_to_camera); `cost` and `still`, the mismatch in cells after the motion and without it.  float64 on
    the host from the plane record; one small host read."""
    rec = [int(x) for x in result.best[b, p].cpu().tolist()]
    if rec[0] != EVALUATED:
        return None
    k, si, sj, pi, pj, qi, qj, ti, tj = rec[1], rec[2], rec[3], rec[8], rec[9], rec[10], rec[11], rec[12], rec[13]
    A = result.angles
    angle = 2.0 * np.pi * (k if 2 * k <= A else k - A) / A
    c, u, v, n = _axes(result.planes, b)
    pa = placement.grid_point(c, u, v, result.grid, result.cell_mm, pi + 0.5, pj + 0.5)
    pb = placement.grid_point(c, u, v, result.grid, result.cell_mm, qi + si + 0.5, qj + sj + 0.5)
    rot = np.cos(angle) * (np.outer(u, u) + np.outer(v, v)) + np.sin(angle) * (np.outer(v, u) - np.outer(u, v)) + np.outer(n, n)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot, pb - rot @ pa
    cell = result.cell_mm / 1000.0
    return MotionTransform(angle, k, (ti * cell, tj * cell), pb - pa, T, rec[4], rec[7])


def moved(result, min_shift=0.01, min_angle=None):
    """[B,P] bool on the device: the pair was evaluated and its pivot travelled at least `min_shift` metres or it turned
    by at least `min_angle` radians (None: one step of the table)."""
    best = result.best
    A = result.angles
    step = 2.0 * np.pi / A
    need = step if min_angle is None else float(min_angle)
    k = best[..., 1]
    turn = torch.minimum(k, A - k).to(torch.float64) * step
    travel = torch.sqrt((best[..., 12].to(torch.float64) ** 2 + best[..., 13].to(torch.float64) ** 2)) * (result.cell_mm / 1000.0)
    return (best[..., 0] == EVALUATED) & ((travel >= float(min_shift)) | ((k > 0) & (turn >= need - 1e-12)))


def ambiguous(result, slack):
    """[B,P] bool on the device: the pair was evaluated and a rotation at least two steps away from the best one costs at
    most `slack` cells more: the turn of a round or square object says little."""
    best = result.best
    return (best[..., 0] == EVALUATED) & (best[..., 14] >= 0) & (best[..., 14] - best[..., 4] <= int(slack))


class Follower:
    """The motion of every object of a stream, frame against the frame before.  The plane is given once and every frame
    is rasterised in it: the camera must not move relative to the table while the follower lives (a moving camera needs
    a new plane and a new Follower).  plane: a support.fit_plane result or (normal, d, centroid, u, v) for the B frames
    of an update; grid, cell and free_space_args go to placement.free_space; angles, radius to register."""

    def __init__(self, plane, grid=256, cell=0.010, angles=32, radius=8, **free_space_args):
        rotation_table(angles)
        if not 0 <= int(radius) <= _native.MOTION_MAX_RADIUS:
            raise ValueError(f"radius = {radius} outside 0..{_native.MOTION_MAX_RADIUS}")
        self.plane, self.grid, self.cell, self.angles, self.radius, self.args = plane, grid, cell, int(angles), int(radius), free_space_args
        self.last = None

    def update(self, labels, xyz, ids=None):
        """Rasterises the frame, registers it against the frame kept from the last update and keeps the new one.  ids:
        the ids to follow, as pairs (a, a); None: every id that owns cells in both frames.  Returns a MotionResult, or
        None on the first frame and when no id is on both grids."""
        placed = placement.free_space(labels, xyz, self.plane, grid=self.grid, cell=self.cell, **self.args)
        last, self.last = self.last, placed
        if last is None:
            return None
        if ids is None:
            both = ((last.cells[:, 1:] > 0) & (placed.cells[:, 1:] > 0)).any(0).cpu().numpy()
            ids = (np.nonzero(both)[0] + 1)[:_native.MOTION_MAX_PAIRS]
        if len(ids) == 0:
            return None
        return register(last, placed, same_ids(ids), angles=self.angles, radius=self.radius)
