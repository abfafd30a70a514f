"""What the table looked like where the camera cannot see it now: a per-stream memory of the table grid, fused with every
new frame on the device (uoc_scene_step, include/uoc_hip.h).

    mem = Memory(grid=256, max_age=30)                        # one stream; the state lives on the GPU
    placed = placement.free_space(labels, xyz, fitted)        # this frame alone: the arm's shadow is `unknown`
    res = mem.update(placed)                                  # observed cells overwrite, hidden ones keep what was last seen
    res.state[b], res.owner[b], res.dist2[b]                  # the fused grids, as free_space's
    res.age[b], res.change[b]                                 # 0 seen now / k steps ago / -1 unknown; CODES per cell
    res.ids[b, a], res.info[b]                                # ID_FIELDS per owner id, INFO_FIELDS per frame
    routes.plan(res.placed, ...), footprint.fit(res.placed, ...)      # every grid stage takes res.placed
    appeared, vanished = changed(res)                         # [B,128] bool on the device

A cell observed in this frame replaces what the memory held and is flagged when it contradicts it (table became
obstacle, obstacle became table, the obstacle has another owner).  A cell not observed keeps its last sighting for at
most `max_age` steps, unless it is an obstacle whose id the caller drops (`drop`: the object was taken away or moved,
for instance what motion.moved reports).  The memory lives on the lattice of one plane: a frame whose record differs
restarts the stream.  Integer arithmetic in HIP kernels: defined exactly, independent of launch order and batch.
`Memory.update` neither copies to the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _native, placement

NUM_IDS = 128
CODES = {"same": _native.SCENE_SAME, "appeared": _native.SCENE_APPEARED, "vanished": _native.SCENE_VANISHED,
         "reowned": _native.SCENE_REOWNED}
ID_FIELDS = ("cells_now", "cells_kept", "oldest", "appeared", "vanished", "reowned_in", "reowned_out", "forgotten")
INFO_FIELDS = ("status", "steps", "observed", "kept", "forgotten", "appeared", "vanished", "reowned")
NO_LATTICE, STEPPED, RESTARTED = 0, 1, 2                   # info[..., 0]


class SceneResult(_native.Fields):
    """Device tensors.  state, owner, dist2, age, change: [B,G,G] int32, the fused grids; ids [B,128,8] int32 (ID_FIELDS per
    owner id, row 0: the obstacles without an id); info [B,8] int32 (INFO_FIELDS); answers [B,Q,4] int32 as free_space's.
    placed: a PlacementResult of the fused grids, what the other grid stages take."""


def _check_age(max_age) -> int:
    if not 0 <= int(max_age) <= _native.SCENE_MAX_AGE:
        raise ValueError(f"max_age = {max_age} outside 0..{_native.SCENE_MAX_AGE}")
    return int(max_age)


def state_words(grid) -> int:
    """int32 words of one stream's state."""
    return _native.SCENE_MEM_WORD + int(grid) * int(grid)


def drop_mask(ids, B):
    """The drop masks [B,4] int32 (host, numpy) of `ids`: a list of ids for every stream, or a list of B id lists."""
    ids = list(ids)
    per = [list(x) for x in ids] if ids and all(isinstance(x, (list, tuple, np.ndarray)) for x in ids) else [ids] * int(B)
    if len(per) != int(B):
        raise ValueError(f"drop: {len(per)} id lists for {B} streams")
    w = np.zeros((int(B), 4), np.uint32)
    for b, row in enumerate(per):
        for a in row:
            a = int(a)
            if not 0 <= a < NUM_IDS:
                raise ValueError(f"drop: id {a} outside 0..{NUM_IDS - 1}")
            w[b, a >> 5] |= np.uint32(1 << (a & 31))
    return w.view(np.int32)


def _pack_drop(drop, B, dev):
    """None, id lists or a [B,128] bool device tensor -> None or [B,4] int32 on the device, without a host read."""
    if drop is None:
        return None
    if isinstance(drop, torch.Tensor):
        if drop.device != dev or tuple(drop.shape) != (B, NUM_IDS) or drop.dtype != torch.bool:
            raise _native.NativeError(f"scene: drop is not a [{B},{NUM_IDS}] bool tensor on {dev}")
        bits = drop.view(B, 4, 32).to(torch.int64)
        weight = torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, dtype=torch.int64, device=dev)
        weight[31] = -(1 << 31)                            # bit 31 is the sign of an int32 word
        return (bits * weight).sum(-1).to(torch.int32).contiguous()
    return torch.from_numpy(drop_mask(drop, B)).to(dev)


def scene_records(state_cur, owner_cur, frame, drop, mem, max_age, unknown_blocks, queries=()):
    """The raw uoc_scene_step call on bare tensors: (state, owner, dist2, age, change [B,G,G], ids [B,128,8], info [B,8],
    answers [B,Q,4]) int32 on the device, no synchronisation.  state_cur, owner_cur: device tensors [B,G,G] or [G,G] of any
    integer type and layout (they are made int32 and contiguous); frame: [B,16] int64 on the device or None; drop: [B,4]
    int32 on the device or None; mem: the streams' state, int32 [B, 48 + G*G] contiguous, updated in place; queries: a
    sequence of (need2, ai, aj, mode)."""
    sc, oc = _native.grid_inputs("scene", state_cur, owner_cur)
    B, G = int(sc.shape[0]), int(sc.shape[1])
    dev = sc.device
    _check_age(max_age)
    qs = placement._check_queries(queries)
    Q = len(qs)
    if not (_native.on_gpu(mem) and mem.device == dev and mem.dtype == torch.int32 and mem.is_contiguous()
            and tuple(mem.shape) == (B, state_words(G))):
        raise _native.NativeError(f"scene: the state is not a contiguous int32 [{B},{state_words(G)}] tensor on {dev}")
    if frame is not None:
        if not (isinstance(frame, torch.Tensor) and frame.device == dev and frame.dtype == torch.int64 and tuple(frame.shape) == (B, 16)):
            raise _native.NativeError(f"scene: the frame records do not match the {B} frames on {dev}")
        frame = frame.contiguous()
    if drop is not None:
        if not (isinstance(drop, torch.Tensor) and drop.device == dev and drop.dtype == torch.int32 and tuple(drop.shape) == (B, 4)):
            raise _native.NativeError(f"scene: drop is not an int32 [{B},4] tensor on {dev}")
        drop = drop.contiguous()
    ws = _native.workspace("uoc_scene_workspace_bytes", dev, B, G, who="scene", hint=f"B={B} or {placement.grid_hint(G)}")
    state, owner, dist2, age, change = (torch.empty((B, G, G), dtype=torch.int32, device=dev) for _ in range(5))
    ids = torch.empty((B, NUM_IDS, _native.SCENE_ID_WORDS), dtype=torch.int32, device=dev)
    info = torch.empty((B, _native.SCENE_INFO_WORDS), dtype=torch.int32, device=dev)
    answers = torch.empty((B, Q, 4), dtype=torch.int32, device=dev)
    _native.call("uoc_scene_step", dev, sc, oc, frame, drop, B, G, int(max_age), 1 if unknown_blocks else 0,
                 _native.host_words(qs, 4) if Q else None, Q, mem, state, owner, dist2, age, change, ids, info,
                 answers if Q else None, ws, ws.numel())
    return state, owner, dist2, age, change, ids, info, answers


class Memory:
    """The memory of `streams` table grids of `grid` x `grid` cells.  It owns the state tensor (`.state`, int32
    [streams, 48 + grid*grid] on the device: the lattice record, the meta words and one word per cell).  max_age: how many
    steps a cell that is not observed keeps its last sighting, 0..32767 (0: plain frame differencing); unknown_blocks:
    None takes each frame's own setting."""

    def __init__(self, grid, max_age=30, unknown_blocks=None, streams=1, device=None):
        self.grid = placement.check_grid(grid)
        self.max_age = _check_age(max_age)
        self.unknown_blocks = None if unknown_blocks is None else bool(unknown_blocks)
        self.streams = int(streams)
        if not 1 <= self.streams <= 65535:
            raise ValueError(f"streams = {streams} outside 1..65535")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _native.NativeError(f"scene.Memory: device {dev} is not a GPU (there is no CPU fallback)")
        self.state = torch.zeros((self.streams, state_words(self.grid)), dtype=torch.int32, device=dev)

    def reset(self, which=-1):
        """Forgets stream `which`, or every stream with -1."""
        if not -1 <= int(which) < self.streams:
            raise ValueError(f"reset: which = {which} outside -1..{self.streams - 1}")
        _native.call("uoc_scene_reset", self.state.device, self.state, self.streams, self.grid, int(which))

    def steps(self):
        """[streams] int32 on the device: the steps each stream has taken."""
        return self.state[:, _native.SCENE_META_WORD]

    def update(self, placed, drop=None, queries=None) -> SceneResult:
        """placed: a placement.free_space result of `streams` frames on this grid, every frame of a stream rasterised in the
        same plane.  drop: None, a list of ids (for every stream), a list of id lists per stream, or a [streams,128] bool
        device tensor: the remembered obstacles of these ids are forgotten where they are not observed.  queries: up to 16
        (need2, ai, aj, mode) from placement.widest / nearest, answered on the fused grid.  Returns a SceneResult."""
        B, G = self.streams, self.grid
        if placed.grid != G or tuple(placed.state.shape) != (B, G, G):
            raise ValueError(f"update: a result of {tuple(placed.state.shape)} cells for a memory of {B} streams of grid {G}")
        if placed.state.device != self.state.device:
            raise _native.NativeError(f"update: the result is on {placed.state.device}, the memory on {self.state.device}")
        qs = placement._check_queries(queries)
        ub = placed.unknown_blocks if self.unknown_blocks is None else self.unknown_blocks
        state, owner, dist2, age, change, ids, info, answers = scene_records(
            placed.state, placed.owner, getattr(placed, "frame", None), _pack_drop(drop, B, self.state.device), self.state,
            self.max_age, ub, qs)
        cells = ids[..., 0] + ids[..., 1]
        cells[:, 0] = placed.cells[:, 0]
        fused = placement.PlacementResult(state=state, owner=owner, dist2=dist2, cells=cells, outside=cells[:, 0], frame=placed.frame,
                                          answers=answers, planes=placed.planes, queries=qs, grid=G, cell_mm=placed.cell_mm,
                                          h_obs_mm=placed.h_obs_mm, tau_mm=placed.tau_mm, min_pts=placed.min_pts,
                                          unknown_blocks=bool(ub))
        return SceneResult(state=state, owner=owner, dist2=dist2, age=age, change=change, ids=ids, info=info, answers=answers,
                           placed=fused, max_age=self.max_age, grid=G)


def changed(result, min_cells=4):
    """(appeared, vanished): [B,128] bool on the device, the ids with at least `min_cells` cells that turned from table to
    their obstacle, and from their obstacle to table, in this step."""
    return result.ids[..., 3] >= int(min_cells), result.ids[..., 4] >= int(min_cells)


def remembered_mask(result):
    """[B,G,G] bool on the device: the cells of the fused grid that were not observed in this frame."""
    return result.age > 0
