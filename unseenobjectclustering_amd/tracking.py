"""Stable object ids across the frames of a stream, on the device (uoc_track_step, include/uoc_hip.h).

    tracker = Tracker(min_iou=0.3, max_age=5)
    tracked = tracker.update(refined)                 # raw label map [H,W] / [1,H,W] on the GPU -> int32 map of track slots
    objs = extract_objects(tracked, xyz)              # records keyed by track slot
    tracker.tracks()                                  # the one host read: slot, uid, age, hits, area, born of the live tracks

Every label map the segmentation produces numbers its objects from scratch.  The tracker matches the objects of the
incoming map (ids 1..127, anything else is background) against the last sighting of every live track by mask IoU —
greedily, on exact integer arithmetic — and renumbers the map with track slots 1..127: an object keeps its slot while
it is in view and gets it back after an occlusion of at most `max_age` frames; `uid` numbers the objects of a stream
1, 2, 3, ... and is never reused.  `streams` independent streams are stepped by one call and never interact.  The
state lives in device memory; `update` enqueues three kernels and neither copies to the host nor synchronises.
No CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _native

NUM_SLOTS = _native.TRACK_SLOTS
_HDR, _META, _CONT = _native.TRACK_HEADER_WORDS, _native.TRACK_META_WORD, _native.TRACK_CONT_WORDS
_NF = len(_native.TRACK_FIELDS)


def iou_threshold(min_iou) -> int:
    """q = round(min_iou * 65536), the integer threshold of the candidate test inter * 65536 >= q * union."""
    min_iou = float(min_iou)
    if not 0.0 < min_iou <= 1.0:
        raise ValueError(f"min_iou = {min_iou} outside (0, 1]")
    return max(1, int(round(min_iou * 65536)))


class Tracker:
    """Tracker(min_iou=0.3, max_age=5, streams=1).  The device state is allocated at the first update and re-allocated
    (which resets it) when H, W, the device or the number of streams of the input change."""

    def __init__(self, min_iou=0.3, max_age=5, streams=1):
        self.q = iou_threshold(min_iou)
        self.min_iou = float(min_iou)
        self.max_age = int(max_age)
        self.streams = int(streams)
        if self.max_age < 0:
            raise ValueError(f"max_age = {max_age} is negative")
        if self.streams < 1:
            raise ValueError(f"streams = {streams} must be at least 1")
        self._key = None            # (device, B, H, W) of the allocated state
        self._state = self._words = self._ws = self._lut = self._tracks = None

    # ---- state -------------------------------------------------------------------------------------
    def _ensure(self, dev, B, H, W):
        key = (dev, B, H, W)
        if self._key == key:
            return
        self._state = _native.workspace("uoc_track_state_bytes", dev, B, H, W, who="Tracker", hint=f"B={B} H={H} W={W} (H*W must be below 2^31)")
        self._words = self._state.view(torch.int32).view(B, -1)
        self._ws = _native.workspace("uoc_track_workspace_bytes", dev, B, who="Tracker", hint=f"B={B}", floor=16)
        self._lut = torch.zeros((B, NUM_SLOTS), dtype=torch.int32, device=dev)
        self._tracks = torch.zeros((B, NUM_SLOTS, _NF), dtype=torch.int32, device=dev)
        self._key = key
        self._reset(-1)

    def _reset(self, which):
        dev, B, H, W = self._key
        _native.call("uoc_track_reset", dev, self._state, B, H, W, which)

    def reset(self, stream=None):
        """Forgets every track of `stream` (all streams when None): its next update starts again at slot 1, uid 1."""
        if stream is not None and not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream = {stream} outside [0, {self.streams})")
        if self._key is None:
            return
        self._reset(-1 if stream is None else int(stream))
        sel = slice(None) if stream is None else int(stream)
        self._lut[sel] = 0
        self._tracks[sel] = 0

    # ---- stepping ------------------------------------------------------------------------------------
    def _step(self, lab, out, lut, tracks):
        dev, B, H, W = self._key
        _native.call("uoc_track_step", dev, lab, B, H, W, self.q, self.max_age, self._state, out, lut, tracks, self._ws, self._ws.numel())

    def update(self, labels):
        """labels: device tensor [H,W] (one stream) or [streams,H,W] of int32 / int64 / float ids.  Returns the tracked
        map, int32, same shape: 0 = background, else the track slot in 1..127."""
        lab = _native.label_input("Tracker.update", labels)
        squeeze = lab.dim() == 2
        if squeeze:
            lab = lab[None]
        if lab.dim() != 3 or lab.shape[0] != self.streams:
            raise _native.NativeError(f"Tracker.update: labels {tuple(labels.shape)} must be [H,W] or [{self.streams},H,W]")
        B, H, W = (int(v) for v in lab.shape)
        self._ensure(lab.device, B, H, W)
        out = torch.empty_like(lab)
        self._step(lab, out, self._lut, self._tracks)
        return out[0] if squeeze else out

    # ---- views -----------------------------------------------------------------------------------------
    @property
    def lut(self):
        """[streams,128] int32 on the device: raw id -> track slot of the last update (0 = background / dropped)."""
        return self._lut

    @property
    def table(self):
        """[streams,128,5] int32 on the device: uid, age, hits, area, born per slot after the last update."""
        return self._tracks

    @property
    def memory(self):
        """[streams,H,W] int32 view of the state's memory map (the last uncovered sighting of every live track)."""
        if self._key is None:
            return None
        _, B, H, W = self._key
        return self._words[:, _HDR + _CONT:_HDR + _CONT + H * W].view(B, H, W)

    @property
    def state_words(self):
        """[streams, words] int32 view of the whole device state (header, contingency scratch, memory map)."""
        return self._words

    def tracks(self, stream=0):
        """The live tracks of `stream` as host arrays — the one deliberate device-to-host read: dict of slot, uid, age,
        hits, area, born (ascending slot), plus dropped, step and next_uid."""
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream = {stream} outside [0, {self.streams})")
        if self._key is None:
            head = np.zeros(_HDR, dtype=np.int32)
        else:
            head = self._words[int(stream), :_HDR].cpu().numpy()
        tab = head[:NUM_SLOTS * _NF].reshape(NUM_SLOTS, _NF)
        slot = np.nonzero(tab[:, 0])[0].astype(np.int32)
        rec = {name: tab[slot, k].copy() for k, name in enumerate(_native.TRACK_FIELDS)}
        rec.update(slot=slot, next_uid=int(head[_META]) + 1, step=int(head[_META + 1]), dropped=int(head[_META + 2]))
        return rec


def track_sequence(labels, min_iou=0.3, max_age=5, tracker=None):
    """One stream's gathered block: labels [T,H,W] on the device, frame after frame through one tracker (a fresh one
    unless `tracker` continues a stream), the T steps enqueued back to back without a host read.  Returns the tracked
    maps [T,H,W] int32 and uids [T,128] int32 (uid of every slot after step t, 0 = free)."""
    tr = tracker if tracker is not None else Tracker(min_iou, max_age, streams=1)
    if tr.streams != 1:
        raise ValueError("track_sequence steps one stream")
    lab = _native.label_input("track_sequence", labels)
    if lab.dim() != 3:
        raise _native.NativeError(f"track_sequence: labels {tuple(labels.shape)} must be [T,H,W]")
    T, H, W = (int(v) for v in lab.shape)
    out = torch.empty_like(lab)
    table = torch.zeros((T, NUM_SLOTS, _NF), dtype=torch.int32, device=lab.device)
    if T:
        tr._ensure(lab.device, 1, H, W)
    for t in range(T):
        tr._step(lab[t], out[t], tr._lut, table[t])
    if T:
        tr._tracks.copy_(table[T - 1:T])
    return out, table[:, :, 0].contiguous()
