"""How the objects of a frame stand to each other, on the device (uoc_relations, include/uoc_hip.h):
which lie side by side, which is in front of which, which is cut by the image edge, which can be picked first.

    res = relate(refined, xyz)                        # labels [B,H,W] / [H,W] on the GPU, xyz = sample['depth'] [B,3,H,W]
    res.front[b, a, c]                                # neighbouring pixel pairs where id a is nearer than id c by >= gap
    res.layer[b, k], res.free[b, k], res.order[b, k]  # object k: peeling layer, pickable now, rank in the pick order
    pick_order(res, b)                                # the present ids, the topmost first

Pairs of 4- or 8-neighbouring pixels with different ids (1..127, everything else is id 0) are counted into three 128x128
tables: `border` (all of them), `touch` (both depths valid and closer than `gap`) and `front` (the nearer id first).
An id occludes another when it is in front on at least `min_pairs` pairs and on more pairs than the other way round;
layers come from peeling the occlusion graph.  Integer arithmetic in HIP kernels: defined exactly, independent of launch
order and batch.  `relate` neither copies to the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

import torch

from . import _native

NUM_IDS = 128
OBJECT_FIELDS = tuple(name for name, _ in _native.UocRelationObject._fields_)
TABLES = ("border", "touch", "front")


class RelationResult(_native.Fields):
    """Device tensors, all int32.  border, touch, front: [B,128,128]; pixels, edge, border_sum (the record's `border`),
    border_bg, hidden, n_touch, n_above, n_below, layer, free, order: [B,128]."""


def relation_records(labels, xyz, connectivity, gap_mm, min_pairs):
    """The raw uoc_relations call: (pairs [B,3,128,128] int32, objects [B,128,11] int32 holding uoc_relation_object), on
    the device, no synchronisation.  labels int32 [B,H,W] and xyz float32 [B,3,H,W] contiguous on one GPU."""
    B, H, W = (int(v) for v in labels.shape)
    dev = labels.device
    ws = _native.workspace("uoc_relations_workspace_bytes", dev, B, H, W, who="relate", hint=f"B={B} H={H} W={W} (H*W must be below 2^29)")
    pairs = torch.empty((B, 3, NUM_IDS, NUM_IDS), dtype=torch.int32, device=dev)
    objs = torch.empty((B, NUM_IDS, len(OBJECT_FIELDS)), dtype=torch.int32, device=dev)
    _native.call("uoc_relations", dev, labels, xyz, B, H, W, int(connectivity), int(gap_mm), int(min_pairs), pairs, objs, ws, ws.numel())
    return pairs, objs


def relate(labels, xyz, connectivity=4, gap=0.015, min_pairs=8) -> RelationResult:
    """labels: device tensor [B,H,W] or [H,W] of int32 / int64 / float ids; xyz: [B,3,H,W] or [3,H,W] float metres
    (sample['depth']), of which only z is read.  connectivity 4 or 8; gap = the depth step in metres from which two
    neighbouring pixels are in front of / behind each other, used in whole millimetres (int(round(gap*1000)) in
    1..65535); min_pairs >= 1 pairs make a relation.  Returns a RelationResult."""
    if int(connectivity) not in (4, 8):
        raise ValueError(f"connectivity = {connectivity} is neither 4 nor 8")
    gap_mm = int(round(float(gap) * 1000))
    if not 1 <= gap_mm <= _native.REL_MAX_GAP_MM:
        raise ValueError(f"gap = {gap} m is {gap_mm} mm, outside 1..{_native.REL_MAX_GAP_MM} mm")
    if int(min_pairs) < 1:
        raise ValueError(f"min_pairs = {min_pairs} is below 1")
    lab, xyz = _native.frame_inputs("relate", labels, xyz)
    pairs, objs = relation_records(lab, xyz, connectivity, gap_mm, min_pairs)
    fields = {("border_sum" if k == "border" else k): objs[..., i] for i, k in enumerate(OBJECT_FIELDS)}
    fields.update(border=pairs[:, _native.REL_BORDER], touch=pairs[:, _native.REL_TOUCH], front=pairs[:, _native.REL_FRONT])
    return RelationResult(connectivity=int(connectivity), gap_mm=gap_mm, min_pairs=int(min_pairs), **fields)


# ---- host helpers: small id lists for the consumer (each copies one row or one table to the host) ----------------------
def pick_order(result, b=0):
    """The present ids of frame b in pick order: `order` 1, 2, ... (upper layers first, cycles last, ids ascending)."""
    order = result.order[b].cpu()
    ids = torch.nonzero(order > 0)[:, 0]
    return [int(i) for i in ids[torch.argsort(order[ids])]]


def occluders(result, b, a):
    """The ids in 1..127 that occlude id a in frame b, ascending."""
    front = result.front[b].cpu()
    col, row = front[1:, int(a)], front[int(a), 1:]
    return [int(i) + 1 for i in torch.nonzero((col >= result.min_pairs) & (col > row))[:, 0]]


def neighbours(result, b, a):
    """The ids in 1..127 that touch id a in frame b, ascending."""
    return [int(i) + 1 for i in torch.nonzero(result.touch[b, int(a), 1:].cpu() >= result.min_pairs)[:, 0]]
