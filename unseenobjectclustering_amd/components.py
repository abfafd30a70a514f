"""Spatially connected components of a label map, on the device (uoc_cc_split, include/uoc_hip.h).

    out, table, counts = split_components(refined, connectivity=8, min_area=50, mode="largest")
    objs = extract_objects(out, xyz)                  # boxes no longer stretched by speckle
    tracked = tracker.update(out)
    component_table(table, counts)                    # the one host read: src, area, root, siblings per kept component

The clustering gives every pixel the id of its nearest seed in embedding space and never asks whether the pixels of an
id touch each other.  This step does: a component is a maximal set of pixels of one frame with the same id (1..127,
anything else is background) that are 4- or 8-connected through pixels of that id.  Components below `min_area` pixels
become background.  mode="all" renumbers the others 1..127 in raster order of their first pixel (two look-alike objects
that share an id come apart); mode="largest" keeps, per raw id, only the largest one under the raw id (speckle goes).
Integers only: the result is defined exactly.  `split_components` enqueues six or seven kernels and neither copies to
the host nor synchronises.  No CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _native

NUM_IDS = 128
_NF = len(_native.CC_FIELDS)


def split_components(labels, connectivity=8, min_area=1, mode="all"):
    """labels: device tensor [H,W], [1,H,W] or [B,H,W] of int32 / int64 / float ids.  Returns (out, table, counts) on the
    device: out int32 of the input's shape with values 0..127; table [B,128,4] int32 = src, area, root, siblings per
    new id (mode "all") or raw id (mode "largest"); counts [B,4] int32 = found, small, kept, dropped."""
    lab = _native.label_input("split_components", labels)
    if mode not in _native.CC_MODES:
        raise ValueError(f"mode = {mode!r} is neither 'all' nor 'largest'")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity = {connectivity} is neither 4 nor 8")
    if int(min_area) < 1:
        raise ValueError(f"min_area = {min_area} below 1")
    if lab.dim() not in (2, 3):
        raise _native.NativeError(f"split_components: labels {tuple(labels.shape)} must be [H,W] or [B,H,W]")
    lab3 = lab[None] if lab.dim() == 2 else lab
    B, H, W = (int(v) for v in lab3.shape)
    dev = lab.device
    ws = _native.workspace("uoc_cc_workspace_bytes", dev, B, H, W, who="split_components", hint=f"B={B} H={H} W={W} (H*W must be below 2^31)")
    out = torch.empty_like(lab3)
    table = torch.empty((B, NUM_IDS, _NF), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _native.call("uoc_cc_split", dev, lab3, B, H, W, int(connectivity), int(min_area), _native.CC_MODES[mode], out, table, counts,
                 ws, ws.numel())
    return out.view(lab.shape), table, counts


def component_table(table, counts, frame=0):
    """The non-empty rows of a frame's table as host arrays — the one deliberate device-to-host read: dict of label
    (the id in `out`), src, area, root, siblings (ascending label), plus found, small, kept, dropped."""
    tab = table[int(frame)].cpu().numpy()
    cnt = counts[int(frame)].cpu().numpy()
    label = np.nonzero(tab[:, 1])[0].astype(np.int32)
    rec = {name: tab[label, k].copy() for k, name in enumerate(_native.CC_FIELDS)}
    rec.update(label=label, found=int(cnt[0]), small=int(cnt[1]), kept=int(cnt[2]), dropped=int(cnt[3]))
    return rec
