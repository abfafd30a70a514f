"""Engineered inputs for the two-stage glue kernels (csrc/roi.hip): every builder returns plain numpy / torch CPU inputs
that sit ON a decision edge of the reference — a coverage fraction equal to its threshold, a padding product of x.5, a box
clamped on one border, an overlap of exactly 0.5, bit-equal or NaN sort keys — plus the metadata that
tests/test_glue_cases_host.py needs to prove, with oracle/glue_oracle.py alone, that the edge is really hit.
tests/test_glue_edges_gpu.py runs the same inputs through the HIP kernels.

Also here: the float64 / nearest references of the resampling sweeps and the bound the bilinear crops are held to."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from unseenobjectclustering_amd import _native

THRESHOLDS = (0.5, 0.8)             # the two depth-coverage thresholds the project uses ('ocid', 'osd' / test_sample)
NOT_POSITIVE = (0.0, -0.0, -1.5, float("nan"), -3.0e38)      # none of these counts as z > 0
POSITIVE = (0.5, 1.0, 3.75)
SWEEP_S = (1, 2, 3, 7, 8, 16)       # crop sizes of the resampling sweeps
SWEEP_EXTENT = 40                   # window extents 1..40
SWEEP_H, SWEEP_W = 61, 67           # frame of the sweeps (odd, no multiple of anything)


# ---- depth-coverage filter -------------------------------------------------------------------------------------------
# id, pixels, pixels with z > 0, and the edge the label is named for: ("at", thr) -> fraction == thr in float32 (kept at
# thr: the test is `<`); ("below", thr) -> the nearest fraction below thr with that pixel count (removed at thr);
# ("none", thr) -> no covered pixel (removed)
FILTER_SPEC = (
    dict(id=1, cnt=5, zpos=4, edge=("at", 0.8)),
    dict(id=2, cnt=5, zpos=3, edge=("below", 0.8)),
    dict(id=3, cnt=10, zpos=8, edge=("at", 0.8)),
    dict(id=7, cnt=10, zpos=7, edge=("below", 0.8)),
    dict(id=16, cnt=5, zpos=4, edge=("at", 0.8)),        # 10000 % 128: an unguarded id would land here
    dict(id=19, cnt=2, zpos=1, edge=("at", 0.5)),
    dict(id=20, cnt=2, zpos=0, edge=("below", 0.5)),
    dict(id=33, cnt=5, zpos=4, edge=("at", 0.8), blobs=True),     # two distant blobs, one id
    dict(id=50, cnt=10, zpos=5, edge=("at", 0.5)),
    dict(id=64, cnt=149, zpos=119, edge=("below", 0.8)),          # 0.79866: the nearest below with many pixels
    dict(id=90, cnt=6, zpos=0, edge=("none", 0.5)),                  # no pixel with z > 0 at all
    dict(id=100, cnt=149, zpos=74, edge=("below", 0.5)),          # 0.49664
    dict(id=127, cnt=5, zpos=4, edge=("at", 0.8)),                # the largest id
)
FILTER_H, FILTER_W = 24, 31


def _paint(lab, z, pix, mid, zpos, rng):
    """Label the flat pixel indices `pix` with `mid`; `zpos` of them (random ones) get a positive z, the rest cycle
    through the values that are not positive (0, -0, negative, NaN, very negative)."""
    pix = np.asarray(pix)
    order = rng.permutation(len(pix))
    vals = np.empty(len(pix), np.float32)
    vals[order[:zpos]] = np.resize(np.asarray(POSITIVE, np.float32), zpos)
    vals[order[zpos:]] = np.resize(np.asarray(NOT_POSITIVE, np.float32), len(pix) - zpos)
    lab.reshape(-1)[pix] = mid
    z.reshape(-1)[pix] = vals


def _filter_item(spec, rng, H=FILTER_H, W=FILTER_W):
    """One [H,W] label map and its [3,H,W] XYZ image.  Background (label 0) has no depth at all; the x and y planes are
    positive everywhere, so a kernel that reads the wrong plane (a wrong batch stride) finds every label covered."""
    lab = np.zeros((H, W), np.float32)
    xyz = np.ones((3, H, W), np.float32)
    xyz[2] = 0.0
    cursor = 3
    for s in spec:
        n = s["cnt"]
        if s.get("blobs"):
            pix = list(range(cursor, cursor + 3)) + list(range(H * W - 3 - (n - 3), H * W - 3))
            cursor += 3 + 2
        else:
            pix = list(range(cursor, cursor + n))
            cursor += n + 2
        assert cursor < H * W - 12, "frame too small for the spec"
        _paint(lab, xyz[2], pix, s["id"], s["zpos"], rng)
    return lab, xyz


def filter_frame():
    """-> labels [1,H,W] float32, depth [1,3,H,W] float32, FILTER_SPEC."""
    lab, xyz = _filter_item(FILTER_SPEC, np.random.RandomState(21))
    return torch.from_numpy(lab)[None], torch.from_numpy(xyz)[None], FILTER_SPEC


# per item of a batch of 3: label 5 fails only in item 1 and label 6 only in item 2 — with statistics that are not reset
# per item both would pass (13/15) —, labels 9 and 11 exist in item 1 only.
FILTER_BATCH_SPEC = (
    (dict(id=5, cnt=10, zpos=10), dict(id=6, cnt=5, zpos=5), dict(id=1, cnt=5, zpos=4)),
    (dict(id=5, cnt=5, zpos=3), dict(id=6, cnt=5, zpos=5), dict(id=9, cnt=2, zpos=0), dict(id=11, cnt=4, zpos=4)),
    (dict(id=5, cnt=5, zpos=5), dict(id=6, cnt=5, zpos=3), dict(id=1, cnt=5, zpos=4)),
)


def filter_batch():
    """-> labels [3,H,W] float32, depth [3,3,H,W] float32, FILTER_BATCH_SPEC."""
    rng = np.random.RandomState(22)
    items = [_filter_item(spec, rng) for spec in FILTER_BATCH_SPEC]
    return (torch.from_numpy(np.stack([i[0] for i in items])), torch.from_numpy(np.stack([i[1] for i in items])),
            FILTER_BATCH_SPEC)


INVALID_IDS = (-1, 128, 10000, -128, 2 ** 31 - 1, -2 ** 31)


def filter_raw_abi():
    """filter_frame() as int32 with background pixels overwritten by ids outside [0, 128), all without depth: taken
    modulo 128 they would fall on labels 127, 0 and 16, which sit exactly at 0.8 and would drop below it.
    -> labels int32 [1,H,W], depth, the same map with those pixels set to 0 (what the oracle can take), their mask."""
    lab, depth, _ = filter_frame()
    raw = lab.to(torch.int32)
    free = torch.nonzero(raw.reshape(-1) == 0).reshape(-1)
    where = free[torch.arange(0, 3 * len(INVALID_IDS)) * 5 + 1]
    vals = torch.tensor(INVALID_IDS, dtype=torch.int64).repeat(3).to(torch.int32)
    clean = raw.clone()
    raw.reshape(-1)[where] = vals
    invalid = torch.zeros_like(raw, dtype=torch.bool)
    invalid.reshape(-1)[where] = True
    return raw, depth, clean, invalid


# ---- boxes -----------------------------------------------------------------------------------------------------------
PAD_EXTENTS = (0, 1, 2, 3, 6, 10, 14)
PAD_EXPECT = {0: 0, 1: 0, 2: 0, 3: 1, 6: 2, 10: 2, 14: 4}      # round-half-to-even of extent / 4: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
PAD_IDS = (3, 8, 21, 40, 77, 101, 127)


def box_padding():
    """Seven rectangles: x extents 0,1,2,3,6,10,14 against y extents 14,10,6,3,2,1,0, far enough from every border that
    nothing is clamped.  -> label map [H,W] float32, [(id, ex, ey)]."""
    H, W = 28, 68
    lab = torch.zeros(H, W)
    xs = (5, 8, 12, 17, 23, 32, 45)
    meta = []
    for mid, x, ex, ey in zip(PAD_IDS, xs, PAD_EXTENTS, PAD_EXTENTS[::-1]):
        lab[5:5 + ey + 1, x:x + ex + 1] = mid
        meta.append((mid, ex, ey))
    return lab, meta


def box_clamp():
    """Four 7x7 objects (padding 2), each one pixel from ONE border.  -> label map, {id: index of the clamped box entry}
    (0 = x0 on the left border, 1 = y0 top, 2 = x1 right, 3 = y1 bottom)."""
    H, W = 40, 50
    lab = torch.zeros(H, W)
    lab[16:23, 1:8] = 1
    lab[16:23, W - 8:W - 1] = 2
    lab[1:8, 21:28] = 3
    lab[H - 8:H - 1, 21:28] = 4
    return lab, {1: 0, 2: 2, 3: 1, 4: 3}


def box_whole_frame():
    return torch.full((9, 11), 5.0)


def box_thin():
    """Single pixels (two of them in frame corners), a single row and a single column."""
    H, W = 20, 30
    lab = torch.zeros(H, W)
    lab[0, 0] = 1
    lab[10, 15] = 2
    lab[5, 3:18] = 3          # extent 14 x 0
    lab[2:13, 25] = 4         # extent 0 x 10
    lab[H - 1, W - 1] = 5
    return lab


def box_thin_frames():
    row = torch.tensor([0, 1, 1, 1, 0, 0, 2, 0, 3, 3, 3, 3, 3], dtype=torch.float32)
    return row[None, :].clone(), row[:, None].clone()


def box_many():
    """127 objects, the table's capacity, in the 4x4 cells of a 32x64 frame; ids are shuffled over the cells so that the
    ascending id order is not the raster order, and every fifth object is one pixel."""
    rng = np.random.RandomState(23)
    H, W = 32, 64
    lab = torch.zeros(H, W)
    cells = rng.permutation(128)[:127]
    for mid, cell in enumerate(cells, start=1):
        cy, cx = 4 * (cell // 16), 4 * (cell % 16)
        h, w = (1, 1) if mid % 5 == 0 else (rng.randint(1, 5), rng.randint(1, 5))
        oy, ox = rng.randint(0, 5 - h), rng.randint(0, 5 - w)
        lab[cy + oy:cy + oy + h, cx + ox:cx + ox + w] = mid
    return lab


def box_blobs():
    lab = torch.zeros(24, 31)
    lab[2:5, 3:7] = 6
    lab[18:21, 25:29] = 6
    lab[10:12, 10:13] = 2
    return lab


def box_cases():
    """name -> label map [H,W] float32: every frame of section 'boxes'."""
    row, col = box_thin_frames()
    return {"padding": box_padding()[0], "clamp": box_clamp()[0], "whole_frame": box_whole_frame(), "thin": box_thin(),
            "frame_1xN": row, "frame_Nx1": col, "many": box_many(), "blobs": box_blobs()}


# ---- crops -----------------------------------------------------------------------------------------------------------
def ramp_noise(C, H, W, seed):
    """[C,H,W] float32 whose value differs in every pixel of every window: a ramp per channel (different slopes, so a
    transposed tap shows) plus noise (so a shifted tap does not cancel against the ramp)."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.stack([(0.37 + 0.11 * c) * x - (0.23 + 0.07 * c) * y + rng.standard_normal((H, W)) for c in range(C)])
    return torch.from_numpy(out.astype(np.float32))


def id_pattern(H, W):
    """Label map with ids 1..5, id = 1 + (x + 3y) % 5: a nearest index that is off by (dx, dy) lands on another id
    unless dx + 3 dy is a multiple of 5, so neither an off-by-one nor a transposition goes unseen."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (1 + (x + 3 * y) % 5).float()


def sweep_boxes(seed, H=SWEEP_H, W=SWEEP_W):
    """Every window extent (ch, cw) in 1..40 x 1..40 once, at a random place of the frame (borders included).
    -> int64 [1600, 4] x0,y0,x1,y1."""
    rng = np.random.RandomState(seed)
    out = []
    for ch in range(1, SWEEP_EXTENT + 1):
        for cw in range(1, SWEEP_EXTENT + 1):
            x0, y0 = rng.randint(0, W - cw + 1), rng.randint(0, H - ch + 1)
            out.append((x0, y0, x0 + cw - 1, y0 + ch - 1))
    return np.asarray(out, np.int64)


def roi_table(boxes, labels):
    """A hand-made uoc_roi_table of up to 127 boxes."""
    t = _native.RoiTable()
    t.K = len(boxes)
    assert 1 <= t.K <= 127
    for k, (b, l) in enumerate(zip(boxes, labels)):
        for i in range(4):
            t.box[k][i] = int(b[i])
        t.label[k] = int(l)
    return t


def ref_bilinear(img64, boxes, S):
    """F.interpolate(bilinear, align_corners=True) of every window of the float64 image [C,H,W] -> [K,C,S,S] float64."""
    return torch.stack([F.interpolate(img64[None, :, y0:y1 + 1, x0:x1 + 1], size=(S, S), mode="bilinear", align_corners=True)[0]
                        for x0, y0, x1, y1 in boxes.tolist()])


def ref_mask(lab, ids, boxes, S):
    """The oracle's mask crop (float32 F.interpolate, nearest) of (lab == id) in every window -> [K,S,S] float32."""
    return torch.stack([F.interpolate((lab == mid).float()[None, None, y0:y1 + 1, x0:x1 + 1], size=(S, S), mode="nearest")[0, 0]
                        for mid, (x0, y0, x1, y1) in zip(ids, boxes.tolist())])


def bilinear_bound(img, boxes):
    """Per window: 2^-23 ((cw-1) max|dx| + (ch-1) max|dy|) + 8 2^-24 max|v| -> float64 [K].
    The float32 source coordinate scale * index carries two roundings, a relative 2^-23: at most 2^-23 (cw-1) pixels
    along x, and the interpolant is continuous and piecewise linear with slope max|dx| (likewise y); the last term is the
    rounding of the weights and of the four-tap sum."""
    img = img.double()
    out = []
    for x0, y0, x1, y1 in boxes.tolist():
        w = img[:, y0:y1 + 1, x0:x1 + 1]
        dx = float((w[:, :, 1:] - w[:, :, :-1]).abs().max()) if x1 > x0 else 0.0
        dy = float((w[:, 1:, :] - w[:, :-1, :]).abs().max()) if y1 > y0 else 0.0
        out.append(2.0 ** -23 * ((x1 - x0) * dx + (y1 - y0) * dy) + 8 * 2.0 ** -24 * float(w.abs().max()))
    return np.asarray(out)


def poisoned_windows():
    """Six disjoint windows (1x1, 1xN, Nx1 and three larger) in a frame that is NaN everywhere else, the last row and
    column included: a tap that leaves its window — even with weight 0 — turns the crop into NaN.
    -> rgb [3,H,W], depth [3,H,W], label map [H,W], boxes int64 [6,4]."""
    H, W = 40, 48
    boxes = np.asarray([(2, 2, 2, 2), (5, 2, 20, 2), (2, 5, 2, 22), (6, 6, 18, 20), (22, 4, 45, 17), (21, 21, 46, 38)], np.int64)
    inside = torch.zeros(H, W, dtype=torch.bool)
    for x0, y0, x1, y1 in boxes.tolist():
        assert not inside[max(y0 - 1, 0):y1 + 2, max(x0 - 1, 0):x1 + 2].any(), "windows must not touch"
        inside[y0:y1 + 1, x0:x1 + 1] = True
    assert not inside[H - 1].any() and not inside[:, W - 1].any()
    rgb, depth = ramp_noise(3, H, W, 31), ramp_noise(3, H, W, 32)
    rgb[:, ~inside] = float("nan")
    depth[:, ~inside] = float("nan")
    return rgb, depth, id_pattern(H, W), boxes


# ---- paste-back ------------------------------------------------------------------------------------------------------
def shelf_pack(sizes, H, W):
    """Packs (h, w) boxes into as few HxW frames as a shelf packer manages, no two boxes of a frame overlapping.
    -> list of frames, each an int64 array [K,4] x0,y0,x1,y1."""
    frames, cur, x, y, shelf = [], [], 0, 0, 0
    for h, w in sorted(sizes, key=lambda s: (-s[0], -s[1])):
        if x + w > W:
            x, y, shelf = 0, y + shelf, 0
        if y + h > H:
            frames.append(np.asarray(cur, np.int64))
            cur, x, y, shelf = [], 0, 0, 0
        cur.append((x, y, x + w - 1, y + h - 1))
        x, shelf = x + w, max(shelf, h)
    frames.append(np.asarray(cur, np.int64))
    return frames


def paste_sweep_frames(H=64, W=72):
    """Every box size (h, w) in 1..40 x 1..40 once, as frames of disjoint boxes."""
    return shelf_pack([(h, w) for h in range(1, SWEEP_EXTENT + 1) for w in range(1, SWEEP_EXTENT + 1)], H, W)


def paste_labels(K, S):
    """Crop labels that differ between neighbouring crop pixels: (sy S + sx + 7k) % 127 -> [K,S,S] float32."""
    sy, sx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    return torch.stack([((sy * S + sx + 7 * k) % 127).float() for k in range(K)])


def match_all_kept_no_depth(labels_crop, rois, H, W):
    """oracle.match_label_crop for the paste sweep's special case, vectorised per ROI (the oracle's two loops over each
    ROI's cluster ids cost milliseconds per ROI, the sweep has 9600): every cluster overlaps the mask, so nothing is
    rejected; no depth, so the ROIs are painted by box area, large first (Python's stable sort on the float32 0-dim
    tensors); the boxes are disjoint.  Pinned to the oracle itself by tests/test_glue_cases_host.py.  -> refined [H,W]."""
    K = labels_crop.shape[0]
    keys = [(i, (rois[i, 3] - rois[i, 1] + 1) * (rois[i, 2] - rois[i, 0] + 1)) for i in range(K)]
    order = [i for i, _ in sorted(keys, key=lambda kv: kv[1], reverse=True)]
    refined = torch.zeros(H, W)
    count = 0
    for i in order:
        ids, inverse = torch.unique(labels_crop[i], return_inverse=True)
        relabeled = (inverse + 1 + count).float()
        count += len(ids)
        x0, y0, x1, y1 = [int(v) for v in rois[i].tolist()]
        refined[y0:y1 + 1, x0:x1 + 1] = F.interpolate(relabeled[None, None], size=(y1 - y0 + 1, x1 - x0 + 1), mode="nearest")[0, 0]
    return refined


# ---- matching --------------------------------------------------------------------------------------------------------
def eighths(rng, shape):
    """Depth values that are multiples of 1/8 in [0.5, 4): sums of up to 256 of them are exact in float32 and in
    float64, so a mean is ONE correctly rounded division whatever the summation order."""
    return torch.from_numpy(rng.randint(4, 32, size=shape).astype(np.float32) / 8)


def _crop_from_clusters(S, clusters, rng):
    """clusters: [(id, pixels, pixels inside the stage-1 mask)], scattered at random over the SxS crop.
    -> labels [S,S] float32, mask [S,S] float32."""
    assert sum(c[1] for c in clusters) == S * S
    perm = rng.permutation(S * S)
    lab, mask = np.zeros(S * S, np.float32), np.zeros(S * S, np.float32)
    a = 0
    for mid, n, inside in clusters:
        lab[perm[a:a + n]] = mid
        mask[perm[a:a + inside]] = 1.0
        a += n
    return torch.from_numpy(lab).view(S, S), torch.from_numpy(mask).view(S, S)


# ROI 0: overlap exactly 0.5 (kept) and the nearest fraction below (dropped), with few and with many pixels; id 0 kept
# (and renumbered), ids with gaps, id 127.  ROI 1: every cluster dropped.
OVERLAP_CLUSTERS = (
    ((0, 8, 4), (5, 8, 3), (64, 101, 50), (127, 100, 50), (90, 39, 39)),
    ((3, 128, 63), (4, 128, 0)),
)
OVERLAP_KEPT = ({0, 127, 90}, set())


def overlap_case():
    """-> dict(initial_masks [1,H,W], labels_crop [2,16,16], mask [2,16,16], rois [2,4] float32, depth [2,3,16,16])."""
    rng = np.random.RandomState(24)
    S, H, W = 16, 40, 48
    parts = [_crop_from_clusters(S, c, rng) for c in OVERLAP_CLUSTERS]
    depth = eighths(rng, (2, 3, S, S))
    rois = torch.tensor([[3, 4, 30, 25], [20, 15, 44, 37]], dtype=torch.float32)
    return dict(initial_masks=torch.zeros(1, H, W), labels_crop=torch.stack([p[0] for p in parts]),
                mask=torch.stack([p[1] for p in parts]), rois=rois, depth=depth)


# the five ROIs of the paint-order case, by role
ORDER_ROLES = ("near", "far", "tie_a", "tie_b", "nan")
ORDER_BOXES = {"near": (4, 4, 23, 19), "far": (14, 10, 35, 29), "tie_a": (26, 2, 45, 13), "tie_b": (30, 6, 45, 20),
               "nan": (2, 22, 20, 38)}        # tie_a and tie_b: 20x12 and 16x15 pixels, the same area


def order_case(perm=(0, 1, 2, 3, 4)):
    """Five overlapping ROIs with S = 8, listed in the order ORDER_ROLES[perm[.]]:
      near   mean depth 1.0; its upper half is a kept cluster, its lower half a dropped one, both partly over `far`
      far    mean depth 3.0: painted first although `near` may come first in the list; shows through near's dropped half
      tie_a, tie_b   overlapping, bit-equal mean depth 2.0 from different values: the list order decides
      nan    every kept pixel has z <= 0: its key is NaN, and the order is what CPython's sort makes of that
    -> dict like overlap_case() plus roles (the list of role names)."""
    rng = np.random.RandomState(25)
    S, H, W = 8, 40, 48
    half = torch.zeros(S, S)
    half[:, S // 2:] = 1.0
    crops = {}
    z = torch.full((S, S), 1.0)
    z[::2] = 0.75
    z[1::2] = 1.25
    lower = half.t().contiguous()
    crops["near"] = (2.0 + 7.0 * lower, 1.0 - lower, z)                        # ids 2 (kept, upper half) and 9 (dropped)
    crops["far"] = (paste_labels(1, S)[0] % 3, torch.ones(S, S), torch.full((S, S), 3.0))
    za = torch.full((S, S), 2.0)
    zb = torch.full((S, S), 1.5)
    zb[:, ::2] = 2.5
    crops["tie_a"] = (4.0 * half, torch.ones(S, S), za)
    crops["tie_b"] = (1.0 + 5.0 * half, torch.ones(S, S), zb)
    zn = torch.zeros(S, S)
    zn[:, 1::2] = -0.5
    crops["nan"] = (torch.full((S, S), 7.0), torch.ones(S, S), zn)
    roles = [ORDER_ROLES[p] for p in perm]
    depth = eighths(rng, (5, 3, S, S))
    for k, r in enumerate(roles):
        depth[k, 2] = crops[r][2]
    return dict(initial_masks=torch.zeros(1, H, W), labels_crop=torch.stack([crops[r][0] for r in roles]),
                mask=torch.stack([crops[r][1] for r in roles]),
                rois=torch.tensor([ORDER_BOXES[r] for r in roles], dtype=torch.float32), depth=depth, roles=roles)


ORDER_PERMS = ((0, 1, 2, 3, 4), (4, 1, 0, 3, 2), (1, 3, 4, 2, 0))


def stats_case(K, S=8, seed=26):
    """K random crops for uoc_roi_match_stats: ids 0..3 with a random mask (overlaps on both sides of 0.5), depth in
    eighths with a fifth of the pixels at z <= 0; every seventh ROI has no depth at all (NaN mean)."""
    rng = np.random.RandomState(seed + K)
    labels = torch.from_numpy(rng.randint(0, 4, size=(K, S, S)).astype(np.float32))
    mask = torch.from_numpy((rng.rand(K, S, S) < 0.5).astype(np.float32))
    depth = eighths(rng, (K, 3, S, S))
    depth[:, 2][torch.from_numpy(rng.rand(K, S, S) < 0.2)] = 0.0
    depth[6::7, 2] = -1.0
    return labels, mask, depth


def oracle_keep_meanz(labels_crop, mask, depth):
    """The two intermediate quantities of oracle.match_label_crop, computed by its own statements: keep [K,128] (cluster
    c of ROI k is not rejected) and the float32 sort key (mean z > 0 of the kept pixels, of all pixels if none is kept).
    tests/test_glue_cases_host.py ties `keep` to the -1 entries the oracle itself returns."""
    K = labels_crop.shape[0]
    keep = torch.zeros(K, 128, dtype=torch.int32)
    meanz = torch.zeros(K)
    out = labels_crop.clone()
    for i in range(K):
        for mid in torch.unique(labels_crop[i]):
            if mid < 0:         # pixels that are -1 on input belong to no cluster (the oracle leaves them at -1 either way)
                continue
            sel = labels_crop[i] == mid
            frac = torch.sum(sel.float() * mask[i]) / torch.sum(sel.float())
            if frac < 0.5:
                out[i][sel] = -1
            else:
                keep[i, int(mid)] = 1
        kept = out[i] > -1
        z = depth[i, 2][kept] if torch.sum(kept) > 0 else depth[i, 2]
        meanz[i] = torch.mean(z[z > 0])
    return keep, meanz, out


def match_raw_abi():
    """order_case() as int32 crop labels with ids outside [0, 128) scattered over every crop, most of them inside the
    stage-1 mask: taken modulo 128 they would be kept clusters 127, 0 and 16 and shift the renumbering.  The kernels
    count them for no cluster and paint nothing from them, which is what the oracle does with pixels that are -1 on input.
    -> the case, raw labels int32 [K,S,S], the same labels with those pixels at -1 (float32)."""
    c = order_case()
    rng = np.random.RandomState(27)
    raw = c["labels_crop"].to(torch.int32)
    hit = torch.from_numpy(rng.rand(*raw.shape) < 0.15)
    vals = torch.tensor(INVALID_IDS, dtype=torch.int64)[torch.from_numpy(rng.randint(0, len(INVALID_IDS), size=tuple(raw.shape)))]
    raw[hit] = vals[hit].to(torch.int32)
    clean = raw.float()
    clean[hit] = -1.0
    return c, raw, clean
