"""The definition of uoc_relations (include/uoc_hip.h) restated with numpy integers, a seeded tabletop
scene generator and the engineered frames the GPU tests run.  The pair tables are vectorised over shifted arrays (a
480x640 frame takes milliseconds); the relations, the peeling and the order are plain loops over the 128 ids.

    relations(lab, z, connectivity, gap_mm, min_pairs) -> dict: border, touch, front [128,128] int32 and one [128]
                                                          int32 array per field of uoc_relation_object (FIELDS)
"""
import numpy as np

NL = 128
FIELDS = ("pixels", "edge", "border_sum", "border_bg", "hidden", "n_touch", "n_above", "n_below", "layer", "free", "order")
TABLES = ("border", "touch", "front")
# (dy, dx) from a pixel to the neighbours it owns the pair with: every unordered pair once
FORWARD = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}


def ids_of(lab):
    lab = np.asarray(lab).astype(np.int64)
    return np.where((lab >= 1) & (lab <= NL - 1), lab, 0)


def depth_mm(z):
    """zq where the depth is valid, -1 elsewhere.  fp32 product, rounded half to even (np.rint)."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(z) & (z > 0) & (z <= np.float32(65.0))
        q = np.rint(np.where(valid, z, np.float32(0)) * np.float32(1000.0))
    return np.where(valid, q.astype(np.int64), -1)


def _shifted(arr, dy, dx):
    """(owner pixels, their neighbour at (dy, dx)) as two equally shaped views."""
    H, W = arr.shape
    if dx >= 0:
        return arr[:H - dy, :W - dx], arr[dy:, dx:]
    return arr[:H - dy, -dx:], arr[dy:, :W + dx]


def pair_tables(lab, z, connectivity, gap_mm):
    a_all, q_all = ids_of(lab), depth_mm(z)
    border, touch, front = (np.zeros(NL * NL, np.int64) for _ in range(3))
    for dy, dx in FORWARD[connectivity]:
        a, b = _shifted(a_all, dy, dx)
        qa, qb = _shifted(q_all, dy, dx)
        m = a != b
        a, b, qa, qb = a[m], b[m], qa[m], qb[m]
        border += np.bincount(a * NL + b, minlength=NL * NL) + np.bincount(b * NL + a, minlength=NL * NL)
        valid = (qa >= 0) & (qb >= 0)
        near = valid & (np.abs(qa - qb) < gap_mm)
        touch += np.bincount((a * NL + b)[near], minlength=NL * NL) + np.bincount((b * NL + a)[near], minlength=NL * NL)
        far = valid & ~near
        n = np.where(qa < qb, a, b)[far]
        f = np.where(qa < qb, b, a)[far]
        front += np.bincount(n * NL + f, minlength=NL * NL)
    return tuple(t.reshape(NL, NL) for t in (border, touch, front))


def occlusion_matrix(front, min_pairs):
    """occ[a][b]: a occludes b (ids 1..127)."""
    occ = (front >= min_pairs) & (front > front.T)
    occ[0, :] = occ[:, 0] = False
    return occ


def peel(present, occ):
    layer = np.zeros(NL, np.int64)
    r = 1
    while True:
        done = (layer > 0)
        new = [a for a in range(1, NL) if present[a] and layer[a] == 0 and not np.any(occ[:, a] & ~done)]
        if not new:
            break
        layer[new] = r
        r += 1
    layer[present & (layer == 0)] = -1
    return layer


def relations(lab, z, connectivity=4, gap_mm=15, min_pairs=8):
    lab = np.asarray(lab)
    H, W = lab.shape
    border, touch, front = pair_tables(lab, z, connectivity, gap_mm)
    ids = ids_of(lab)
    pixels = np.bincount(ids.ravel(), minlength=NL)
    on_edge = np.zeros((H, W), bool)
    on_edge[0, :] = on_edge[-1, :] = on_edge[:, 0] = on_edge[:, -1] = True
    edge = np.bincount(ids[on_edge], minlength=NL)
    present = pixels > 0
    present[0] = False
    occ = occlusion_matrix(front, min_pairs)
    tch = touch >= min_pairs
    tch[0, :] = tch[:, 0] = False
    layer = peel(present, occ)
    out = {k: np.zeros(NL, np.int64) for k in FIELDS}
    keys = sorted(((NL if layer[a] < 0 else layer[a]), a) for a in range(1, NL) if present[a])
    for rank, (_, a) in enumerate(keys, 1):
        out["order"][a] = rank
    for a in range(1, NL):
        if not present[a]:
            continue
        out["pixels"][a], out["edge"][a] = pixels[a], edge[a]
        out["border_sum"][a], out["border_bg"][a], out["hidden"][a] = border[a].sum(), border[a, 0], front[0, a]
        out["n_touch"][a], out["n_above"][a], out["n_below"][a] = tch[a].sum(), occ[:, a].sum(), occ[a].sum()
        out["layer"][a] = layer[a]
        out["free"][a] = int(out["n_above"][a] == 0 and out["hidden"][a] < min_pairs and edge[a] == 0)
    out = {k: v.astype(np.int32) for k, v in out.items()}
    out.update(border=border.astype(np.int32), touch=touch.astype(np.int32), front=front.astype(np.int32))
    return out


def xyz_of(z):
    """[3,H,W] float32 with z in channel 2; x and y are pixel rays of a 500-pixel focal length (not read by the step)."""
    z = np.asarray(z, dtype=np.float32)
    H, W = z.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(u - W / 2) * z / 500, (v - H / 2) * z / 500, z]).astype(np.float32)


# ---- seeded scenes -----------------------------------------------------------------------------------------------------
def tabletop(H, W, seed, noise=0.001, holes=0.05):
    """A table (z growing towards the top of the image) with rectangles and ellipses painted far to near, 4 cm apart in
    depth: 1 and 2 overlap (2 occludes 1), 3 and 4 stand side by side at one depth (they touch), 5 is cut by the left
    image edge, then three seeded ellipses in front of all of them.  Millimetre noise, 5 % zero-depth holes.
    Returns (labels [H,W] int32, xyz [3,H,W] float32)."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    fy, fx = (yy + 0.5) / H, (xx + 0.5) / W
    lab = np.zeros((H, W), np.int32)
    z = (1.0 + 0.1 * (1.0 - fy)).astype(np.float64)

    def rect(x0, x1, y0, y1):
        return (fx >= x0) & (fx < x1) & (fy >= y0) & (fy < y1)

    def ellipse(cx, cy, rx, ry):
        return ((fx - cx) / rx) ** 2 + ((fy - cy) / ry) ** 2 <= 1.0

    shapes = [rect(0.10, 0.45, 0.15, 0.55), ellipse(0.45, 0.55, 0.15, 0.20), rect(0.55, 0.70, 0.10, 0.45),
              rect(0.70, 0.85, 0.10, 0.45), rect(0.0, 0.12, 0.60, 0.90)]
    depths = [0.90, 0.86, 0.82, 0.82, 0.78]
    for k in range(3):
        shapes.append(ellipse(rng.uniform(0.2, 0.9), rng.uniform(0.3, 0.9), rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.15)))
        depths.append(0.74 - 0.04 * k)
    for k, (m, d) in enumerate(zip(shapes, depths), 1):
        lab[m] = k
        z[m] = d
    z += rng.normal(0.0, noise, size=z.shape)
    z[rng.random(z.shape) < holes] = 0.0
    return lab, xyz_of(z)


def checkerboard(H, W):
    """Ids 1 and 2 alternating, id 1 ten centimetres nearer: every pair of two ids that a block sees falls into one
    cell of each table (the counter-width case; the diagonal neighbours carry the pixel's own id)."""
    yy, xx = np.mgrid[0:H, 0:W]
    odd = ((yy + xx) & 1).astype(bool)
    return np.where(odd, 2, 1).astype(np.int32), xyz_of(np.where(odd, 0.6, 0.5))


def row_stripes(H, W):
    """Ids 1 and 2 in alternating rows, id 1 nearer: at connectivity 8 three of a pixel's four pairs fall into one cell,
    the most two ids can reach."""
    odd = (np.mgrid[0:H, 0:W][0] & 1).astype(bool)
    return np.where(odd, 2, 1).astype(np.int32), xyz_of(np.where(odd, 0.6, 0.5))


# ---- engineered frames -------------------------------------------------------------------------------------------------
def strips(H, specs):
    """Vertical strips side by side.  spec = (id, width, z) or (id, width, z, rows): the strip's top `rows` rows carry
    the id, the rest of the column block is background at depth 2.0."""
    W = sum(s[1] for s in specs)
    lab, z = np.zeros((H, W), np.int32), np.full((H, W), 2.0)
    x = 0
    for s in specs:
        rows = s[3] if len(s) > 3 else H
        lab[:rows, x:x + s[1]] = s[0]
        z[:rows, x:x + s[1]] = s[2]
        x += s[1]
    return lab, z


def _case(lab, z, connectivity=4, gap_mm=15, min_pairs=1):
    return dict(lab=np.asarray(lab, np.int32), xyz=xyz_of(z), connectivity=connectivity, gap_mm=gap_mm, min_pairs=min_pairs)


def case_one_by_one():
    return _case([[5]], [[1.0]])


def case_pair_h():
    return _case([[1, 2]], [[1.0, 1.1]])


def case_pair_v():
    return _case([[1], [2]], [[1.1], [1.0]])


def case_chain5():
    """1 occludes 2 occludes ... 5: layers 1..5."""
    return _case(*strips(10, [(k, 4, 0.4 + 0.1 * k) for k in range(1, 6)]), min_pairs=8)


def case_cycle():
    """1 in front of 2, 2 in front of 3, 3 in front of (the second strip of) 1, and 4 behind 1: all four get layer -1."""
    return _case(*strips(10, [(1, 3, 0.5), (2, 3, 0.6), (3, 3, 0.7), (1, 3, 0.8), (4, 3, 0.9)]), min_pairs=8)


def case_tie():
    """front[1][2] == front[2][1] == 4: neither occludes the other."""
    lab, z = strips(8, [(1, 3, 0.5), (2, 3, 0.6)])
    z[4:, :3], z[4:, 3:] = 0.6, 0.5
    return _case(lab, z, min_pairs=4)


def case_at_min_pairs():
    """min_pairs = 5.  front[1][2] = 5 (occludes), front[3][4] = 4 (does not); touch[5][6] = 5, touch[7][8] = 4."""
    return _case(*strips(6, [(1, 2, 0.5, 5), (2, 2, 0.6, 5), (0, 2, 2.0), (3, 2, 0.5, 4), (4, 2, 0.6, 4), (0, 2, 2.0),
                             (5, 2, 0.7, 5), (6, 2, 0.7, 5), (0, 2, 2.0), (7, 2, 0.7, 4), (8, 2, 0.7, 4)]), min_pairs=5)


def case_at_gap():
    """gap_mm = 15.  zq 500 against 515: in front; 500 against 514: touching."""
    return _case(*strips(4, [(1, 2, 0.500), (2, 2, 0.515), (0, 2, 2.0), (3, 2, 0.500), (4, 2, 0.514)]), min_pairs=4)


def case_bad_depth():
    """Every second pixel of the rows has a depth that is NaN, inf, 0, negative, exactly 65.0 (valid) or just above
    (invalid); their neighbours are valid."""
    above = np.nextafter(np.float32(65.0), np.float32(np.inf))
    odd = [np.nan, np.inf, 0.0, -1.0, 65.0, above, -np.inf, 1e-9]
    lab = np.tile(np.array([1, 2], np.int32), (2, len(odd)))
    z = np.empty((2, 2 * len(odd)), np.float32)
    z[0, 0::2], z[0, 1::2] = odd, 64.9
    z[1, 0::2], z[1, 1::2] = 64.99, odd[::-1]
    return _case(lab, z, connectivity=8)


def case_bad_labels():
    """0, 128, -1 and 1000 are all id 0: no pair among them, pairs against the ids 1 and 127."""
    lab = [[0, 128, -1, 1000, 1, 127], [128, 1, 1, -1, 127, 0], [1000, 0, 127, 128, -1, 1]]
    z = 1.0 + 0.02 * np.arange(18).reshape(3, 6)
    return _case(lab, z, connectivity=8)


def case_one_id():
    return _case(np.full((9, 13), 7), np.full((9, 13), 0.8))


def case_stripes127():
    """127 ids in stripes, each 2 cm behind its left neighbour: a chain of 127 layers."""
    return _case(*strips(6, [(k, 2, 0.5 + 0.02 * k) for k in range(1, 128)]), min_pairs=6)


def case_checkerboard():
    lab, xyz = checkerboard(16, 16)
    return dict(lab=lab, xyz=xyz, connectivity=8, gap_mm=15, min_pairs=8)


ENGINEERED = {"one_by_one": case_one_by_one, "pair_h": case_pair_h, "pair_v": case_pair_v, "chain5": case_chain5,
              "cycle": case_cycle, "tie": case_tie, "at_min_pairs": case_at_min_pairs, "at_gap": case_at_gap,
              "bad_depth": case_bad_depth, "bad_labels": case_bad_labels, "one_id": case_one_id,
              "stripes127": case_stripes127, "checkerboard": case_checkerboard}
