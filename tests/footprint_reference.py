"""The definition of uoc_footprint (include/uoc_hip.h) restated with numpy integers, and the grids the
tests run it on.  Nothing here comes from the package's footprint, grasp or placement modules: every constant is written
out, so a wrong constant in the package fails a test.

`footprint` is the restatement the GPU tests compare with (one span per mask row, runs of FREE cells, slices of the run
table); `footprint_literal` follows the definition offset by offset and is what tests/test_footprint_host.py holds
`footprint` against."""
import numpy as np

S = 16384
UNIT = 256
MAX_HALF = 16384
MAX_RECTS = 8
MAX_DIRS = 32
MAX_ANCHOR = 4096
ROOMIEST, NEAREST = 0, 1
IDX_MASK = 0x3FFFF
DIST_CAP = 65536
NO_POSE = (0, -1, -1, -1, 0, 0, 0, 0)
INFLATE = 184                                                   # what rect(conservative=True) adds: 0.71875 cell


def direction_table(A):
    k = np.arange(A, dtype=np.float64)
    return np.stack([np.rint(np.cos(np.pi * k / A) * S), np.rint(np.sin(np.pi * k / A) * S)], axis=1).astype(np.int64)


def record(HL, HW, ignore=0, mode=ROOMIEST, ai=0, aj=0):
    return (int(HL), int(HW), int(ignore), int(mode), int(ai), int(aj), 0, 0)


def radius(HL, HW):
    """R: the smallest integer with (256 R)^2 >= HL^2 + HW^2."""
    q, R = HL * HL + HW * HW, 0
    while (UNIT * R) ** 2 < q:
        R += 1
    return R


def check_params(dirs, rects, unknown_blocks):
    dirs = np.asarray(dirs, np.int64)
    assert dirs.ndim == 2 and dirs.shape[1] == 2 and 1 <= len(dirs) <= MAX_DIRS and np.abs(dirs).max() <= S
    assert 1 <= len(rects) <= MAX_RECTS and unknown_blocks in (0, 1)
    for r in rects:
        HL, HW, ignore, mode, ai, aj, z6, z7 = (int(x) for x in r)
        assert 0 <= HL <= MAX_HALF and 0 <= HW <= MAX_HALF and HL * HL + HW * HW <= MAX_HALF * MAX_HALF
        assert 0 <= ignore <= 127 and mode in (ROOMIEST, NEAREST) and z6 == 0 and z7 == 0
        assert -MAX_ANCHOR <= ai < MAX_ANCHOR and -MAX_ANCHOR <= aj < MAX_ANCHOR


def mask_offsets(dirs, k, HL, HW, window=None):
    """The offsets of M as a list of (di, dj), by the definition, over |di|, |dj| <= window (R + 1 when None)."""
    cx, cy = int(dirs[k][0]), int(dirs[k][1])
    w = radius(HL, HW) + 1 if window is None else window
    return [(di, dj) for di in range(-w, w + 1) for dj in range(-w, w + 1)
            if abs(di * cx + dj * cy) <= 64 * HL and abs(-di * cy + dj * cx) <= 64 * HW]


def mask_spans(dirs, k, HL, HW):
    """{di: (dj_lo, dj_hi)} of the non-empty rows of M: the smallest and the largest dj of the row."""
    rows = {}
    for di, dj in mask_offsets(dirs, k, HL, HW):
        lo, hi = rows.get(di, (dj, dj))
        rows[di] = (min(lo, dj), max(hi, dj))
    return rows


def free_cells(state, owner, ignore, unknown_blocks):
    """[G,G] bool: the cells that are FREE for a rectangle with this `ignore`."""
    st, ow = np.asarray(state).astype(np.int64), np.asarray(owner).astype(np.int64)
    obstacle = (st == 2) & (ow >= 1) & (ow <= 127)
    unknown = ~obstacle & (st != 1)
    free = (st == 1) | (unknown & (not unknown_blocks))
    if ignore >= 1:
        free |= obstacle & (ow == ignore)
    return free


def runs_of(free):
    """[G,G] int64: the length of the run of FREE cells that ends at each cell, along j."""
    G = free.shape[1]
    j = np.arange(G, dtype=np.int64)[None, :]
    last_blocked = np.maximum.accumulate(np.where(free, -1, j), axis=1)
    return np.where(free, j - last_blocked, 0)


def key_of(mode, d, da, idx, k):
    top = (d + 1) if mode == ROOMIEST else ((1 << 27) - 1 - da)
    return (top << 23) | ((IDX_MASK - idx) << 5) | (31 - k)


def _finish(words, dist2, rects, A, found):
    """fits, count and best from the per-rectangle uint32 words [F,G,G]."""
    F, G = words.shape[0], words.shape[1]
    if not found:
        words = np.zeros_like(words)
    count = np.zeros((F, 32), np.int32)
    best = np.zeros((F, 8), np.int32)
    d = np.clip(np.asarray(dist2).astype(np.int64), 0, DIST_CAP)
    I, J = np.meshgrid(np.arange(G, dtype=np.int64), np.arange(G, dtype=np.int64), indexing="ij")
    idx = I * G + J
    for f in range(F):
        w = words[f].astype(np.int64)
        for k in range(32):
            count[f, k] = int(((w >> k) & 1).sum())
        assert not count[f, A:].any()
        mode, ai, aj = (int(x) for x in rects[f][3:6])
        hit = w != 0
        if not hit.any():
            best[f] = NO_POSE
            continue
        low = (w & -w)                                         # the lowest set bit: the lowest k carries the largest key
        k0 = np.zeros_like(w)
        for k in range(32):
            k0[low == (1 << k)] = k
        da = (I - ai) ** 2 + (J - aj) ** 2
        top = (d + 1) if mode == ROOMIEST else ((1 << 27) - 1 - da)
        key = np.where(hit, (top << 23) | ((IDX_MASK - idx) << 5) | (31 - k0), 0)
        c = int(np.argmax(key))                                 # strict total order: one maximum
        i, j = divmod(c, G)
        best[f] = (1, i, j, int(k0[i, j]), int(d[i, j]), int(da[i, j]), int(count[f].sum()), int(hit.sum()))
    return {"fits": words.astype(np.uint32).view(np.int32), "count": count, "best": best}


def _found(frame):
    return frame is None or int(np.asarray(frame).reshape(-1)[13]) == 1


def footprint(state, owner, dist2, dirs, rects, unknown_blocks, frame=None):
    """One frame: state, owner, dist2 [G,G] integer arrays, dirs [A,2], rects [F][8], frame None or the 16 int64 words.
    Returns {"fits": [F,G,G] int32, "count": [F,32] int32, "best": [F,8] int32}.  The span and run form."""
    dirs = np.asarray(dirs, np.int64)
    check_params(dirs, rects, unknown_blocks)
    G, A, F = np.asarray(state).shape[0], len(dirs), len(rects)
    words = np.zeros((F, G, G), np.uint32)
    for f, r in enumerate(rects):
        HL, HW, ignore = int(r[0]), int(r[1]), int(r[2])
        free = free_cells(state, owner, ignore, unknown_blocks)
        run = runs_of(free)
        for k in range(A):
            rows = mask_spans(dirs, k, HL, HW)
            dmax = max(abs(di) for di in rows)
            lo_min, hi_max = min(lo for lo, _ in rows.values()), max(hi for _, hi in rows.values())
            i0, i1, j0, j1 = dmax, G - dmax, -lo_min, G - hi_max          # the centres whose spans all lie inside the grid
            if i0 >= i1 or j0 >= j1:
                continue
            ok = np.ones((i1 - i0, j1 - j0), bool)
            for di, (lo, hi) in rows.items():
                ok &= run[i0 + di:i1 + di, j0 + hi:j1 + hi] >= hi - lo + 1
                if not ok.any():
                    break
            words[f, i0:i1, j0:j1] |= ok.astype(np.uint32) << np.uint32(k)
    return _finish(words, dist2, rects, A, _found(frame))


def footprint_literal(state, owner, dist2, dirs, rects, unknown_blocks, frame=None, window=None):
    """The definition followed offset by offset: bit k is set iff every cell of the mask lies inside the grid and is FREE."""
    dirs = np.asarray(dirs, np.int64)
    check_params(dirs, rects, unknown_blocks)
    G, A, F = np.asarray(state).shape[0], len(dirs), len(rects)
    words = np.zeros((F, G, G), np.uint32)
    for f, r in enumerate(rects):
        HL, HW, ignore = int(r[0]), int(r[1]), int(r[2])
        free = free_cells(state, owner, ignore, unknown_blocks)
        P = (window if window is not None else radius(HL, HW) + 1)
        padded = np.zeros((G + 2 * P, G + 2 * P), bool)          # a cell outside the grid is never FREE
        padded[P:P + G, P:P + G] = free
        for k in range(A):
            ok = np.ones((G, G), bool)
            for di, dj in mask_offsets(dirs, k, HL, HW, window):
                ok &= padded[P + di:P + di + G, P + dj:P + dj + G]
            words[f] |= ok.astype(np.uint32) << np.uint32(k)
    return _finish(words, dist2, rects, A, _found(frame))


def batch(states, owners, dist2s, dirs, rects, unknown_blocks, frames=None):
    """`footprint` per frame, stacked: fits [B,F,G,G], count [B,F,32], best [B,F,8]."""
    outs = [footprint(states[b], owners[b], dist2s[b], dirs, rects, unknown_blocks, None if frames is None else frames[b])
            for b in range(len(states))]
    return {k: np.stack([o[k] for o in outs]) for k in ("fits", "count", "best")}


# ---- grids ------------------------------------------------------------------------------------------------------------
def table(G, fill=1):
    return np.full((G, G), fill, np.int32), np.zeros((G, G), np.int32)


def clearance(state, owner, unknown_blocks=1):
    """A dist2 grid in the manner of uoc_placement: the exact squared distance to the nearest cell that is not FREE (no
    ignore), the cells outside the grid included, capped by nothing.  Brute force over rows: small grids only matter."""
    free = free_cells(state, owner, 0, unknown_blocks)
    G = free.shape[0]
    P = np.zeros((G + 2, G + 2), bool)
    P[1:-1, 1:-1] = free
    bi, bj = np.nonzero(~P)
    I, J = np.meshgrid(np.arange(1, G + 1), np.arange(1, G + 1), indexing="ij")
    out = np.full((G, G), np.iinfo(np.int64).max, np.int64)
    for s in range(0, len(bi), 4096):
        d = (I[..., None] - bi[s:s + 4096]) ** 2 + (J[..., None] - bj[s:s + 4096]) ** 2
        out = np.minimum(out, d.min(axis=-1))
    return out.astype(np.int32)


def seeded_dist2(G, seed):
    """dist2 values for grids where the geometry is beside the point: 0..G*G/4 with -1 and 70000 sprinkled in."""
    rng = np.random.default_rng(1000 + seed)
    d = rng.integers(0, max(2, G * G // 4), (G, G)).astype(np.int32)
    odd = rng.random((G, G)) < 0.05
    d[odd] = rng.choice(np.array([-1, 70000, 65536, 65537], np.int32), int(odd.sum()))
    return d


def random_grid(G, seed, noise=0.03):
    """A seeded grid in the manner of tests/grasp_reference.py: table with patches of unknown, 3-6 convex blobs with ids
    from 1..127 and `noise` of the cells redrawn at random: states -1..3 and owners -5..129 (out-of-contract values
    included).  Returns state, owner, dist2."""
    rng = np.random.default_rng(seed)
    st, ow = table(G)
    I, J = np.meshgrid(np.arange(G) + .5, np.arange(G) + .5, indexing="ij")
    for _ in range(3):
        ci, cj, r = rng.uniform(0, G, 2).tolist() + [rng.uniform(1, max(2, G / 6))]
        st[(I - ci) ** 2 + (J - cj) ** 2 <= r * r] = 0
    for a in rng.choice(np.arange(1, 128), size=int(rng.integers(3, 7)), replace=False):
        ci, cj = rng.uniform(0, G, 2)
        ra, rb = rng.uniform(0.6, max(1.0, G / 8)), rng.uniform(0.6, max(1.0, G / 20))
        th = rng.uniform(0, np.pi)
        u, v = (I - ci) * np.cos(th) + (J - cj) * np.sin(th), -(I - ci) * np.sin(th) + (J - cj) * np.cos(th)
        mask = ((u / ra) ** 2 + (v / rb) ** 2 <= 1) if rng.random() < 0.5 else ((abs(u) <= ra) & (abs(v) <= rb))
        st[mask], ow[mask] = 2, int(a)
    redraw = rng.random((G, G)) < noise
    st[redraw] = rng.integers(-1, 4, int(redraw.sum()))
    ow[redraw] = rng.choice(np.concatenate([[-5, 0, 128, 129], np.unique(ow[ow > 0])]), int(redraw.sum()))
    return st, ow, seeded_dist2(G, seed)


def present_id(owner, state):
    ids = np.unique(owner[(state == 2) & (owner >= 1) & (owner <= 127)])
    return int(ids[0]) if len(ids) else 1


def corridor(G, width, along_i=True, at=None):
    """Obstacle (id 3) everywhere but a corridor of table `width` cells wide through the whole grid."""
    st, ow = table(G, 2)
    ow[:] = 3
    a = (G - width) // 2 if at is None else at
    if along_i:
        st[:, a:a + width], ow[:, a:a + width] = 1, 0
    else:
        st[a:a + width, :], ow[a:a + width, :] = 1, 0
    return st, ow


def bar8():
    """The hand-counted case: an 8x8 grid of obstacle (id 3) with a corridor of table in columns 3..5 (3 cells wide)
    through all 8 rows, and the 3x1-cell bar HL = 256, HW = 0 at A = 2.  k = 0 (along i): the mask is (-1,0), (0,0),
    (1,0): rows 1..6 of the three columns: 18 cells.  k = 1 (along j): (0,-1), (0,0), (0,1): column 4 only, all 8 rows:
    8 cells.  26 poses on 18 + 2 = 20 cells (rows 0 and 7 of column 4 fit only across)."""
    return corridor(8, 3, along_i=True, at=3)


def case_one_blocker(G=32):
    st, ow = table(G)
    st[G // 2, G // 2 + 1], ow[G // 2, G // 2 + 1] = 2, 9
    return st, ow


def case_one_orientation(G=32):
    """A slot of table 1 cell wide and 17 long along j in a grid of obstacle: a 15x1-cell bar (HL = 1920, HW = 128) fits
    only along j; a bar of no width (HW = 0) has, off the axes, hardly a lattice point but its centre and fits anyhow."""
    st, ow = table(G, 2)
    ow[:] = 5
    st[15:16, 6:23], ow[15:16, 6:23] = 1, 0
    return st, ow


def case_last_row_column(G=16):
    """Obstacle but for the last two rows and the last two columns: footprints that touch row G-1 and column G-1."""
    st, ow = table(G, 2)
    ow[:] = 2
    st[G - 2:, :], ow[G - 2:, :] = 1, 0
    st[:, G - 2:], ow[:, G - 2:] = 1, 0
    return st, ow


def case_only_obstacle(G=24):
    """One 4x6 box of id 7 on a table."""
    st, ow = table(G)
    st[10:14, 8:14], ow[10:14, 8:14] = 2, 7
    return st, ow


def case_out_of_contract(G=24):
    """Table with state-2 cells of owner 0, 128 and -5 and cells of state 3 and -1: all unknown; a cell of owner 7 whose
    state is 1 is table."""
    st, ow = table(G)
    st[4, 4], ow[4, 4] = 2, 0
    st[4, 12], ow[4, 12] = 2, 128
    st[12, 4], ow[12, 4] = 2, -5
    st[12, 12] = 3
    st[18, 18], ow[18, 18] = -1, 7
    st[18, 6], ow[18, 6] = 1, 7
    st[20, 12], ow[20, 12] = 2, 7
    return st, ow


ENGINEERED = {
    "empty_table": lambda: table(32),
    "all_obstacle": lambda: (np.full((16, 16), 2, np.int32), np.full((16, 16), 4, np.int32)),
    "all_unknown": lambda: table(16, 0),
    "one_blocker": case_one_blocker,
    "corridor_i_5": lambda: corridor(32, 5, True),
    "corridor_i_4": lambda: corridor(32, 4, True),
    "corridor_j_5": lambda: corridor(32, 5, False),
    "corridor_j_4": lambda: corridor(32, 4, False),
    "one_orientation": case_one_orientation,
    "last_row_column": case_last_row_column,
    "only_obstacle": case_only_obstacle,
    "out_of_contract": case_out_of_contract,
    "bar8": bar8,
}

# (A, rects): the parameter sets the engineered grids run under.  5x1.. cells: HL = 512 + 128 covers di = -2..2.
ENGINEERED_SETS = [
    (2, [record(640, 0), record(0, 0)]),                                       # a 5-cell bar, exactly as wide as corridor_*_5; a point
    (16, [record(640, 384), record(1024, 128, ignore=7), record(1024, 128, ignore=9)]),
    (5, [record(256, 256, mode=NEAREST, ai=-40, aj=4000), record(700, 0, ignore=3, mode=NEAREST, ai=5, aj=5)]),
    (1, [record(1800, 0), record(0, 1800, ignore=127)]),
    (32, [record(640, 0, mode=NEAREST, ai=4095, aj=-4096)]),                   # bit 31
]

# Six sets that reach every limit: A = 1 and 32, F = 1 and 8, HL, HW = 0 and the limits, ignore 0 / present / absent / 127,
# both modes, anchors at both ends, both unknown_blocks.  `P` stands for an id that is present on the grid.
RANDOM_SETS = [
    (16, [("rec", 1024, 256, 0, ROOMIEST, 0, 0)], 1),
    (32, [("rec", 16384, 0, 0, ROOMIEST, 0, 0), ("rec", 0, 16384, "P", NEAREST, -4096, 4095), ("rec", 11585, 11585, 0, ROOMIEST, 0, 0),
          ("rec", 0, 0, 0, NEAREST, 4095, -4096), ("rec", 300, 300, "P", ROOMIEST, 0, 0), ("rec", 2000, 255, 127, NEAREST, 3, 200),
          ("rec", 255, 255, 126, ROOMIEST, 0, 0), ("rec", 4000, 900, "P", NEAREST, 100, 100)], 1),
    (1, [("rec", 700, 300, "P", NEAREST, 2, 2)], 0),
    (5, [("rec", 512, 0, 0, ROOMIEST, 0, 0), ("rec", 0, 512, 0, ROOMIEST, 0, 0), ("rec", 513, 1, "P", ROOMIEST, 0, 0)], 0),
    (32, [("rec", 1300, 400, "P", ROOMIEST, 0, 0), ("rec", 1300, 400, 0, NEAREST, -1, -1)], 0),
    (7, [("rec", 3000, 128, 0, NEAREST, 0, 511), ("rec", 128, 3000, "P", ROOMIEST, 0, 0), ("rec", 184, 184, 0, ROOMIEST, 0, 0),
         ("rec", 8000, 0, "P", ROOMIEST, 0, 0), ("rec", 0, 0, "P", ROOMIEST, 0, 0), ("rec", 16383, 1, 0, ROOMIEST, 0, 0),
         ("rec", 1, 16383, 0, ROOMIEST, 0, 0), ("rec", 600, 600, 1, NEAREST, 7, 7)], 1),
]


def resolve(rect_specs, present):
    return [record(HL, HW, present if ig == "P" else ig, mode, ai, aj) for _, HL, HW, ig, mode, ai, aj in rect_specs]


def flat_frame(found=1):
    """A frame record of the plane z = 1 m seen from above: N, D, U, V, qc and `found`."""
    F = np.zeros(16, np.int64)
    F[0:3], F[3] = (0, 0, -S), 1000 * S
    F[4:7], F[7:10], F[10:13], F[13] = (S, 0, 0), (0, -S, 0), (0, 0, 1000), found
    return F
