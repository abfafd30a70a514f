"""Plain Python / numpy restatement of uoc_placement (include/uoc_hip.h): the semantics the GPU tests check against.
Integers only (int64 arrays and Python ints); the distance transform is done separably (a column pass with
accumulate, a row pass over shifted arrays), `edt_brute` is the all-pairs definition it is checked against.  Also the
seeded tabletop scenes and the engineered frames of the GPU tests; tests/test_placement_host.py asserts that they
contain what they are used for."""
import numpy as np

from tests import support_reference as S13

NUM_IDS = 128
Q_MAX = 32767
S = 16384
WIDEST, NEAREST = 0, 1
NO_ANSWER = (-1, -1, 0, 0)
IGNORED, TABLE, OBSTACLE = -1, 0, 1


# ---- F: the frame in integers -------------------------------------------------------------------------------------------
def plane_from_record(rec):
    """A uoc_plane record (21 int32 words) -> dict found, normal, d, centroid, u, v (float32)."""
    rec = np.ascontiguousarray(rec, np.int32)
    f = rec.view(np.float32)
    return dict(found=int(rec[0]), normal=f[4:7].copy(), d=f[7].copy(), centroid=f[8:11].copy(), u=f[15:18].copy(), v=f[18:21].copy())


def frame_record(plane):
    """int64 [16]: N[3], D, U[3], V[3], qc[3], found, 0, 0 -- all zero for a frame without a usable plane."""
    F = np.zeros(16, np.int64)
    if plane is None or int(plane["found"]) != 1:
        return F
    n, u, v, c = (np.asarray(plane[k], np.float32).reshape(3) for k in ("normal", "u", "v", "centroid"))
    d = np.float32(plane["d"])
    with np.errstate(invalid="ignore", over="ignore"):
        unit = np.concatenate([n, u, v])
        if not (np.isfinite(unit).all() and (np.abs(unit) <= np.float32(2.0)).all() and np.isfinite(d) and abs(d) <= np.float32(1000.0)):
            return F
        if not np.isfinite(c).all():
            return F
        qc = np.rint(c * np.float32(1000.0))                   # fp32 product, round half to even
        if not (np.abs(qc) <= Q_MAX).all():
            return F
    F[0:3] = np.rint(n.astype(np.float64) * 16384.0).astype(np.int64)
    F[3] = int(np.rint(np.float64(d) * 16384000.0))
    F[4:7] = np.rint(u.astype(np.float64) * 16384.0).astype(np.int64)
    F[7:10] = np.rint(v.astype(np.float64) * 16384.0).astype(np.int64)
    F[10:13] = qc.astype(np.int64)
    F[13] = 1
    return F


# ---- P: points ------------------------------------------------------------------------------------------------------------
def point_events(labels, xyz, F, G, cell_mm, h_obs_mm, tau_mm):
    """Per pixel, flat in raster order: dict part (bool: takes part), outside (bool), i, j (int64, cell; meaningful where
    part), cls (IGNORED / TABLE / OBSTACLE; IGNORED where outside), id (0..127), T (int64)."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    X = np.asarray(xyz, np.float32).reshape(3, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        part = np.isfinite(X).all(axis=0) & (X[2] > 0)
        r = np.rint(X * np.float32(1000.0))
        part &= (np.abs(r) <= Q_MAX).all(axis=0)
    q = np.where(part, r, 0).astype(np.int64)
    N, D, U, V, qc = F[0:3], int(F[3]), F[4:7], F[7:10], F[10:13]
    T = N @ q + D
    rel = q - qc[:, None]
    div = cell_mm * S
    i = (U @ rel) // div + G // 2                                # numpy's // on int64 floors towards minus infinity
    j = (V @ rel) // div + G // 2
    inside = (i >= 0) & (i < G) & (j >= 0) & (j < G)
    ident = np.where((lab >= 1) & (lab < NUM_IDS), lab, 0)
    cls = np.full(lab.shape, IGNORED, np.int64)
    live = part & inside & (T >= -tau_mm * S)
    obstacle = live & ((ident != 0) | (T > h_obs_mm * S))
    cls[obstacle] = OBSTACLE
    cls[live & ~obstacle & (T <= tau_mm * S)] = TABLE
    return dict(part=part, outside=part & ~inside, i=i, j=j, cls=cls, id=ident, T=T)


def raster(ev, G):
    """(n_obs, n_table, owner [G,G] int64, outside) from point_events."""
    n_obs, n_table, owner = (np.zeros(G * G, np.int64) for _ in range(3))
    cell = ev["i"] * G + ev["j"]
    ob, tb = ev["cls"] == OBSTACLE, ev["cls"] == TABLE
    np.add.at(n_obs, cell[ob], 1)
    np.add.at(n_table, cell[tb], 1)
    np.maximum.at(owner, cell[ob], ev["id"][ob])
    return n_obs.reshape(G, G), n_table.reshape(G, G), owner.reshape(G, G), int(ev["outside"].sum())


def atomic_events(ev, G, group):
    """(before, after): the atomic operations of the raster pass if every point issued its own (one count event per
    table or obstacle point, one owner event per labelled obstacle point), and after every wave has merged the equal
    events of its `group` consecutive pixels (256 with vector loads, 64 without)."""
    cell = ev["i"] * G + ev["j"]
    live = ev["cls"] != IGNORED
    cnt = np.where(live, cell * 2 + (ev["cls"] == OBSTACLE), -1)
    own = np.where((ev["cls"] == OBSTACLE) & (ev["id"] > 0), cell * NUM_IDS + ev["id"], -1)
    before = int((cnt >= 0).sum() + (own >= 0).sum())
    after = 0
    wave = np.arange(len(cell)) // group
    for code in (cnt, own):
        keep = code >= 0
        after += len(np.unique(np.stack([wave[keep], code[keep]]), axis=1).T)
    return before, after


# ---- C, E: cells and clearance -----------------------------------------------------------------------------------------
def cell_states(n_obs, n_table, owner, min_pts):
    state = np.where(n_obs >= min_pts, 2, np.where(n_table >= min_pts, 1, 0)).astype(np.int64)
    own = np.where(state == 2, owner, 0)
    cells = np.bincount(own[state == 2].reshape(-1), minlength=NUM_IDS).astype(np.int64)
    cells[0] = 0
    return state, own, cells


def edt_brute(blocking):
    """All pairs: the smallest squared distance to a blocking cell, every cell outside the grid blocking."""
    G = blocking.shape[0]
    pad = np.ones((G + 2, G + 2), bool)
    pad[1:-1, 1:-1] = blocking
    bi, bj = np.nonzero(pad)
    out = np.zeros((G, G), np.int64)
    for i in range(G):
        for j in range(G):
            out[i, j] = int(((bi - 1 - i) ** 2 + (bj - 1 - j) ** 2).min())
    return out


def column_distance(blocking):
    """g[i][j]: the distance along i to the nearest blocking cell of column j, the virtual ones at -1 and G included."""
    G = blocking.shape[0]
    idx = np.arange(G)[:, None]
    up = np.maximum.accumulate(np.where(blocking, idx, -1), axis=0)
    down = np.minimum.accumulate(np.where(blocking, idx, G)[::-1], axis=0)[::-1]
    return np.minimum(idx - up, down - idx).astype(np.int64)


def edt(blocking):
    G = blocking.shape[0]
    g2 = np.zeros((G, G + 2), np.int64)                         # the virtual columns -1 and G: g = 0
    g2[:, 1:-1] = column_distance(blocking) ** 2
    col = np.arange(G)
    best = np.minimum((col + 1) ** 2, (G - col) ** 2)[None, :].repeat(G, axis=0)
    for off in range(-(G // 2), G // 2 + 1):                    # dist2 <= (G/2)^2: farther columns cannot win
        src = col + off
        ok = (src >= 0) & (src < G)
        best[:, ok] = np.minimum(best[:, ok], g2[:, 1:-1][:, src[ok]] + off * off)
    return best


# ---- Q: queries --------------------------------------------------------------------------------------------------------------
def answer(state, dist2, query):
    need2, ai, aj, mode = (int(x) for x in query)
    G = state.shape[0]
    ii, jj = np.nonzero(state == 1)
    d2 = dist2[ii, jj].astype(np.int64)
    if mode == NEAREST:
        ok = d2 >= need2
        ii, jj, d2 = ii[ok], jj[ok], d2[ok]
    if len(ii) == 0:
        return NO_ANSWER
    if mode == WIDEST:                                           # lexsort: the last key is the primary one
        k = np.lexsort((ii * G + jj, -d2))[0]
        return int(ii[k]), int(jj[k]), int(d2[k]), int(d2[k] >= need2)
    k = np.lexsort((ii * G + jj, -d2, (ii - ai) ** 2 + (jj - aj) ** 2))[0]
    return int(ii[k]), int(jj[k]), int(d2[k]), 1


def contenders(state, dist2, query):
    """How many candidates share the winner's first criterion (more than one: the tie rule decides)."""
    need2, ai, aj, mode = (int(x) for x in query)
    ii, jj = np.nonzero(state == 1)
    d2 = dist2[ii, jj]
    if mode == WIDEST:
        return int((d2 == d2.max()).sum()) if len(d2) else 0
    ok = d2 >= need2
    da = (ii[ok] - ai) ** 2 + (jj[ok] - aj) ** 2
    return int((da == da.min()).sum()) if len(da) else 0


def free_space(labels, xyz, plane, G, cell_mm, h_obs_mm, tau_mm, min_pts, unknown_blocks, queries=()):
    """One frame.  Returns dict state, owner, dist2 [G,G] int32, counts [128] int32, frame [16] int64, answers [Q,4] int32."""
    F = frame_record(plane)
    Q = len(queries)
    if not F[13]:
        z = np.zeros((G, G), np.int32)
        return dict(state=z, owner=z.copy(), dist2=z.copy(), counts=np.zeros(NUM_IDS, np.int32), frame=F,
                    answers=np.array([NO_ANSWER] * Q, np.int32).reshape(Q, 4))
    n_obs, n_table, owner, outside = raster(point_events(labels, xyz, F, G, cell_mm, h_obs_mm, tau_mm), G)
    state, own, cells = cell_states(n_obs, n_table, owner, min_pts)
    dist2 = edt((state == 2) | ((state == 0) & bool(unknown_blocks)))
    assert dist2.max() <= (G // 2) ** 2 and (dist2[state == 2] == 0).all()
    counts = cells.copy()
    counts[0] = outside
    return dict(state=state.astype(np.int32), owner=own.astype(np.int32), dist2=dist2.astype(np.int32), counts=counts.astype(np.int32),
                frame=F, answers=np.array([answer(state, dist2, q) for q in queries], np.int32).reshape(Q, 4))


FIELDS = ("state", "owner", "dist2", "counts", "frame", "answers")


# ---- scenes ---------------------------------------------------------------------------------------------------------------
PLANE_N, PLANE_D = S13.PLANE_N, S13.PLANE_D
Z_EDGE = 1.25            # the table ends where its depth reaches Z_EDGE (inside the image); past the edge the floor
FLOOR_DROP = 0.15        # ... a parallel plane this far below it, and a wall at Z_WALL where the floor runs out
Z_WALL = 3.5


def true_plane():
    """The table's plane as a caller would upload it: float32 normal, d, a point on it, u, v (S13.refine's rule)."""
    n = PLANE_N
    u = np.array([1.0, 0.0, 0.0]) - n[0] * n
    u /= np.linalg.norm(u)
    c = np.array([0.0, 0.0, -PLANE_D / n[2]])                  # where the optical axis meets the plane
    f32 = lambda a: np.asarray(a, np.float32)                   # noqa: E731
    return dict(found=1, normal=f32(n), d=np.float32(PLANE_D), centroid=f32(c), u=f32(u), v=f32(np.cross(n, u)))


def tabletop(H, W, seed, nobj=5, noise=0.0005, holes=0.05):
    """(labels [H,W] int32, xyz [3,H,W] float32): §13's camera over the tilted plane PLANE_N.p + PLANE_D = 0, ray-cast
    per pixel; the table's far edge lies inside the image and past it the rays reach the floor FLOOR_DROP below (or a
    wall); `nobj` labelled boxes lifted 4-15 cm off the table along its normal (each hides the table behind it: an
    occlusion shadow), one flat labelled patch (id nobj + 1) lying on the table, gaussian z noise, z in whole millimetres
    and `holes` of the pixels without depth."""
    rng = np.random.default_rng(seed)
    f = 0.9 * max(H, W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    rx, ry = (xs - (W - 1) / 2) / f, (ys - (H - 1) / 2) / f
    denom = PLANE_N[0] * rx + PLANE_N[1] * ry + PLANE_N[2]
    safe = np.where(denom < 0, denom, -1.0)
    zt = np.where(denom < 0, -PLANE_D / safe, np.inf)
    zf = np.where(denom < 0, -(PLANE_D + FLOOR_DROP) / safe, np.inf)
    on_table = (zt > 0.25) & (zt < Z_EDGE)
    z = np.where(on_table, zt, np.where(zf < Z_WALL, zf, Z_WALL))
    lab = np.zeros((H, W), np.int32)
    lift = np.zeros((H, W))
    for k in range(nobj):
        bh, bw = max(1, int(H * rng.uniform(0.08, 0.2))), max(1, int(W * rng.uniform(0.06, 0.16)))
        y0, x0 = int(rng.integers(H // 3, max(H // 3 + 1, H - bh))), int(rng.integers(0, max(1, W - bw)))
        lab[y0:y0 + bh, x0:x0 + bw] = k + 1
        lift[y0:y0 + bh, x0:x0 + bw] = rng.uniform(0.04, 0.15)
    ph, pw = max(1, H // 10), max(1, W // 8)
    y0, x0 = int(rng.integers(H // 2, max(H // 2 + 1, H - ph))), int(rng.integers(0, max(1, W - pw)))
    patch = np.zeros((H, W), bool)
    patch[y0:y0 + ph, x0:x0 + pw] = True
    lab[patch & (lab == 0) & on_table] = nobj + 1
    lift[~on_table] = 0.0
    lab[~on_table] = 0
    p = np.stack([rx * z, ry * z, z]) + lift * PLANE_N[:, None, None]
    zz = np.round((p[2] + noise * rng.standard_normal((H, W))) * 1000.0) / 1000.0
    scale = zz / p[2]
    xyz = np.stack([p[0] * scale, p[1] * scale, zz]).astype(np.float32)
    xyz[:, rng.random((H, W)) < holes] = 0.0
    return lab, xyz


# ---- engineered frames: the exact plane z = 1 m seen from above, coordinates given in whole millimetres -------------------
def flat_plane(found=1):
    f32 = lambda *a: np.array(a, np.float32)                    # noqa: E731
    return dict(found=found, normal=f32(0, 0, -1), d=np.float32(1.0), centroid=f32(0, 0, 1), u=f32(1, 0, 0), v=f32(0, -1, 0))


def frame_of(points, H, W, stride=1):
    """Pixels k*stride of an H x W frame carry points[k] = (x_mm, y_mm, z_mm, label) with coordinates q/1000 in fp32
    (or floats passed through: NaN, inf); every other pixel has no depth."""
    lab = np.zeros(H * W, np.int32)
    xyz = np.zeros((3, H * W), np.float32)
    assert len(points) * stride <= H * W
    for k, (x, y, z, l) in enumerate(points):
        lab[k * stride] = l
        xyz[:, k * stride] = np.array([x, y, z], np.float32) / np.float32(1000.0)
    return lab.reshape(H, W), xyz.reshape(3, H, W)


def at(i, j, G, cell_mm, h_mm=0, dx=0, dy=0):
    """A point (x_mm, y_mm, z_mm) of the flat plane that lands in cell (i, j), dx / dy millimetres into the cell from its
    low-i / low-j corner, h_mm above the plane."""
    return ((i - G // 2) * cell_mm + dx, -((j - G // 2) * cell_mm + dy), 1000 - h_mm)


def expect(case, got_events):
    """The reference's own check that an engineered frame lands where it is meant to: case['expect'] lists, per point,
    (i, j, cls) or 'out' (outside the grid) or None (takes no part)."""
    stride = case.get("stride", 1)
    for k, want in enumerate(case["expect"]):
        p = k * stride
        if want is None:
            assert not got_events["part"][p], (case["name"], k)
        elif want == "out":
            assert got_events["outside"][p], (case["name"], k)
        else:
            got = (int(got_events["i"][p]), int(got_events["j"][p]), int(got_events["cls"][p]))
            assert got_events["part"][p] and not got_events["outside"][p] and got == tuple(want), (case["name"], k, got, want)


def _case(name, points, expect_, H=6, W=11, stride=1, G=16, cell_mm=10, h_obs_mm=20, tau_mm=10, min_pts=1, queries=(), plane=None):
    lab, xyz = frame_of(points, H, W, stride)
    return dict(name=name, lab=lab, xyz=xyz, expect=expect_, stride=stride, G=G, cell_mm=cell_mm, h_obs_mm=h_obs_mm,
                tau_mm=tau_mm, min_pts=min_pts, queries=list(queries), plane=plane if plane is not None else flat_plane())


def case_boundaries():
    """Cell boundaries on both sides of the grid centre, along i and along j: exactly on the boundary and one millimetre
    to either side; floor division puts -1 mm into cell G/2 - 1 and -11 mm into G/2 - 2."""
    pts, exp = [], []
    for k, (x, i) in enumerate([(0, 8), (-1, 7), (1, 8), (10, 9), (9, 8), (11, 9), (-10, 7), (-11, 6), (-9, 7), (-20, 6), (-21, 5)]):
        pts.append((x, -(k - 5) * 10 - 5, 1000, 0))                # j = k - 5 + 8, mid-cell
        exp.append((i, k + 3, TABLE))
        pts.append((35, -x, 1000, 0))                              # the same along j (v = -y): i = 11
        exp.append((11, i, TABLE))
    return _case("boundaries", pts, exp, H=5, W=9, stride=2)


def case_heights():
    """T at h_obs, one above it, at tau, one above it, at -tau and one below it (h_obs 20 mm, tau 10 mm), unlabelled and
    labelled; with h_obs < tau (5 / 10) the band between them is an obstacle."""
    pts, exp = [], []
    for k, (h, cls) in enumerate([(20, IGNORED), (21, OBSTACLE), (10, TABLE), (11, IGNORED), (-10, TABLE), (-11, IGNORED), (0, TABLE)]):
        pts.append(at(2, k + 1, 16, 10, h, 5, 5) + (0,))
        exp.append((2, k + 1, cls))
        pts.append(at(5, k + 1, 16, 10, h, 5, 5) + (9,))           # a label makes an obstacle of everything not below -tau
        exp.append((5, k + 1, IGNORED if h < -10 else OBSTACLE))
    return _case("heights", pts, exp, H=4, W=7, stride=2)


def case_heights_low_obs():
    pts = [at(3, k + 1, 16, 10, h, 5, 5) + (0,) for k, h in enumerate([5, 6, 10, 11, -10, -11])]
    exp = [(3, k + 1, c) for k, c in enumerate([TABLE, OBSTACLE, OBSTACLE, OBSTACLE, TABLE, IGNORED])]
    return _case("heights_low_obs", pts, exp, h_obs_mm=5, tau_mm=10)


def case_min_pts():
    """min_pts 3: cells with 3 and 2 obstacle points, 3 and 2 table points, and 2 obstacle + 3 table points (table)."""
    pts, exp = [], []
    for j, (no, nt) in enumerate([(3, 0), (2, 0), (0, 3), (0, 2), (2, 3), (3, 3)]):
        for _ in range(no):
            pts.append(at(4, j + 2, 16, 10, 50, 5, 5) + (7 if j == 0 else 0,))
            exp.append((4, j + 2, OBSTACLE))
        for _ in range(nt):
            pts.append(at(4, j + 2, 16, 10, 0, 2, 7) + (0,))
            exp.append((4, j + 2, TABLE))
    return _case("min_pts", pts, exp, H=5, W=7, min_pts=3)


def case_grid_edge():
    """Points in the cells -1 and G (outside) next to the cells 0 and G - 1, along both axes."""
    G = 16
    pts = [at(-1, 3, G, 10, 0, 9, 5), at(0, 3, G, 10, 0, 0, 5), at(G - 1, 3, G, 10, 0, 9, 5), at(G, 3, G, 10, 0, 0, 5),
           at(3, -1, G, 10, 0, 5, 9), at(3, 0, G, 10, 0, 5, 0), at(3, G - 1, G, 10, 0, 5, 9), at(3, G, G, 10, 0, 5, 0),
           at(-1, -1, G, 10, 500, 5, 5), at(G, G, G, 10, -500, 5, 5)]   # outside counts whatever the height
    exp = ["out", (0, 3, TABLE), (G - 1, 3, TABLE), "out", "out", (3, 0, TABLE), (3, G - 1, TABLE), "out", "out", "out"]
    return _case("grid_edge", [p + (0,) for p in pts], exp)


def case_empty():
    return _case("empty", [], [], H=3, W=5, queries=[(0, 0, 0, WIDEST), (1, 2, 2, NEAREST)])


def case_all_table():
    """Every cell a table cell: dist2 is the distance to the grid's border; the widest query is a four-way tie."""
    G = 8
    pts = [at(i, j, G, 10, 0, 5, 5) + (0,) for i in range(G) for j in range(G)]
    return _case("all_table", pts, [(i, j, TABLE) for i in range(G) for j in range(G)], H=8, W=8, G=G,
                 queries=[(16, 0, 0, WIDEST), (17, 0, 0, WIDEST), (4, 7, 7, NEAREST)])


def tie_queries(state, dist2, need2s=(1, 2, 4, 5, 9)):
    """Two nearest queries found by search over anchors on the obstacle cells and around the grid: one whose nearest
    candidates (several, equally far from the anchor) differ in dist2, so that the larger clearance decides, and one
    where they agree in dist2 as well, so that the lowest index decides."""
    G = state.shape[0]
    ii, jj = np.nonzero(state == 1)
    anchors = [(int(i), int(j)) for i, j in zip(*np.nonzero(state == 2))][:400]
    anchors += [(i, j) for i in range(-2, G + 2) for j in (-2, -1, G, G + 1)] + [(i, j) for j in range(G) for i in (-2, -1, G, G + 1)]
    if G <= 16:
        anchors += [(i, j) for i in range(G) for j in range(G)]
    by_clearance = by_index = None
    for need2 in need2s:
        ok = dist2[ii, jj] >= need2
        if not ok.any():
            continue
        for ai, aj in anchors:
            da = (ii[ok] - ai) ** 2 + (jj[ok] - aj) ** 2
            d2 = np.sort(dist2[ii[ok], jj[ok]][da == da.min()])
            if len(d2) >= 2 and d2[-1] > d2[-2] and by_clearance is None:
                by_clearance = (need2, ai, aj, NEAREST)
            if len(d2) >= 2 and d2[-1] == d2[-2] and by_index is None:
                by_index = (need2, ai, aj, NEAREST)
            if by_clearance is not None and by_index is not None:
                return by_clearance, by_index
    raise AssertionError("no anchor with a tie of each kind")


def case_single_block():
    """A 16 x 16 table with one labelled cell off the centre.  Sixteen queries: widest and nearest with need2 at the
    largest dist2 and one above it, a nearest query decided by the larger clearance and one decided by the lowest index
    (tie_queries), anchors on the blocking cell, outside the grid and at the ends of their range, a need2 nothing meets."""
    G = 16
    pts = [at(i, j, G, 10, 30 if (i, j) == (5, 6) else 0, 5, 5) + (4 if (i, j) == (5, 6) else 0,) for i in range(G) for j in range(G)]
    exp = [(i, j, OBSTACLE if (i, j) == (5, 6) else TABLE) for i in range(G) for j in range(G)]
    c = _case("single_block", pts, exp, H=16, W=16, G=G)
    r = free_space(c["lab"], c["xyz"], c["plane"], G, 10, 20, 10, 1, 1)
    top = int(r["dist2"][r["state"] == 1].max())
    c["queries"] = [(top, 0, 0, WIDEST), (top + 1, 0, 0, WIDEST), (top, 0, 0, NEAREST), (top + 1, 0, 0, NEAREST), (0, 15, 15, WIDEST),
                    *tie_queries(r["state"].astype(np.int64), r["dist2"].astype(np.int64)), (1, 5, 6, NEAREST), (4, 5, 6, NEAREST),
                    (2, -3, 20, NEAREST), (1, -4096, 4095, NEAREST), (1, 4095, -4096, NEAREST), (1 << 30, 3, 3, NEAREST),
                    (0, 5, 6, NEAREST), (1 << 30, 0, 0, WIDEST), (top, 15, 0, NEAREST)]
    assert len(c["queries"]) == 16
    return c


def case_labels():
    """Labels 0 / 128 / -1 / 1000 are no ids (a table point stays a table point); 1 and 127 are."""
    pts = [at(6, j + 1, 16, 10, 0, 5, 5) + (l,) for j, l in enumerate([0, 128, -1, 1000, 1, 127])]
    exp = [(6, j + 1, c) for j, c in enumerate([TABLE, TABLE, TABLE, TABLE, OBSTACLE, OBSTACLE])]
    pts += [at(6, 9, 16, 10, 40, 5, 5) + (3,), at(6, 9, 16, 10, 40, 5, 5) + (90,), at(6, 9, 16, 10, 40, 5, 5) + (0,)]   # owner = max id
    exp += [(6, 9, OBSTACLE)] * 3
    return _case("labels", pts, exp)


def case_invalid():
    """NaN / inf / 0 / negative z, NaN x, a coordinate at 32.767 m (takes part, far outside) and one beyond it (does not)."""
    nan, inf = float("nan"), float("inf")
    pts = [(0, 0, nan, 0), (0, 0, inf, 0), (0, 0, 0, 5), (0, 0, -1000, 0), (nan, 0, 1000, 0), (0, -inf, 1000, 0),
           (32767, 0, 1000, 0), (32768, 0, 1000, 0), (0, -32767, 1000, 3), (0, 32768, 1000, 0), (5, -5, 32767, 0), (5, -5, 32768, 0),
           (5, -5, 1000, 0)]
    exp = [None] * 6 + ["out", None, "out", None, (8, 8, IGNORED), None, (8, 8, TABLE)]
    return _case("invalid", pts, exp, H=3, W=5)


ENGINEERED = {c.__name__[5:]: c for c in (case_boundaries, case_heights, case_heights_low_obs, case_min_pts, case_grid_edge,
                                          case_empty, case_all_table, case_single_block, case_labels, case_invalid)}


def run_case(c, **override):
    """The reference result of an engineered case (after asserting that its points land where they are meant to)."""
    kw = {k: override.get(k, c[k]) for k in ("G", "cell_mm", "h_obs_mm", "tau_mm", "min_pts")}
    if not override:
        expect(c, point_events(c["lab"], c["xyz"], frame_record(c["plane"]), c["G"], c["cell_mm"], c["h_obs_mm"], c["tau_mm"]))
    return free_space(c["lab"], c["xyz"], c["plane"], kw["G"], kw["cell_mm"], kw["h_obs_mm"], kw["tau_mm"], kw["min_pts"],
                      override.get("unknown_blocks", 1), override.get("queries", c["queries"]))
