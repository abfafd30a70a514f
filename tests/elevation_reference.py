"""Plain Python / numpy restatement of uoc_elevation (include/uoc_hip.h, steps F..I) for one frame: the semantics the GPU
tests check against.  Integers only (int64 arrays and Python ints).  Step P and the separable distance transform come from
tests/placement_reference.py; `level_brute` restates the level rule cell by cell and `edt_brute` the clearance over all
pairs, for small grids.  Also the engineered frames of the GPU tests, on the exact plane z = 1 m seen from above with
coordinates in whole millimetres; tests/test_elevation_host.py asserts that they contain what they are used for."""
import numpy as np

from tests import placement_reference as P

NUM_IDS = 128
S = P.S
NONE = -32768
KEY_BIAS = 1024
HQ_MAX = 32767
NO_ANSWER = (-1, -1, 0, 0)
NO_TOP = (0, 0, -1, -1, 0, 0, 0, 0)
FIELDS = ("elev", "owner", "pts", "near", "dist2", "tops", "info", "answers")
ANY = -1
BAND = (-32768, 32767)

frame_record, flat_plane, frame_of, at, tabletop, true_plane = P.frame_record, P.flat_plane, P.frame_of, P.at, P.tabletop, P.true_plane


# ---- F ------------------------------------------------------------------------------------------------------------------
def frame_ok(F):
    F = [int(x) for x in np.asarray(F, np.int64).reshape(16)]
    return F[13] == 1 and all(abs(F[k]) <= 32768 for k in (0, 1, 2, 4, 5, 6, 7, 8, 9)) and abs(F[3]) <= 1 << 34 \
        and all(abs(F[k]) <= 32767 for k in (10, 11, 12))


# ---- P, H, N ------------------------------------------------------------------------------------------------------------
def kept_points(labels, xyz, F, G, cell_mm, tau_mm):
    """(cell, key, id of the kept points, in raster order; outside; the pixel index of every kept point)."""
    ev = P.point_events(labels, xyz, np.asarray(F, np.int64), G, cell_mm, 0, tau_mm)
    inside = ev["part"] & ~ev["outside"]
    keep = inside & (ev["T"] >= -tau_mm * S)
    hq = np.minimum(ev["T"][keep] >> 14, HQ_MAX)                 # numpy's >> on int64 is arithmetic: a floor
    return (ev["i"][keep] * G + ev["j"][keep]).astype(np.int64), (hq + KEY_BIAS).astype(np.int64), ev["id"][keep].astype(np.int64), \
        int(ev["outside"].sum()), np.nonzero(keep)[0]


def cells_of(cell, key, ident, G, step_mm):
    """(pts, top, near) as flat int64 arrays of G*G."""
    pts, top, near = (np.zeros(G * G, np.int64) for _ in range(3))
    assert len(key) == 0 or (key.min() >= 24 and key.max() <= 33791)
    np.add.at(pts, cell, 1)
    np.maximum.at(top, cell, (key << 7) | ident)
    np.add.at(near, cell[key >= (top[cell] >> 7) - step_mm], 1)
    return pts, top, near


# ---- L ------------------------------------------------------------------------------------------------------------------
def blocking_of(solid, owner, elev, step_mm):
    """[G,G] bool from [G,G] solid / owner / elev, shifted arrays; the border is always blocking."""
    G = solid.shape[0]
    blk = ~solid.copy()
    blk[0, :] = blk[-1, :] = blk[:, 0] = blk[:, -1] = True
    c = (slice(1, -1), slice(1, -1))
    for nb in ((slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)), (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))):
        ok = solid[nb] & (owner[nb] == owner[c]) & (np.abs(elev[nb] - elev[c]) <= step_mm)
        blk[c] |= ~ok
    assert blk.shape == (G, G)
    return blk


def level_brute(solid, owner, elev, step_mm):
    """The level rule cell by cell, cells outside the grid not solid."""
    G = solid.shape[0]
    blk = np.zeros((G, G), bool)
    for i in range(G):
        for j in range(G):
            bad = not solid[i, j]
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                a, b = i + di, j + dj
                if not (0 <= a < G and 0 <= b < G and solid[a, b]):
                    bad = True
                elif owner[a, b] != owner[i, j] or abs(int(elev[a, b]) - int(elev[i, j])) > step_mm:
                    bad = True
            blk[i, j] = bad
    return blk


# ---- T, Q ---------------------------------------------------------------------------------------------------------------
def widest(mask, dist2):
    """(i, j, dist2) of the cell of `mask` with the largest dist2, ties to the lowest index, or None."""
    ii, jj = np.nonzero(mask)
    if len(ii) == 0:
        return None
    G = mask.shape[0]
    d2 = dist2[ii, jj].astype(np.int64)
    k = np.lexsort((ii * G + jj, -d2))[0]
    return int(ii[k]), int(jj[k]), int(d2[k])


def tops_of(solid, blocking, owner, elev, dist2):
    tops = np.array([NO_TOP] * NUM_IDS, np.int64)
    for a in range(NUM_IDS):
        mine = solid & (owner == a)
        cells = int(mine.sum())
        if cells == 0:
            continue
        lev = mine & ~blocking
        level = int(lev.sum())
        tops[a, 0], tops[a, 1], tops[a, 6] = cells, level, int(elev[mine].max())
        if level:
            i, j, d2 = widest(lev, dist2)
            total = int(elev[lev].astype(np.int64).sum())
            tops[a, 2:6] = (i, j, d2, int(elev[i, j]))
            tops[a, 7] = total // level                          # Python's // floors towards minus infinity
    return tops


def answer(blocking, owner, elev, dist2, query):
    need2, ident, hmin, hmax = (int(x) for x in query)
    cand = ~blocking & (elev >= hmin) & (elev <= hmax) & ((owner >= 1) if ident == ANY else (owner == ident))
    w = widest(cand, dist2)
    return NO_ANSWER if w is None else (w[0], w[1], w[2], int(w[2] >= need2))


def heights(labels, xyz, F, G, cell_mm, tau_mm, step_mm, min_pts, queries=(), brute=False):
    """One frame.  F: the int64 [16] frame record.  Returns dict elev, owner, pts, near, dist2 [G,G] int32, tops [128,8]
    int32, info [4] int32, answers [Q,4] int32 (and solid, blocking [G,G] bool).  brute: the all-pairs level and
    clearance steps."""
    Q = len(queries)
    if not frame_ok(F):
        z = np.zeros((G, G), np.int32)
        return dict(elev=np.full((G, G), NONE, np.int32), owner=z, pts=z.copy(), near=z.copy(), dist2=z.copy(),
                    tops=np.array([NO_TOP] * NUM_IDS, np.int32), info=np.zeros(4, np.int32),
                    answers=np.array([NO_ANSWER] * Q, np.int32).reshape(Q, 4), solid=z.astype(bool), blocking=~z.astype(bool))
    cell, key, ident, outside, _ = kept_points(labels, xyz, F, G, cell_mm, tau_mm)
    pts, top, near = (a.reshape(G, G) for a in cells_of(cell, key, ident, G, step_mm))
    elev = np.where(pts > 0, (top >> 7) - KEY_BIAS, NONE)
    owner = np.where(pts > 0, top & 127, 0)
    solid = near >= min_pts
    assert (near <= pts).all() and ((pts > 0) == (near > 0)).all()
    blocking = level_brute(solid, owner, elev, step_mm) if brute else blocking_of(solid, owner, elev, step_mm)
    dist2 = P.edt_brute(blocking) if brute else P.edt(blocking)
    assert dist2.max() <= (G // 2) ** 2 and ((dist2 == 0) == blocking).all()
    info = np.array([1, outside, int((pts > 0).sum()), int(solid.sum())], np.int32)
    return dict(elev=elev.astype(np.int32), owner=owner.astype(np.int32), pts=pts.astype(np.int32), near=near.astype(np.int32),
                dist2=dist2.astype(np.int32), tops=tops_of(solid, blocking, owner, elev, dist2).astype(np.int32), info=info,
                answers=np.array([answer(blocking, owner, elev, dist2, q) for q in queries], np.int32).reshape(Q, 4),
                solid=solid, blocking=blocking)


def atomic_events(labels, xyz, F, G, cell_mm, tau_mm, step_mm, group):
    """(before, after): the atomic operations of the two point passes if every kept point issued its own (an add and a
    maximum in the first pass, an add per near point in the second), and after every wave has merged the equal cells of
    its `group` consecutive pixels (256 with vector loads, 64 without)."""
    cell, key, ident, _, pix = kept_points(labels, xyz, F, G, cell_mm, tau_mm)
    _, top, _ = cells_of(cell, key, ident, G, step_mm)
    is_near = key >= (top[cell] >> 7) - step_mm
    before = 2 * len(cell) + int(is_near.sum())
    wave = pix // group
    first = len(np.unique(np.stack([wave, cell]), axis=1).T)
    second = len(np.unique(np.stack([wave[is_near], cell[is_near]]), axis=1).T)
    return before, 2 * first + second


# ---- engineered frames ---------------------------------------------------------------------------------------------------
def _case(name, points, H, W, G=16, cell_mm=10, tau_mm=10, step_mm=5, min_pts=1, queries=(), F=None, stride=1):
    lab, xyz = frame_of(points, H, W, stride)
    return dict(name=name, lab=lab, xyz=xyz, G=G, cell_mm=cell_mm, tau_mm=tau_mm, step_mm=step_mm, min_pts=min_pts,
                queries=list(queries), F=frame_record(flat_plane()) if F is None else np.asarray(F, np.int64))


def run_case(c, **over):
    kw = {k: over.get(k, c[k]) for k in ("G", "cell_mm", "tau_mm", "step_mm", "min_pts", "queries")}
    return heights(c["lab"], c["xyz"], over.get("F", c["F"]), kw["G"], kw["cell_mm"], kw["tau_mm"], kw["step_mm"], kw["min_pts"],
                   kw["queries"], brute=over.get("brute", False))


def plate(G, cell_mm, h_of, id_of, i0=0, i1=None, j0=0, j1=None, per_cell=1):
    """`per_cell` points in every cell of rows i0..i1-1, columns j0..j1-1: height h_of(i, j) mm, label id_of(i, j)."""
    i1, j1 = G if i1 is None else i1, G if j1 is None else j1
    return [at(i, j, G, cell_mm, h_of(i, j), 2 + 3 * k, 5) + (id_of(i, j),) for i in range(i0, i1) for j in range(j0, j1)
            for k in range(per_cell)]


def case_height_bounds():
    """tau 10: T = -tau*S kept (hq = -10), one below (h = -11) ignored; T = -1 is not reachable with whole millimetres on
    the flat frame, so h = -1 stands for the negative floor here and test_elevation_host.py checks T = -1 on a frame record
    with D lowered by one; the clamp: h = 32766 is past z > 0, so the clamp is checked through a record with a large D."""
    pts = [at(3, 3, 16, 10, -10, 5, 5) + (0,), at(3, 4, 16, 10, -11, 5, 5) + (0,), at(3, 5, 16, 10, -1, 5, 5) + (0,),
           at(3, 6, 16, 10, 0, 5, 5) + (2,), at(3, 7, 16, 10, 900, 5, 5) + (3,)]
    return _case("height_bounds", pts, 3, 5)


def case_height_shifted():
    """The flat frame with D lowered by one unit (T = h*S - 1: h = 0 gives T = -1, hq = -1; h = -10 falls below -tau*S) and
    a second record with D raised to the clamp: hq = 32767 for every point (D = 2^34 is the largest accepted)."""
    c = case_height_bounds()
    F = c["F"].copy()
    F[3] -= 1
    c["F"], c["name"] = F, "height_shifted"
    return c


def case_height_clamp():
    c = case_height_bounds()
    F = c["F"].copy()
    F[3] = 1 << 34
    c["F"], c["name"] = F, "height_clamp"
    return c


def case_two_ids():
    """Two ids at one height in one cell: the larger id owns it; a higher point of a smaller id wins over both."""
    pts = [at(4, 4, 16, 10, 30, 3, 3) + (5,), at(4, 4, 16, 10, 30, 6, 6) + (9,), at(4, 4, 16, 10, 30, 8, 2) + (0,),
           at(4, 6, 16, 10, 30, 3, 3) + (9,), at(4, 6, 16, 10, 31, 6, 6) + (5,)]
    return _case("two_ids", pts, 1, 5)


def case_step():
    """A 6 x 6 plate of id 1 at 50 mm inside a G = 16 grid with a staircase along j: columns 5..10 at 50, 55, 60, 66, 66,
    66: a step of exactly step_mm (5) is level, step_mm + 1 (60 -> 66) blocks both sides.  Cell (7, 5) carries extra
    points at top - 5 (near) and top - 6 (not near)."""
    hs = {5: 50, 6: 55, 7: 60, 8: 66, 9: 66, 10: 66}
    pts = plate(16, 10, lambda i, j: hs[j], lambda i, j: 1, 4, 11, 5, 11)
    pts += [at(7, 5, 16, 10, 45, 8, 8) + (1,), at(7, 5, 16, 10, 44, 8, 2) + (1,)]
    return _case("step", pts, 6, 8)


def case_lone_point():
    """A table of two points per cell and one lone point 40 mm above cell (8, 8): with min_pts 2 the cell is not solid and
    its four neighbours are blocking; with min_pts 1 it is a one-cell plateau that blocks by the step rule."""
    pts = plate(16, 10, lambda i, j: 0, lambda i, j: 0, per_cell=2) + [at(8, 8, 16, 10, 40, 5, 8) + (0,)]
    return _case("lone_point", pts, 19, 27, min_pts=2)


def case_two_owners():
    """Ids 1 and 2 side by side at equal elev (columns 4..7 and 8..11, rows 4..11): both sides of the seam are blocking."""
    pts = plate(16, 10, lambda i, j: 30, lambda i, j: 1 if j < 8 else 2, 4, 12, 4, 12)
    return _case("two_owners", pts, 8, 8)


def case_grid_edge():
    """Every cell of a G = 8 grid solid at one height, and points in the cells -1 and G: the border is blocking, outside
    is counted."""
    G = 8
    pts = plate(G, 10, lambda i, j: 20, lambda i, j: 4)
    pts += [at(-1, 3, G, 10, 20, 9, 5) + (4,), at(G, 3, G, 10, 20, 0, 5) + (4,), at(3, -1, G, 10, 0, 5, 9) + (0,),
            at(3, G, G, 10, 500, 5, 0) + (0,), at(-1, -1, G, 10, -500, 5, 5) + (0,)]
    return _case("grid_edge", pts, 9, 8, G=G, queries=[(1, 4, BAND[0], BAND[1]), (9, ANY, 20, 20)])


def case_empty():
    return _case("empty", [], 3, 5, queries=[(0, ANY, BAND[0], BAND[1]), (1, 0, 0, 0)])


def case_not_found():
    c = case_two_owners()
    F = c["F"].copy()
    F[13] = 0
    c.update(F=F, name="not_found", queries=[(0, ANY, BAND[0], BAND[1]), (0, 1, BAND[0], BAND[1])])
    return c


def bad_word_cases():
    """The frame record with one word out of range, for word 0, word 3 and word 10 (and found = 2): no plane."""
    out = []
    for word, value in ((0, 32769), (3, (1 << 34) + 1), (10, -32768), (13, 2)):
        c = case_two_owners()
        F = c["F"].copy()
        F[word] = value
        c.update(F=F, name=f"bad_word_{word}", queries=[(0, ANY, BAND[0], BAND[1])])
        out.append(c)
    return out


def case_all_ids():
    """Ids 1..127 as one tower each: 3 x 3 cells at 20 + a mm on a G = 64 grid of table points; every row of tops is
    filled (one level cell per tower: its centre)."""
    G = 64
    owner = np.zeros((G, G), np.int64)
    for a in range(1, 128):
        r, c = divmod(a - 1, 12)
        owner[2 + 5 * r:5 + 5 * r, 2 + 5 * c:5 + 5 * c] = a
    pts = plate(G, 10, lambda i, j: 20 + owner[i, j] if owner[i, j] else 0, lambda i, j: int(owner[i, j]))
    return _case("all_ids", pts, 64, 64, G=G, queries=[(1, 127, 0, 200), (2, 64, 84, 84), (1, ANY, 0, 147), (1, 0, 0, 0)])


def case_two_plateaus():
    """Two equal 5 x 5 plateaus of id 3 at 40 mm: the lowest index wins in tops and in a query.  Sixteen queries: id -1 never
    answers with a table cell although the table is wider; the band inclusive at both ends; a band and an id without a
    candidate; need2 at dist2 and one above."""
    G = 32
    own = lambda i, j: 3 if (4 <= i < 9 and (4 <= j < 9 or 20 <= j < 25)) else (7 if (20 <= i < 23 and 4 <= j < 7) else 0)   # noqa: E731
    hof = lambda i, j: {3: 40, 7: 90, 0: 0}[own(i, j)]          # noqa: E731
    c = _case("two_plateaus", plate(G, 10, hof, own), 32, 32, G=G)
    r = run_case(c)
    d3, d0 = int(r["tops"][3, 4]), int(r["tops"][0, 4])
    c["queries"] = [(d3, 3, BAND[0], BAND[1]), (d3 + 1, 3, BAND[0], BAND[1]), (d3, ANY, BAND[0], BAND[1]), (0, 0, BAND[0], BAND[1]),
                    (d0, 0, 0, 0), (d0 + 1, 0, 0, 0), (1, ANY, 40, 40), (1, ANY, 41, 89), (1, ANY, 41, 90), (1, ANY, 90, BAND[1]),
                    (1, ANY, BAND[0], 39), (1, 5, BAND[0], BAND[1]), (1, 127, 0, 100), (1, 3, 39, 40), (1, 3, 40, 41), (1 << 30, 7, 90, 90)]
    assert len(c["queries"]) == 16
    return c


ENGINEERED = {c.__name__[5:]: c for c in (case_height_bounds, case_height_shifted, case_height_clamp, case_two_ids, case_step,
                                          case_lone_point, case_two_owners, case_grid_edge, case_empty, case_not_found, case_all_ids,
                                          case_two_plateaus)}
ENGINEERED.update({c["name"]: (lambda c=c: c) for c in bad_word_cases()})
