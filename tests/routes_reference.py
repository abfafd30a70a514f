"""The definition of uoc_routes (include/uoc_hip.h) restated with numpy, Python integers and heapq, and the
grids the tests run it on.  Nothing here comes from the package's routes, footprint or placement modules: every constant
is written out, so a wrong constant in the package fails a test.

`routes` is the restatement the GPU tests compare with: PASSABLE by the all-offsets form of the definition, a heap
Dijkstra over the moves, the closest-approach key and the walk back.  `passable_spans` is the span-and-run form the
kernels use; tests/test_routes_host.py holds it against the all-offsets form."""
import heapq

import numpy as np

S = 16384
MAX_QUERIES = 8
MAX_NEED2 = 4096
MAX_PATH = 4096
MOVES = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))
COST = (5, 5, 5, 5, 7, 7, 7, 7)
IDX_MASK = 0x3FFFF
COST_MASK = (1 << 21) - 1
DA_MASK = (1 << 19) - 1
NO_ROUTE = (0, 0, -1, -1, 0, 0, 0, 0)


def record(need2, src, dst=None, ignore=0):
    ti, tj = (-1, -1) if dst is None else dst
    return (int(need2), int(src[0]), int(src[1]), int(ti), int(tj), int(ignore), 0, 0)


def check_params(G, queries, unknown_blocks, max_path):
    assert G % 8 == 0 and 8 <= G <= 512 and 1 <= len(queries) <= MAX_QUERIES and unknown_blocks in (0, 1) and 1 <= max_path <= MAX_PATH
    for q in queries:
        need2, si, sj, ti, tj, ignore, z6, z7 = (int(x) for x in q)
        assert 0 <= need2 <= MAX_NEED2 and 0 <= si < G and 0 <= sj < G and 0 <= ignore <= 127 and z6 == 0 and z7 == 0
        assert (ti, tj) == (-1, -1) or (0 <= ti < G and 0 <= tj < G)


def free_cells(state, owner, ignore, unknown_blocks):
    """[G,G] bool: the cells that are FREE for a query with this `ignore`."""
    st, ow = np.asarray(state).astype(np.int64), np.asarray(owner).astype(np.int64)
    obstacle = (st == 2) & (ow >= 1) & (ow <= 127)
    unknown = ~obstacle & (st != 1)
    free = (st == 1) | (unknown & (not unknown_blocks))
    if ignore >= 1:
        free |= obstacle & (ow == ignore)
    return free


def disc_offsets(need2):
    r = 0
    while r * r < need2:
        r += 1
    return [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1) if di * di + dj * dj < need2]


def passable(free, need2):
    """The all-offsets form: FREE, and every offset of the disc lands inside the grid on a FREE cell."""
    G = free.shape[0]
    offs = disc_offsets(need2)
    R = max([abs(d) for o in offs for d in o], default=0)
    padded = np.zeros((G + 2 * R, G + 2 * R), bool)             # a cell outside the grid is never FREE
    padded[R:R + G, R:R + G] = free
    ok = free.copy()
    for di, dj in offs:
        ok &= padded[R + di:R + di + G, R + dj:R + dj + G]
    return ok


def runs_of(free):
    """[G,G] int64: the length of the run of FREE cells that ends at each cell, along j."""
    G = free.shape[1]
    j = np.arange(G, dtype=np.int64)[None, :]
    last_blocked = np.maximum.accumulate(np.where(free, -1, j), axis=1)
    return np.where(free, j - last_blocked, 0)


def disc_spans(need2):
    """{di: h}: row di of the disc is the span |dj| <= h."""
    rows = {}
    for di, dj in disc_offsets(need2):
        rows[di] = max(rows.get(di, 0), abs(dj))
    return rows


def passable_spans(free, need2):
    """The span-and-run form: row di of the disc around (i, j) is free iff it lies in the grid and the run that ends at
    (i+di, j+h) is at least 2h+1 long."""
    G = free.shape[0]
    run = runs_of(free)
    ok = free.copy()
    I, J = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    for di, h in disc_spans(need2).items():
        inside = (I + di >= 0) & (I + di < G) & (J - h >= 0) & (J + h < G)
        got = run[np.clip(I + di, 0, G - 1), np.clip(J + h, 0, G - 1)]
        ok &= inside & (got >= 2 * h + 1)
    return ok


def move_tables(pas):
    """Per move k a flat list: may the move (di, dj) be made from the cell.  Both ends PASSABLE; a diagonal move also needs
    (i+di, j) and (i, j+dj) PASSABLE."""
    G = pas.shape[0]
    P = np.zeros((G + 2, G + 2), bool)
    P[1:-1, 1:-1] = pas
    at = lambda di, dj: P[1 + di:1 + di + G, 1 + dj:1 + dj + G]        # noqa: E731
    out = []
    for di, dj in MOVES:
        ok = pas & at(di, dj)
        if di and dj:
            ok = ok & at(di, 0) & at(0, dj)
        out.append(ok.reshape(-1).tolist())
    return out


def dijkstra(pas, src):
    """[G,G] int32: the least total move cost from src, -1 where not PASSABLE or not reachable.  A heap Dijkstra."""
    G = pas.shape[0]
    s = src[0] * G + src[1]
    if not pas[src[0], src[1]]:
        return np.full((G, G), -1, np.int32)
    ok = move_tables(pas)
    step = [di * G + dj for di, dj in MOVES]
    big = 1 << 40
    dist = [big] * (G * G)
    dist[s] = 0
    heap = [(0, s)]
    while heap:
        d, c = heapq.heappop(heap)
        if d > dist[c]:
            continue
        for k in range(8):
            if ok[k][c]:
                n, nd = c + step[k], d + COST[k]
                if nd < dist[n]:
                    dist[n] = nd
                    heapq.heappush(heap, (nd, n))
    out = np.array([-1 if d == big else d for d in dist], np.int64).reshape(G, G)
    assert out.max() <= 7 * G * G
    return out.astype(np.int32)


def key_of(da, cost, idx):
    return ((DA_MASK - da) << 39) | ((COST_MASK - cost) << 18) | (IDX_MASK - idx)


def closest(cost, target):
    """The reached cell with the largest key: (i, j), or None when nothing is reached."""
    G = cost.shape[0]
    best, cell = -1, None
    for i, j in np.argwhere(cost >= 0).tolist():
        k = key_of((i - target[0]) ** 2 + (j - target[1]) ** 2, int(cost[i, j]), i * G + j)
        if k > best:
            best, cell = k, (i, j)
    return cell


def move_allowed(pas, c, k):
    """May the move MOVES[k] be made from cell c (the graph is symmetric: n -> c is allowed iff c -> n is)."""
    G = pas.shape[0]
    inside = lambda i, j: 0 <= i < G and 0 <= j < G and bool(pas[i, j])      # noqa: E731
    (i, j), (di, dj) = c, MOVES[k]
    if not (inside(i, j) and inside(i + di, j + dj)):
        return False
    return not (di and dj) or (inside(i + di, j) and inside(i, j + dj))


def backtrack(cost, pas, c, src):
    """The cells from c back to src: at each cell the first neighbour n in MOVES' order with the move allowed and
    cost[n] + w == cost[c]."""
    cells = [tuple(c)]
    while tuple(c) != tuple(src):
        for k, (di, dj) in enumerate(MOVES):
            n = (c[0] + di, c[1] + dj)
            if move_allowed(pas, c, k) and cost[n] >= 0 and int(cost[n]) + COST[k] == int(cost[c]):
                break
        else:
            raise AssertionError(f"no predecessor at {c}")
        c = n
        cells.append(c)
    return cells


def _found(frame):
    return frame is None or int(np.asarray(frame).reshape(-1)[13]) == 1


def routes(state, owner, queries, unknown_blocks, max_path=1024, frame=None, passable_fn=passable):
    """One frame: state, owner [G,G] integer arrays, queries [Q][8], frame None or the 16 int64 words.  Returns
    {"cost": [Q,G,G] int32, "info": [Q,8] int32, "path": [Q,max_path,2] int32}."""
    G, Q = np.asarray(state).shape[0], len(queries)
    check_params(G, queries, unknown_blocks, max_path)
    cost = np.full((Q, G, G), -1, np.int32)
    info = np.zeros((Q, 8), np.int32)
    path = np.full((Q, max_path, 2), -1, np.int32)
    maps, fields = {}, {}
    for q, rec in enumerate(queries):
        need2, si, sj, ti, tj, ignore = (int(x) for x in rec[:6])
        if not _found(frame):
            info[q] = NO_ROUTE
            continue
        if (ignore, need2) not in maps:                         # queries that share (ignore, need2) share a map
            maps[ignore, need2] = passable_fn(free_cells(state, owner, ignore, unknown_blocks), need2)
        pas = maps[ignore, need2]
        if (ignore, need2, si, sj) not in fields:
            fields[ignore, need2, si, sj] = dijkstra(pas, (si, sj))
        c = cost[q] = fields[ignore, need2, si, sj]
        src_ok = bool(pas[si, sj])
        info[q] = (int(src_ok), 0, -1, -1, 0, 0, int((c >= 0).sum()), int(pas.sum()))
        if not src_ok or ti < 0:
            continue
        ci, cj = closest(c, (ti, tj))
        cells = backtrack(c, pas, (ci, cj), (si, sj))
        steps = len(cells) - 1
        info[q, 1:6] = (int((ci, cj) == (ti, tj)), ci, cj, int(c[ci, cj]), steps)
        n = min(steps, max_path - 1) + 1
        path[q, :n] = np.array(cells[:n], np.int32).reshape(n, 2)
    return {"cost": cost, "info": info, "path": path}


# ---- grids ------------------------------------------------------------------------------------------------------------
def table(G, fill=1):
    return np.full((G, G), fill, np.int32), np.zeros((G, G), np.int32)


def flat_frame(found=1):
    """A frame record of the plane z = 1 m seen from above: N, D, U, V, qc and `found`."""
    F = np.zeros(16, np.int64)
    F[0:3], F[3] = (0, 0, -S), 1000 * S
    F[4:7], F[7:10], F[10:13], F[13] = (S, 0, 0), (0, -S, 0), (0, 0, 1000), found
    return F


def random_grid(G, seed, noise=0.03):
    """A seeded grid in the manner of tests/footprint_reference.py: table with patches of unknown, 3-6 convex blobs with
    ids from 1..127 and `noise` of the cells redrawn at random: states -1..3 and owners -5..129 (out-of-contract values
    included).  Returns state, owner."""
    rng = np.random.default_rng(7000 + seed)
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
    return st, ow


def present_id(owner, state):
    ids = np.unique(owner[(state == 2) & (owner >= 1) & (owner <= 127)])
    return int(ids[0]) if len(ids) else 1


def random_queries(G, seed, st, ow, Q=8):
    """Q seeded queries on a grid: sources and targets drawn among the table cells (so that most sources are passable) and
    among all cells; need2 from a small set, so that some queries share (ignore, need2) and some differ; ignore 0, a
    present id and an absent one; one query without a target and one whose target is its source."""
    rng = np.random.default_rng(9000 + seed)
    tab = np.argwhere(np.asarray(st) == 1)
    pick = lambda: tuple(int(x) for x in (tab[rng.integers(len(tab))] if len(tab) and rng.random() < 0.8 else rng.integers(0, G, 2)))  # noqa: E731
    P = present_id(ow, st)
    need2s = [0, 1, 2, 4, 0, 9, 1, 4]
    ignores = [0, 0, P, 0, 0, 0, 126, P]
    out = []
    for q in range(Q):
        src = pick()
        dst = None if q == 3 else src if q == 6 else pick()
        out.append(record(need2s[q], src, dst, ignores[q]))
    return out


def serpentine(G):
    """Corridors of table one cell wide along j on the even rows; the odd rows are obstacle (id 3) but for one cell at
    alternating ends.  From (0, 0) the way to the end of the last corridor takes G/2 corridors of G-1 moves and two moves
    per turn, every one orthogonal: 5 ((G/2) (G-1) + 2 (G/2 - 1))."""
    st, ow = table(G)
    for i in range(1, G, 2):
        st[i, :], ow[i, :] = 2, 3
        j = G - 1 if (i // 2) % 2 == 0 else 0
        st[i, j], ow[i, j] = 1, 0
    return st, ow


def serpentine_end(G):
    """The far end of the last corridor and the cost of getting there from (0, 0)."""
    last = G - 2
    end = (last, G - 1 if (last // 2) % 2 == 0 else 0)
    return end, 5 * ((G // 2) * (G - 1) + 2 * (G // 2 - 1))


def wall(G, col, gap_rows=(), owner=3):
    """A table with a wall of obstacle along column `col` but for the rows in gap_rows."""
    st, ow = table(G)
    st[:, col], ow[:, col] = 2, owner
    for i in gap_rows:
        st[i, col], ow[i, col] = 1, 0
    return st, ow


def chink(G=16):
    """Column G/2 blocked on the rows above the middle, column G/2 + 1 on the rows from the middle down: the two halves
    meet only across the corner between (G/2, G/2) and (G/2 - 1, G/2 + 1), which no move may cut."""
    st, ow = table(G)
    h = G // 2
    st[:h, h], ow[:h, h] = 2, 3
    st[h:, h + 1], ow[h:, h + 1] = 2, 4
    return st, ow


def only_obstacle(G=16):
    """One 3 x 9 box of id 7 across the middle of a table."""
    st, ow = table(G)
    st[6:9, 3:12], ow[6:9, 3:12] = 2, 7
    return st, ow


def out_of_contract(G=16):
    """Table with state-2 cells of owner 0, 128 and -5 and cells of state 3 and -1: all unknown; a cell of owner 7 whose
    state is 1 is table; one real obstacle cell of id 7."""
    st, ow = table(G)
    st[4, 4], ow[4, 4] = 2, 0
    st[4, 10], ow[4, 10] = 2, 128
    st[10, 4], ow[10, 4] = 2, -5
    st[10, 10] = 3
    st[12, 12], ow[12, 12] = -1, 7
    st[12, 6], ow[12, 6] = 1, 7
    st[7, 7], ow[7, 7] = 2, 7
    return st, ow


def hand8():
    """The hand-counted case: an 8 x 8 table with a wall (id 3) on column 4, rows 0..5.  need2 = 0, from (2, 2).
    (2, 3): one move, 5.  (6, 3): four rows down and one column across, one of the moves diagonal: 7 + 3*5 = 22.  (6, 4),
    the first free cell of column 4: 27, because the diagonal from (5, 3) would cut the wall's corner (5, 4).  (7, 5): the
    diagonal from (6, 4) is allowed, (7, 4) and (6, 5) being table: 34.  (7, 7): 44.  (2, 5), across the wall from the
    source: (6, 5) = 32, then four moves straight up: 52.  58 cells reached, the wall's 6 are -1.  The walk back from
    (7, 7) takes (0, -1) before any diagonal: (7,6), (7,5), (7,4), then (-1,-1) to (6,3), (5,3), (4,3), (3,3) and (-1,-1)
    to (2,2): 8 moves."""
    return wall(8, 4, gap_rows=(6, 7))


def walled_target(G=16):
    """A full wall on column 10: a target behind it is not reachable."""
    return wall(G, 10)


def gap_grid(width, G=16):
    """A wall on column 8 with a gap of `width` rows starting at row 6."""
    return wall(G, 8, gap_rows=range(6, 6 + width))


def big_grid(G=512):
    """G = 512 for need2 = 4096 (a disc 127 cells across): a table with a bar of id 5 that leaves a passage 140 cells wide
    on one side, a block of unknown in a corner and a single obstacle cell of id 9 near the other."""
    st, ow = table(G)
    st[250:262, 0:372], ow[250:262, 0:372] = 2, 5
    st[0:40, 0:40] = 0
    st[440, 60], ow[440, 60] = 2, 9
    return st, ow


def engineered():
    """name -> (state, owner, queries): the engineered cases of tests/test_routes_gpu.py, each run under both
    unknown_blocks."""
    out = {}
    for G in (8, 16):
        h = G // 2
        st, ow = table(G)
        out[f"empty_{G}"] = (st, ow, [record(n, (h, h), (0, 0)) for n in (0, 1, 2, 25)] + [record(n, (h, h)) for n in (0, 1, 2, 25)])
        out[f"all_obstacle_{G}"] = (np.full((G, G), 2, np.int32), np.full((G, G), 4, np.int32),
                                    [record(0, (h, h), (0, 0)), record(1, (1, 1)), record(0, (h, h), (1, 1), ignore=4), record(0, (h, h), (1, 1), ignore=5)])
        st, ow = table(G, 0)
        out[f"all_unknown_{G}"] = (st, ow, [record(0, (h, h), (0, 0)), record(4, (h, h), (1, 1)), record(1, (0, 0))])
    for width in (3, 2):                                        # need2 = 4: the disc is 3 cells across
        st, ow = gap_grid(width)
        out[f"gap_{width}"] = (st, ow, [record(4, (7, 3), (7, 12)), record(4, (7, 12), (7, 3)), record(1, (7, 3), (7, 12)), record(2, (7, 3), (7, 12))])
    st, ow = chink()
    out["chink"] = (st, ow, [record(0, (8, 2), (7, 13)), record(1, (8, 8), (7, 9)), record(0, (7, 9), (8, 8)), record(0, (8, 8))])
    st, ow = only_obstacle()
    out["source_not_passable"] = (st, ow, [record(0, (7, 5), (1, 1)), record(4, (1, 1), (12, 12)), record(0, (7, 5)), record(9, (7, 1), (12, 12))])
    st, ow = walled_target()
    out["walled_target"] = (st, ow, [record(0, (8, 2), (8, 13)), record(1, (8, 2), (0, 15)), record(0, (8, 2), (8, 10)), record(0, (8, 13), (8, 2))])
    st, ow = table(16)
    out["target_is_source"] = (st, ow, [record(0, (5, 5), (5, 5)), record(4, (5, 5), (5, 5)), record(4, (0, 0), (0, 0))])
    out["no_target"] = (st, ow, [record(0, (5, 5)), record(9, (8, 8)), record(9, (1, 1))])
    st, ow = only_obstacle()
    out["ignore"] = (st, ow, [record(1, (7, 5), (12, 5), ignore=7), record(1, (2, 5), (12, 5), ignore=7), record(1, (2, 5), (12, 5), ignore=9),
                              record(1, (2, 5), (12, 5), ignore=0), record(1, (7, 5), (12, 5), ignore=9), record(1, (2, 5), (7, 5), ignore=127)])
    st, ow = out_of_contract()
    out["out_of_contract"] = (st, ow, [record(0, (1, 1), (14, 14)), record(1, (1, 1), (12, 12)), record(0, (4, 4), (10, 10)), record(0, (1, 1), (7, 7), ignore=7),
                                       record(1, (12, 6), (4, 10))])
    return out
