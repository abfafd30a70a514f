"""uoc_motion (include/uoc_hip.h) restated in numpy integers, and the grids the motion tests share.

The search is written as it is defined: every rotation, every shift, every cell of both masks, no shortcut.  `motion`
loops over the rotations and counts all shifts of one rotation at once; `cost_one` is the same count for one candidate
in plain Python integers and sets, and tests/test_motion_host.py holds the two to each other.  Where this file and the
header could drift, the header wins."""
import numpy as np

S = 16384
MAX_ROT, MAX_RADIUS, MAX_PAIRS, MAX_CELLS = 64, 16, 16, 4096
NO_ROW = (-1, 0, 0, 0)
BEST_FIELDS = ("status", "k", "si", "sj", "cost", "n_a", "n_b", "still", "pi", "pj", "qi", "qj", "ti", "tj", "second", "zero")


# ---- the definition ---------------------------------------------------------------------------------------------------
def rotation_table(A):
    """Step T: [A,2] int64, (rint(cos(2 pi k / A) S), rint(sin(2 pi k / A) S))."""
    t = 2.0 * np.pi * np.arange(A, dtype=np.float64) / A
    return np.stack([np.rint(np.cos(t) * S), np.rint(np.sin(t) * S)], axis=1).astype(np.int64)


def rd(x):
    return (2 * x + S) // (2 * S)          # floor division, for numpy int64 and for Python integers alike


def forward(d, cx, cy):
    return np.stack([rd(d[..., 0] * cx - d[..., 1] * cy), rd(d[..., 0] * cy + d[..., 1] * cx)], axis=-1)


def inverse(e, cx, cy):
    return np.stack([rd(e[..., 0] * cx + e[..., 1] * cy), rd(-e[..., 0] * cy + e[..., 1] * cx)], axis=-1)


def cells_of(state, owner, a):
    """Step C: the cells [n,2] int64 of id a, in row-major order."""
    return np.argwhere((np.asarray(state) == 2) & (np.asarray(owner) == a)).astype(np.int64)


def pivot(c):
    """Step P."""
    n = len(c)
    return np.array([(2 * int(c[:, 0].sum()) + n) // (2 * n), (2 * int(c[:, 1].sum()) + n) // (2 * n)], np.int64)


def key(cost, si, sj, k, A, R):
    """Step K, a Python integer."""
    return (int(cost) << 33) | ((si * si + sj * sj) << 23) | (min(k, A - k) << 17) | (k << 11) | ((si + R) * (2 * R + 1) + (sj + R))


def unkey(v, R):
    """(cost, s2, kk, k, si, sj) of a key."""
    sidx = v & 2047
    return v >> 33, (v >> 23) & 1023, (v >> 17) & 63, (v >> 11) & 63, sidx // (2 * R + 1) - R, sidx % (2 * R + 1) - R


def shifts_of(R):
    r = np.arange(-R, R + 1, dtype=np.int64)
    si, sj = np.meshgrid(r, r, indexing="ij")
    return np.stack([si.reshape(-1), sj.reshape(-1)], axis=1)          # in the order of sidx


def _misses(targets, mask):
    """targets [..., n, 2]: how many of the n lie outside the grid or off the mask, per leading index."""
    G = mask.shape[0]
    inside = (targets >= 0).all(-1) & (targets < G).all(-1)
    t = np.where(inside[..., None], targets, 0)
    return (~(inside & mask[t[..., 0], t[..., 1]])).sum(-1)


def costs(ca, cb, ma, mb, p, q, cx, cy, R):
    """Step X for one rotation: the cost of every shift, [(2R+1)^2] in the order of sidx."""
    s = shifts_of(R)
    fwd = q + forward(ca - p, cx, cy)                                  # [na,2]
    one = _misses(fwd[None] + s[:, None], mb)
    back = p + inverse(cb[None] - q - s[:, None], cx, cy)              # [shifts,nb,2]
    return one + _misses(back, ma)


def cost_one(ca, cb, G, p, q, cx, cy, si, sj):
    """Step X for one candidate, in Python integers and sets."""
    A_, B_ = set(map(tuple, ca.tolist())), set(map(tuple, cb.tolist()))
    pi, pj, qi, qj, cx, cy = int(p[0]), int(p[1]), int(q[0]), int(q[1]), int(cx), int(cy)
    inside = lambda t: 0 <= t[0] < G and 0 <= t[1] < G      # noqa: E731
    cost = 0
    for i, j in A_:
        di, dj = i - pi, j - pj
        t = (qi + si + rd(di * cx - dj * cy), qj + sj + rd(di * cy + dj * cx))
        cost += not (inside(t) and t in B_)
    for i, j in B_:
        ei, ej = i - qi - si, j - qj - sj
        t = (pi + rd(ei * cx + ej * cy), pj + rd(-ei * cy + ej * cx))
        cost += not (inside(t) and t in A_)
    return cost


def common_frame(fa, fb):
    if fa is None and fb is None:
        return True
    fa, fb = np.asarray(fa, np.int64), np.asarray(fb, np.int64)
    return bool(fa[13] == 1 and fb[13] == 1 and (fa == fb).all())


def motion(state_a, owner_a, state_b, owner_b, table, R, pairs, frame_a=None, frame_b=None):
    """One frame: {"rot": [P,64,4], "best": [P,16]} int32."""
    table = np.asarray(table, np.int64)
    A, P, G = len(table), len(pairs), np.asarray(state_a).shape[0]
    rot = np.tile(np.array(NO_ROW, np.int32), (P, MAX_ROT, 1))
    best = np.zeros((P, 16), np.int32)
    ok = common_frame(frame_a, frame_b)
    for n, (ida, idb) in enumerate(pairs):
        ca, cb = cells_of(state_a, owner_a, ida), cells_of(state_b, owner_b, idb)
        na, nb = (len(ca), len(cb)) if ok else (0, 0)
        status = 0 if not ok else 2 if na == 0 or nb == 0 else 3 if na > MAX_CELLS or nb > MAX_CELLS else 1
        best[n, :7] = (status, -1, 0, 0, 0, na, nb)
        if status != 1:
            continue
        ma, mb = np.zeros((G, G), bool), np.zeros((G, G), bool)
        ma[ca[:, 0], ca[:, 1]] = True
        mb[cb[:, 0], cb[:, 1]] = True
        p, q = pivot(ca), pivot(cb)
        least = None
        for k in range(A):
            c = costs(ca, cb, ma, mb, p, q, int(table[k, 0]), int(table[k, 1]), R)
            s = shifts_of(R)
            keys = [key(c[t], int(s[t, 0]), int(s[t, 1]), k, A, R) for t in range(len(s))]
            v = min(keys)
            cost, _, _, _, si, sj = unkey(v, R)
            rot[n, k] = (cost, si, sj, 0)
            least = v if least is None or v < least else least
        cost, _, _, k, si, sj = unkey(least, R)
        far = [int(rot[n, o, 0]) for o in range(A) if min(abs(o - k), A - abs(o - k)) >= 2]
        best[n] = (1, k, si, sj, cost, na, nb, na + nb - 2 * int((ma & mb).sum()), p[0], p[1], q[0], q[1],
                   q[0] + si - p[0], q[1] + sj - p[1], min(far) if far else -1, 0)
    return {"rot": rot, "best": best}


# ---- the grids --------------------------------------------------------------------------------------------------------
def table(G):
    """An empty table: state 1, owner 0."""
    return np.ones((G, G), np.int32), np.zeros((G, G), np.int32)


def put(grid, cells, a):
    """The cells [n,2] as obstacle cells of id a; cells outside the grid are dropped."""
    st, ow = grid
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    c = c[(c >= 0).all(1) & (c < st.shape[0]).all(1)]
    st[c[:, 0], c[:, 1]], ow[c[:, 0], c[:, 1]] = 2, a
    return grid


L_SHAPE = np.array([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (4, 2)], np.int64)       # a long leg and a short one: no symmetry


def l_pair(G, at, move=(0, 0), turn=0, a=5):
    """Two grids with the L at `at` and, in the second, turned by `turn` quarter turns about its corner cell and moved."""
    c = L_SHAPE.copy()
    for _ in range(turn % 4):
        c = np.stack([-c[:, 1], c[:, 0]], axis=1)        # F of a quarter turn: (di, dj) -> (-dj, di)
    return put(table(G), L_SHAPE + np.asarray(at), a), put(table(G), c + np.asarray(at) + np.asarray(move), a)


def box(i0, i1, j0, j1):
    i, j = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), indexing="ij")
    return np.stack([i.reshape(-1), j.reshape(-1)], axis=1)


def rectangle(G, centre, angle, half):
    """The cells whose centre lies in the rectangle of half extents `half` (cells) about `centre` (grid coordinates), its
    long axis at `angle` from the i axis: [n,2]."""
    i, j = np.meshgrid(np.arange(G) + 0.5, np.arange(G) + 0.5, indexing="ij")
    di, dj = i - centre[0], j - centre[1]
    a = di * np.cos(angle) + dj * np.sin(angle)
    b = -di * np.sin(angle) + dj * np.cos(angle)
    return np.argwhere((np.abs(a) <= half[0]) & (np.abs(b) <= half[1])).astype(np.int64)


def flat_frame(found=1):
    """A frame record of the plane z = 1 m seen from above."""
    F = np.zeros(16, np.int64)
    F[0:3], F[3] = (0, 0, -S), 1000 * S
    F[4:7], F[7:10], F[10:13], F[13] = (S, 0, 0), (0, -S, 0), (0, 0, 1000), found
    return F


def blobs(G, seed, ids=(3, 9, 64, 127)):
    """Two grids of one seeded scene: per id a rectangle at a random pose and, in the second grid, turned and moved a
    little, with a few cells knocked out of both, unknown cells, and cells of other states and owners sprinkled in.
    Returns (state_a, owner_a, state_b, owner_b)."""
    rng = np.random.default_rng(1000 * G + seed)
    ga, gb = table(G), table(G)
    for a in ids:
        half = (rng.uniform(G / 16, G / 7), rng.uniform(G / 32, G / 14))
        c = rng.uniform(G * 0.2, G * 0.8, 2)
        t = rng.uniform(0, np.pi)
        put(ga, rectangle(G, c, t, half), a)
        put(gb, rectangle(G, c + rng.uniform(-2.5, 2.5, 2), t + rng.uniform(-0.8, 0.8), half), a)
    for st, ow in (ga, gb):
        n = max(G * G // 64, 2)
        at = rng.integers(0, G, (n, 2))
        st[at[:, 0], at[:, 1]] = rng.choice(np.array([0, 1, 3, -1, 2], np.int32), n)
        ow[at[:, 0], at[:, 1]] = rng.choice(np.array([0, 128, -5, ids[0], ids[1]], np.int32), n)
    return ga[0], ga[1], gb[0], gb[1]


BLOB_PAIRS = [(3, 3), (9, 9), (64, 64), (127, 127), (3, 9), (9, 3), (5, 5)]        # same ids, crossed ids, an absent id


def ground_truth_cases(n=20, G=64):
    """The accuracy cases: per case (cells_a, cells_b, turn, centre_a, centre_b): a rectangle of half extents 8..14 x
    2.5..5 cells at a random pose, and again after a random turn and a shift of up to 10 cells."""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(n):
        half = (rng.uniform(8, 14), rng.uniform(2.5, 5))
        c = rng.uniform(G / 2 - 4, G / 2 + 4, 2)             # with the move and the half diagonal the cells stay on the grid
        t = rng.uniform(0, np.pi)
        turn = rng.uniform(-np.pi, np.pi)
        move = rng.uniform(-10, 10, 2)
        move *= min(1.0, 10.0 / max(np.hypot(*move), 1e-9))
        out.append((rectangle(G, c, t, half), rectangle(G, c + move, t + turn, half), turn, c, c + move))
    return out
