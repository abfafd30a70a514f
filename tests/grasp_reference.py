"""The definition of uoc_grasp (include/uoc_hip.h) restated with numpy integers, and the grids the tests
run it on.  Nothing here comes from the package's grasp or placement modules: every constant is written out, so a wrong
constant in the package fails a test.

`grasp` is the restatement the GPU tests compare with (one class table per id, the strips by sliding windows and prefix
sums); `grasp_literal` follows the definition sample by sample in plain Python and is what tests/test_grasp_host.py
holds `grasp` against."""
import numpy as np

S = 16384
SHIFT = 14
NUM_IDS = 128
MISS, WIDE, PINCHED, BLOCKED = -1, -2, -3, -4
OWN, FREE, OTHER, OUT, UNKNOWN = 0, 1, 2, 3, 4
LIMITS = {"A": (1, 32), "M": (0, 8), "Wmax": (1, 64), "gap": (0, 4), "F": (1, 8), "Hp": (0, 4)}
DEFAULT = dict(M=2, Wmax=8, gap=1, F=1, Hp=1, unknown_blocks=1)


def direction_table(A):
    k = np.arange(A, dtype=np.float64)
    return np.stack([np.rint(np.cos(np.pi * k / A) * S), np.rint(np.sin(np.pi * k / A) * S)], axis=1).astype(np.int64)


def anchors(state, owner):
    """n [128], ax [128], ay [128] as Python-exact int64 (0 for absent ids and id 0)."""
    n, ax, ay = (np.zeros(NUM_IDS, np.int64) for _ in range(3))
    ii, jj = np.nonzero(state == 2)
    ow = owner[ii, jj].astype(np.int64)
    keep = (ow >= 1) & (ow <= 127)
    ii, jj, ow = ii[keep], jj[keep], ow[keep]
    cnt = np.bincount(ow, minlength=NUM_IDS)
    si = np.bincount(ow, ii, minlength=NUM_IDS).astype(np.int64)             # float64 sums of integers below 2^53: exact
    sj = np.bincount(ow, jj, minlength=NUM_IDS).astype(np.int64)
    for a in range(1, NUM_IDS):
        if cnt[a]:
            n[a] = cnt[a]
            ax[a] = (S * (2 * int(si[a]) + int(cnt[a]))) // (2 * int(cnt[a]))
            ay[a] = (S * (2 * int(sj[a]) + int(cnt[a]))) // (2 * int(cnt[a]))
    return n, ax, ay


def classes(state, owner, a, X, Y, unknown_blocks):
    """The class of the samples (X, Y) (int64 arrays, units of 1/S cell) relative to id a."""
    G = state.shape[0]
    i, j = X >> SHIFT, Y >> SHIFT                       # numpy's >> on int64 is arithmetic: floor
    inside = (i >= 0) & (i < G) & (j >= 0) & (j < G)
    ic, jc = np.clip(i, 0, G - 1), np.clip(j, 0, G - 1)
    st, ow = state[ic, jc].astype(np.int64), owner[ic, jc].astype(np.int64)
    cls = np.full(X.shape, UNKNOWN, np.int8)
    cls[(st == 1) | ((st == 0) & (not unknown_blocks))] = FREE
    cls[(st == 2) & (ow >= 1) & (ow <= 127)] = OTHER
    cls[(st == 2) & (ow == a)] = OWN
    cls[~inside] = OUT
    return cls


def key_of(k, m, w, A, M, Wmax):
    return 1 + (((M - abs(m)) << 24) | ((Wmax - w) << 16) | ((A - 1 - k) << 8) | (1 if m >= 0 else 0))


def check_params(A, M, Wmax, gap, F, Hp, unknown_blocks, dirs):
    for name, v in (("A", A), ("M", M), ("Wmax", Wmax), ("gap", gap), ("F", F), ("Hp", Hp)):
        lo, hi = LIMITS[name]
        assert lo <= v <= hi, (name, v)
    assert unknown_blocks in (0, 1) and np.abs(dirs).max() <= S


def grasp(state, owner, dirs, M, Wmax, gap, F, Hp, unknown_blocks):
    """One frame: state, owner [G,G] integer arrays, dirs [A,2].  Returns {"cand": [128,A,2M+1,2] int32, "best": [128,8]
    int32}."""
    state, owner, dirs = np.asarray(state), np.asarray(owner), np.asarray(dirs, np.int64)
    A = len(dirs)
    check_params(A, M, Wmax, gap, F, Hp, unknown_blocks, dirs)
    NM, R = 2 * M + 1, 2 * Wmax
    E = R + gap + F
    cand = np.zeros((NUM_IDS, A, NM, 2), np.int32)
    best = np.zeros((NUM_IDS, 8), np.int32)
    n, ax, ay = anchors(state, owner)
    t = np.arange(-E, E + 1, dtype=np.int64)[None, None, :]
    l = np.arange(-(M + Hp), M + Hp + 1, dtype=np.int64)[None, :, None]
    cx, cy = dirs[:, 0][:, None, None], dirs[:, 1][:, None, None]
    ks = np.arange(A)
    search = (t[0, 0] >= -R) & (t[0, 0] <= R)
    for a in range(1, NUM_IDS):
        if not n[a]:
            continue
        cls = classes(state, owner, a, ax[a] + t * cx - l * cy, ay[a] + t * cy + l * cx, unknown_blocks)     # [A, lines, T]
        top_key, n_ok, top = 0, 0, None
        for mi in range(NM):
            m = mi - M
            strip = cls[:, mi:mi + 2 * Hp + 1, :]                                 # the lines m-Hp .. m+Hp
            own = (strip == OWN).any(axis=1) & search[None, :]                     # [A, T]
            hit = own.any(axis=1)
            lo = np.where(hit, own.argmax(axis=1), 0)                              # index into t
            hi = np.where(hit, own.shape[1] - 1 - own[:, ::-1].argmax(axis=1), 0)
            w = hi - lo + 1
            squeeze = np.concatenate([np.zeros((A, 1), np.int64), np.cumsum(((strip == OTHER) | (strip == OUT)).any(axis=1), axis=1)], axis=1)
            notfree = np.concatenate([np.zeros((A, 1), np.int64), np.cumsum((strip != FREE).any(axis=1), axis=1)], axis=1)
            reach = gap + F
            for k in ks:
                if not hit[k]:
                    cand[a, k, mi] = (MISS, 0)
                    continue
                tlo = int(lo[k]) - E
                if w[k] > Wmax:
                    code = WIDE
                elif squeeze[k, hi[k] + 1] - squeeze[k, lo[k]]:
                    code = PINCHED
                elif (notfree[k, lo[k]] - notfree[k, lo[k] - reach]) + (notfree[k, hi[k] + 1 + reach] - notfree[k, hi[k] + 1]):
                    code = BLOCKED
                else:
                    code = int(w[k])
                    n_ok += 1
                    key = key_of(int(k), m, code, A, M, Wmax)
                    if key > top_key:
                        top_key, top = key, (1, int(k), m, tlo, code)
                cand[a, k, mi] = (code, tlo)
        best[a] = (top if top else (0, -1, 0, 0, 0)) + (int(ax[a]), int(ay[a]), n_ok)
    return {"cand": cand, "best": best}


def grasp_literal(state, owner, dirs, M, Wmax, gap, F, Hp, unknown_blocks, ids=None):
    """The definition followed sample by sample in Python integers (slow: small grids or a few ids)."""
    state, owner = np.asarray(state), np.asarray(owner)
    G, A = state.shape[0], len(dirs)
    dirs = [(int(c[0]), int(c[1])) for c in dirs]
    check_params(A, M, Wmax, gap, F, Hp, unknown_blocks, np.asarray(dirs))
    R = 2 * Wmax
    cand = np.zeros((NUM_IDS, A, 2 * M + 1, 2), np.int32)
    best = np.zeros((NUM_IDS, 8), np.int32)
    for a in (range(1, NUM_IDS) if ids is None else ids):
        cells = [(i, j) for i in range(G) for j in range(G) if state[i, j] == 2 and owner[i, j] == a] if 1 <= a <= 127 else []
        na = len(cells)
        if na == 0:
            continue
        ax = (S * (2 * sum(c[0] for c in cells) + na)) // (2 * na)
        ay = (S * (2 * sum(c[1] for c in cells) + na)) // (2 * na)

        def cls(k, l, t):
            X, Y = ax + t * dirs[k][0] - l * dirs[k][1], ay + t * dirs[k][1] + l * dirs[k][0]
            i, j = X >> SHIFT, Y >> SHIFT
            if not (0 <= i < G and 0 <= j < G):
                return OUT
            s, o = int(state[i, j]), int(owner[i, j])
            if s == 2:
                return OWN if o == a else (OTHER if 1 <= o <= 127 else UNKNOWN)
            return FREE if s == 1 or (s == 0 and not unknown_blocks) else UNKNOWN

        top_key, top, n_ok = 0, (0, -1, 0, 0, 0), 0
        for k in range(A):
            for m in range(-M, M + 1):
                L = range(m - Hp, m + Hp + 1)
                own = [t for t in range(-R, R + 1) for l in L if cls(k, l, t) == OWN]
                if not own:
                    cand[a, k, m + M] = (MISS, 0)
                    continue
                tlo, thi = min(own), max(own)
                w = thi - tlo + 1
                fingers = list(range(tlo - gap - F, tlo)) + list(range(thi + 1, thi + gap + F + 1))
                if w > Wmax:
                    code = WIDE
                elif any(cls(k, l, t) in (OTHER, OUT) for l in L for t in range(tlo, thi + 1)):
                    code = PINCHED
                elif any(cls(k, l, t) != FREE for l in L for t in fingers):
                    code = BLOCKED
                else:
                    code = w
                    n_ok += 1
                    key = key_of(k, m, w, A, M, Wmax)
                    if key > top_key:
                        top_key, top = key, (1, k, m, tlo, w)
                cand[a, k, m + M] = (code, tlo)
        best[a] = top + (ax, ay, n_ok)
    return {"cand": cand, "best": best}


def code_counts(cand_row):
    """{code class: count} over the (k, m) candidates of one id: 'ok' for the positive codes."""
    c = cand_row[..., 0]
    return {"ok": int((c > 0).sum()), MISS: int((c == MISS).sum()), WIDE: int((c == WIDE).sum()),
            PINCHED: int((c == PINCHED).sum()), BLOCKED: int((c == BLOCKED).sum())}


# ---- grids ------------------------------------------------------------------------------------------------------------
def table(G, fill=1):
    return np.full((G, G), fill, np.int32), np.zeros((G, G), np.int32)


def put(st, ow, mask, a):
    st[mask] = 2
    ow[mask] = a


def box8():
    """An 8x8 table with one 2x4 box of id 1: rows 3..4, columns 2..5."""
    st, ow = table(8)
    st[3:5, 2:6] = 2
    ow[3:5, 2:6] = 1
    return st, ow


def scene64():
    """A 64x64 table: 1 a 20x5 box rotated by 30 degrees, 2 a disc of radius 3, 3 a disc of radius 8, 4 and 5 two touching
    4x6 boxes, 6 an L shape."""
    G = 64
    st, ow = table(G)
    I, J = np.meshgrid(np.arange(G) + .5, np.arange(G) + .5, indexing="ij")
    th = np.deg2rad(30)
    u, v = (I - 32) * np.cos(th) + (J - 32) * np.sin(th), -(I - 32) * np.sin(th) + (J - 32) * np.cos(th)
    put(st, ow, (abs(u) <= 10) & (abs(v) <= 2.5), 1)
    put(st, ow, (I - 12) ** 2 + (J - 12) ** 2 <= 9, 2)
    put(st, ow, (I - 50) ** 2 + (J - 14) ** 2 <= 64, 3)
    st[10:14, 40:46], ow[10:14, 40:46] = 2, 4
    st[14:18, 40:46], ow[14:18, 40:46] = 2, 5
    st[44:56, 44:47], ow[44:56, 44:47] = 2, 6
    st[53:56, 47:56], ow[53:56, 47:56] = 2, 6
    return st, ow


def random_grid(G, seed, blobs=None, noise=0.03, noise_ids=None):
    """A seeded grid: table with patches of unknown, 3-6 convex blobs (ellipses and rotated boxes) with ids drawn from
    1..127, and `noise` of the cells redrawn at random: states 0..3 and owners -1..129 (out-of-contract values included).
    With `noise_ids` the redrawn owners come from -1, 0, 128, 129 and that many ids of 1..127 instead: the same share of
    redrawn cells with fewer present ids, which is what the reference's time grows with."""
    rng = np.random.default_rng(seed)
    st, ow = table(G)
    I, J = np.meshgrid(np.arange(G) + .5, np.arange(G) + .5, indexing="ij")
    for _ in range(3):                                       # unknown patches: occlusion shadows
        ci, cj, r = rng.uniform(0, G, 2).tolist() + [rng.uniform(1, max(2, G / 6))]
        st[(I - ci) ** 2 + (J - cj) ** 2 <= r * r] = 0
    nb = int(rng.integers(3, 7)) if blobs is None else blobs
    ids = rng.choice(np.arange(1, 128), size=nb, replace=False)
    for a in ids:
        ci, cj = rng.uniform(0, G, 2)
        ra, rb = rng.uniform(0.6, max(1.0, G / 8)), rng.uniform(0.6, max(1.0, G / 20))
        th = rng.uniform(0, np.pi)
        u, v = (I - ci) * np.cos(th) + (J - cj) * np.sin(th), -(I - ci) * np.sin(th) + (J - cj) * np.cos(th)
        mask = ((u / ra) ** 2 + (v / rb) ** 2 <= 1) if rng.random() < 0.5 else ((abs(u) <= ra) & (abs(v) <= rb))
        put(st, ow, mask, int(a))
    redraw = rng.random((G, G)) < noise
    st[redraw] = rng.integers(0, 4, int(redraw.sum()))
    if noise_ids is None:
        ow[redraw] = rng.integers(-1, 130, int(redraw.sum()))
    else:
        pool = np.concatenate([[-1, 0, 128, 129], rng.choice(np.arange(1, 128), size=noise_ids, replace=False)])
        ow[redraw] = rng.choice(pool, int(redraw.sum()))
    ow[(st != 2) & ~redraw] = 0
    return st, ow


def case_border():
    """Objects at the grid's border: id 1 in a corner (OUT in the finger zone), id 2 a bar in the last row (a line cannot
    leave a square and come back, but a pad of several lines can: one line of the strip lies outside the grid while
    another crosses the bar: OUT inside [tlo, thi])."""
    st, ow = table(16)
    st[0:2, 0:3], ow[0:2, 0:3] = 2, 1
    st[15, 6:10], ow[15, 6:10] = 2, 2
    return st, ow


def case_widths(Wmax=8):
    """Bars of width Wmax (id 1) and Wmax + 1 (id 2) along j, 2 cells thick."""
    st, ow = table(64)
    st[10:12, 10:10 + Wmax], ow[10:12, 10:10 + Wmax] = 2, 1
    st[30:32, 10:11 + Wmax], ow[30:32, 10:11 + Wmax] = 2, 2
    return st, ow


def case_far_fingers():
    """id 1: two cells 16 apart in a row, so along the row w = 17 with nothing of its own in between: t = -8..8.  A cell of
    id 2 two cells past one end, at t = 10: in the finger zone only when gap + F >= 2.  Everything lies inside the search
    range (R >= 34 wherever the candidate is not WIDE); case_beyond_range has the zones that leave it."""
    st, ow = table(32)
    st[16, 8], ow[16, 8] = 2, 1
    st[16, 24], ow[16, 24] = 2, 1
    st[16, 26], ow[16, 26] = 2, 2
    return st, ow


def case_beyond_range():
    """Finger zones that reach beyond the search range.  id 1: one cell at (16, 16); at Wmax = 1, gap = 4, F = 8 the range
    is t = -2..2 and the zones are t = -12..-1 and 1..12.  A cell of id 2 at (16, 22), t = 6 along j, on one side only, and
    an unknown cell at (5, 16), t = -11 along i.  id 3: a 2-cell bar in row 26, columns 13..14: t = -1..0 along j; at Wmax = 2
    (R = 4) the zones are t = -13..-2 and 1..12, columns 1..12 and 15..26, and a cell of state 3 sits at (26, 25), t = 11."""
    st, ow = table(32)
    st[16, 16], ow[16, 16] = 2, 1
    st[16, 22], ow[16, 22] = 2, 2
    st[5, 16] = 0
    st[26, 13:15], ow[26, 13:15] = 2, 3
    st[26, 25] = 3
    return st, ow


def case_single_cells():
    """Ids with one cell each: 5 in the middle, 127 next to the border, 1 in a corner."""
    st, ow = table(16)
    st[8, 8], ow[8, 8] = 2, 5
    st[1, 14], ow[1, 14] = 2, 127
    st[0, 0], ow[0, 0] = 2, 1
    return st, ow


def case_all_ids():
    """127 ids at once on a 64x64 table: 2x2 boxes on a 12 x 11 lattice, 5 cells apart."""
    st, ow = table(64)
    for a in range(1, 128):
        r, c = divmod(a - 1, 12)
        st[2 + 5 * r:4 + 5 * r, 2 + 5 * c:4 + 5 * c] = 2
        ow[2 + 5 * r:4 + 5 * r, 2 + 5 * c:4 + 5 * c] = a
    return st, ow


def case_empty():
    st, ow = table(16, 0)
    return st, ow


def case_all_obstacle():
    st, ow = table(16, 2)
    ow[:, :8], ow[:, 8:] = 3, 9
    return st, ow


def case_out_of_contract():
    """A 2x3 box of id 7 with, around it, state-2 cells of owner 0 and 128 and cells of state 3 and -1: all unknown; and
    cells of owner 7 whose state is not 2: not the object's."""
    st, ow = table(24)
    st[10:12, 10:13], ow[10:12, 10:13] = 2, 7
    st[10, 14], ow[10, 14] = 2, 0
    st[11, 8], ow[11, 8] = 2, 128
    st[8, 11], ow[8, 11] = 3, 0
    st[13, 11], ow[13, 11] = -1, 7
    st[10, 16], ow[10, 16] = 1, 7
    st[4, 4], ow[4, 4] = 2, -5
    return st, ow


def case_ring():
    """A ring of id 1 around a disc of id 2: the ring's anchor lies on a cell of the disc."""
    st, ow = table(32)
    I, J = np.meshgrid(np.arange(32) + .5, np.arange(32) + .5, indexing="ij")
    d2 = (I - 16) ** 2 + (J - 16) ** 2
    put(st, ow, (d2 <= 81) & (d2 >= 49), 1)
    put(st, ow, d2 <= 9, 2)
    return st, ow


ENGINEERED = {"box8": box8, "scene64": scene64, "border": case_border, "widths": case_widths, "far_fingers": case_far_fingers,
              "beyond_range": case_beyond_range, "single_cells": case_single_cells, "all_ids": case_all_ids, "empty": case_empty,
              "all_obstacle": case_all_obstacle, "out_of_contract": case_out_of_contract, "ring": case_ring}
