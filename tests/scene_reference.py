"""Plain Python / numpy restatement of uoc_scene_step and uoc_scene_reset (include/uoc_hip.h, rules L to Q): the
semantics the GPU tests check against.  Integers only.  The distance transform is the all-pairs definition
(placement_reference.edt_brute) up to BRUTE_MAX_G cells per side and the separable one above it (the host test holds
the two together); a query is answered by sorting every candidate.  `broken` names one rule to get wrong on purpose:
the host test shows that the claim named for that rule then fails.  Also the seeded sequences of the GPU tests."""
import numpy as np

from tests import placement_reference as P15

NUM_IDS = 128
META_WORD, MEM_WORD = 32, 48            # int32 words of a stream's state before its meta / memory words
MAX_AGE = 32767
SAME, APPEARED, VANISHED, REOWNED = 0, 1, 2, 3
ID_FIELDS = ("cells_now", "cells_kept", "oldest", "appeared", "vanished", "reowned_in", "reowned_out", "forgotten")
INFO_FIELDS = ("status", "steps", "observed", "kept", "forgotten", "appeared", "vanished", "reowned")
OUTPUTS = ("state", "owner", "dist2", "age", "change", "ids", "info", "answers")
BRUTE_MAX_G = 64
BREAKS = ("lattice_found", "lattice_compare", "lattice_store", "normalise_state", "normalise_owner", "age_limit", "drop",
          "drop_owner0", "appeared", "vanished", "reowned", "unknown_memory", "oldest", "forgotten_once", "clearance", "query")


def new_state(B, G):
    """int32 [B, 48 + G*G], all zero: B reset streams."""
    return np.zeros((B, MEM_WORD + G * G), np.int32)


def reset(state, which=-1):
    if which < 0:
        state[:] = 0
    else:
        state[which] = 0


def lattice(state_b):
    return state_b[:META_WORD].view(np.int64)


def pack(ms, mo, ma):
    return (np.asarray(ms, np.int64) | (np.asarray(mo, np.int64) << 8) | (np.asarray(ma, np.int64) << 16)).astype(np.int32)


def unpack(words):
    w = np.asarray(words).astype(np.int64)
    return w & 0xFF, (w >> 8) & 0xFF, w >> 16


def drop_words(ids):
    """int32 [4]: the 128-bit drop mask with the bits of `ids` set."""
    w = np.zeros(4, np.uint32)
    for a in ids:
        assert 0 <= int(a) < NUM_IDS
        w[int(a) >> 5] |= np.uint32(1) << np.uint32(int(a) & 31)
    return w.view(np.int32)


_CLEARANCE = {}


def clearance(state, unknown_blocks, brute=None):
    """Rule E.  A sequence often meets the same fused grid again: the last few transforms are kept by their blocking bits."""
    blocking = (state == 2) | ((state == 0) & bool(unknown_blocks))
    if brute is None:
        brute = state.shape[0] <= BRUTE_MAX_G
    key = (blocking.shape[0], bool(brute), np.packbits(blocking).tobytes())
    if key not in _CLEARANCE:
        if len(_CLEARANCE) >= 8:
            _CLEARANCE.clear()
        _CLEARANCE[key] = P15.edt_brute(blocking) if brute else P15.edt(blocking)
    return _CLEARANCE[key].copy()


def step_one(st, state_cur, owner_cur, frame, drop, max_age, unknown_blocks, queries=(), broken=None):
    """One stream, one step.  st: its state words int32 [48 + G*G], updated in place.  state_cur, owner_cur [G,G]
    integers; frame: int64 [16] or None; drop: int32 [4] or None.  Returns a dict of OUTPUTS."""
    assert broken is None or broken in BREAKS
    G = state_cur.shape[0]
    Q = len(queries)
    meta = st[META_WORD:MEM_WORD]
    steps = int(meta[0])
    # L
    status = 1
    if frame is not None:
        F = np.asarray(frame, np.int64).reshape(16)
        found = int(F[13]) != 0 if broken == "lattice_found" else int(F[13]) == 1
        if not found:
            z = np.zeros((G, G), np.int32)
            info = np.zeros(8, np.int32)
            info[1] = steps
            return dict(state=z, owner=z.copy(), dist2=z.copy(), age=z - 1, change=z.copy(), ids=np.zeros((NUM_IDS, 8), np.int32),
                        info=info, answers=np.array([P15.NO_ANSWER] * Q, np.int32).reshape(Q, 4))
        words = 13 if broken == "lattice_compare" else 16
        if steps > 0 and not np.array_equal(lattice(st)[:words], F[:words]):
            status = 2
    ms, mo, ma = unpack(st[MEM_WORD:].reshape(G, G))
    if status == 2:
        ms, mo, ma = (np.zeros((G, G), np.int64) for _ in range(3))
    # N
    sc, oc = np.asarray(state_cur).astype(np.int64), np.asarray(owner_cur).astype(np.int64)
    s = np.where((sc == 1) | (sc == 2), sc, 0)
    if broken == "normalise_state":
        s = np.where(sc > 0, np.minimum(sc, 2), 0)
    o = np.where((s == 2) & (oc >= 1) & (oc <= 127), oc, 0)
    if broken == "normalise_owner":
        o = np.where(s == 2, oc & 127, 0)
    # U
    bits = np.zeros(NUM_IDS, bool)
    if drop is not None:
        w = np.asarray(drop, np.int32).reshape(4).view(np.uint32)
        bits = np.array([(int(w[a >> 5]) >> (a & 31)) & 1 for a in range(NUM_IDS)], bool)
    if broken == "drop":
        bits[:] = False
    observed = s != 0
    dropped = bits[mo] & ((ms != 0) if broken == "drop_owner0" else (ms == 2))
    young = (ma <= max_age) if broken == "age_limit" else (ma < max_age)
    kept = ~observed & (ms != 0) & young & ~dropped
    forgotten = ~observed & (ms != 0) & ~kept
    ns = np.where(observed, s, np.where(kept, ms, 0))
    no = np.where(observed, o, np.where(kept, mo, 0))
    na = np.where(kept, ma + 1, 0)
    age = np.where(observed, 0, np.where(kept, ma + 1, -1))
    change = np.zeros((G, G), np.int64)
    app = observed & (ms == 1) & (s == 2)
    van = observed & (ms == 2) & (s == 1)
    reo = observed & (ms == 2) & (s == 2) & (mo != o)
    if broken == "unknown_memory":
        app |= observed & (ms == 0) & (s == 2)
    if broken != "appeared":
        change[app] = APPEARED
    if broken != "vanished":
        change[van] = VANISHED
    if broken != "reowned":
        change[reo] = REOWNED
    app, van, reo = change == APPEARED, change == VANISHED, change == REOWNED
    # T
    ids = np.zeros((NUM_IDS, 8), np.int64)
    count = lambda mask, who: np.bincount(who[mask].reshape(-1), minlength=NUM_IDS)[:NUM_IDS]      # noqa: E731
    ids[:, 0] = count(observed & (s == 2), o)
    ids[:, 1] = count(kept & (ms == 2), mo)
    for a in np.unique(mo[kept & (ms == 2)]):
        ages = age[kept & (ms == 2) & (mo == a)]
        ids[a, 2] = ages.min() if broken == "oldest" else ages.max()
    ids[:, 3] = count(app, o)
    ids[:, 4] = count(van, mo)
    ids[:, 5] = count(reo, o)
    ids[:, 6] = count(reo, mo)
    ids[:, 7] = count(forgotten & (ms == 2), mo)
    info = np.array([status, steps + 1, observed.sum(), kept.sum(), forgotten.sum(), app.sum(), van.sum(), reo.sum()], np.int64)
    # the state
    new = pack(ns, no, na).reshape(-1)
    if broken == "forgotten_once":
        new = np.where(forgotten.reshape(-1), pack(ms, mo, ma).reshape(-1), new)
    st[MEM_WORD:] = new
    if frame is not None and (steps == 0 or status == 2) and broken != "lattice_store":
        lattice(st)[:] = F
    meta[0] = steps + 1
    meta[1] += status == 2
    # E, Q
    dist2 = clearance(ns, 0 if broken == "clearance" else unknown_blocks)
    cand = np.where(ns == 2, 1, 0) if broken == "query" else ns
    answers = np.array([P15.answer(cand, dist2, q) for q in queries], np.int32).reshape(Q, 4)
    return dict(state=ns.astype(np.int32), owner=no.astype(np.int32), dist2=dist2.astype(np.int32), age=age.astype(np.int32),
                change=change.astype(np.int32), ids=ids.astype(np.int32), info=info.astype(np.int32), answers=answers)


def step(state, state_cur, owner_cur, frame, drop, max_age, unknown_blocks, queries=(), broken=None):
    """B streams.  state int32 [B, 48 + G*G], updated in place; state_cur, owner_cur [B,G,G]; frame int64 [B,16] or None;
    drop int32 [B,4] or None.  Returns a dict of OUTPUTS, each stacked over the streams."""
    outs = [step_one(state[b], state_cur[b], owner_cur[b], None if frame is None else frame[b], None if drop is None else drop[b],
                     max_age, unknown_blocks, queries, broken) for b in range(len(state))]
    return {k: np.stack([o[k] for o in outs]) for k in OUTPUTS}


# ---- grids and sequences ------------------------------------------------------------------------------------------------
def table(G):
    """(state, owner) [G,G] int32: every cell table."""
    return np.ones((G, G), np.int32), np.zeros((G, G), np.int32)


def put(grid, box, ident, state=2):
    """A copy of (state, owner) with the cells [i0, i1) x [j0, j1) of `box` set to `state` (an obstacle of `ident`)."""
    s, o = grid[0].copy(), grid[1].copy()
    i0, i1, j0, j1 = box
    s[i0:i1, j0:j1] = state
    o[i0:i1, j0:j1] = ident if state == 2 else 0
    return s, o


def blank(grid, box):
    return put(grid, box, 0, state=0)


def record(seed=0, found=1):
    """A frame record int64 [16] as uoc_placement stores it, distinct per seed."""
    F = P15.frame_record(P15.flat_plane())
    F[10] += seed
    F[13] = found
    return F


def blobs(G, seed, n=6):
    """(state, owner) [G,G]: a table with a border of unknown cells, `n` rectangles owned by ids 1..n (the last one without
    an id) and a few unknown holes."""
    rng = np.random.default_rng(seed)
    g = table(G)
    g = blank(g, (0, 1, 0, G))
    for k in range(n):
        h, w = int(rng.integers(1, max(2, G // 6))), int(rng.integers(1, max(2, G // 6)))
        i0, j0 = int(rng.integers(1, G - h)), int(rng.integers(0, G - w))
        g = put(g, (i0, i0 + h, j0, j0 + w), k + 1 if k + 1 < n else 0)
    for _ in range(max(2, G // 8)):
        i0, j0 = int(rng.integers(0, G)), int(rng.integers(0, G))
        g = blank(g, (i0, i0 + 1, j0, j0 + 1))
    return g


def sequence(G, seed, steps=6):
    """A list of `steps` frames (state, owner, drop ids): seeded blobs under a blank rectangle that moves across the grid;
    from the third frame on blob 1 stands elsewhere while its old place is hidden, and the fourth frame drops its id."""
    rng = np.random.default_rng(1000 + seed)
    base = blobs(G, seed)
    i1 = np.nonzero((base[0] == 2) & (base[1] == 1))
    frames = []
    for t in range(steps):
        g = base
        if t >= 2 and len(i1[0]):
            s, o = g[0].copy(), g[1].copy()
            s[i1], o[i1] = 1, 0
            g = put((s, o), (G - 3, G - 1, 2, 5), 1)
        w = max(2, G // 4)
        j0 = (t * max(1, G // 6)) % (G - w)
        i0 = int(rng.integers(0, G // 2))
        g = blank(g, (i0, i0 + G // 2, j0, j0 + w))
        if t >= 2 and len(i1[0]):                                  # the old place of blob 1 stays hidden
            s, o = g[0].copy(), g[1].copy()
            s[i1], o[i1] = 0, 0
            g = (s, o)
        frames.append((g[0], g[1], [1] if t == 3 else []))
    return frames


def hand_sequences(G=8):
    """{name: (frames, keyword arguments)}: the hand sequences of tests/test_scene_host.py as one stream each.  A frame is
    (state, owner, drop ids or None, record or None)."""
    full = put(put(blank(table(G), (0, 2, 0, 2)), (3, 5, 3, 5), 5), (6, 7, 1, 3), 0)
    hid = blank(full, (2, 6, 2, 6))
    moved = blank(blank(put(full, (0, 2, 5, 7), 5), (3, 5, 3, 5)), (6, 7, 1, 3))
    shifted = put(put(full, (3, 5, 3, 5), 0, state=1), (3, 5, 4, 6), 5)
    before = blank(put(table(G), (1, 2, 0, G), 3), (2, 3, 0, G))
    now = before
    for j, (state, ident) in enumerate([(1, 0), (2, 3), (2, 4), (2, 0), (0, 0)]):
        now = put(now, (0, 3, j, j + 1), ident, state=state)
    odd = (table(G)[0].copy(), table(G)[1].copy())
    odd[0][0, :6], odd[1][0, :6], odd[1][1, 0] = [3, -1, 2, 2, 2, 2], [7, 7, 0, 128, -5, 127], 9
    rec, other = record(), record(seed=1)
    fr = lambda g, drop=None, r=rec: (g[0], g[1], drop, r)        # noqa: E731
    return {
        "same_twice": ([fr(full), fr(full)], dict(max_age=5)),
        "blank_then_forgotten": ([fr(full)] + [fr(hid)] * 5, dict(max_age=3)),
        "differencing": ([fr(full), fr(hid), fr(shifted), fr(full)], dict(max_age=0)),
        "moved_kept": ([fr(full), fr(moved), fr(moved)], dict(max_age=5)),
        "moved_drop_id": ([fr(full), fr(moved, [5])], dict(max_age=5)),
        "moved_drop_zero": ([fr(full), fr(moved, [0])], dict(max_age=5)),
        "drop_everything": ([fr(full), fr(blank(full, (5, 8, 0, 8)), list(range(NUM_IDS)))], dict(max_age=5)),
        "change_codes": ([fr(before), fr(now), fr(before)], dict(max_age=5)),
        "odd_words": ([fr(odd), fr(blank(odd, (0, 2, 0, 8)))], dict(max_age=5, unknown_blocks=0)),
        "no_lattice": ([fr(full), fr(hid, None, record(found=0)), fr(hid, None, record(found=2)), fr(hid)], dict(max_age=5)),
        "restart": ([fr(full), fr(hid, None, other), fr(hid, None, other), fr(full, None, rec)], dict(max_age=5)),
        "null_frame": ([fr(full, None, None), fr(hid, None, None), fr(hid, None, rec), fr(hid, None, None)], dict(max_age=5)),
    }
