"""The re-identification contract (include/uoc_hip.h) restated in plain Python integers (numpy for the
votes): what uoc_signature, uoc_sig_similarity and uoc_ident_step must compute, bit for bit.  No torch, no GPU.  Test
infrastructure."""
import numpy as np

NUM = 128
WORDS = 104
HIST, DARK, INTENSITY, HIST_END = 8, 89, 90, 99
MAX_N = 1 << 24
FIELDS = ("pid", "uid", "seen", "hits", "pixels")


def sim_threshold(min_sim):
    return max(1, int(round(float(min_sim) * 65536)))


def size_threshold(min_size):
    return int(round(float(min_size) * 256))


def object_ids(labels):
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 1) & (lab < NUM), lab, 0)


def depth_mm(z):
    """relations.hip's rule on a float32 array: whole millimetres, -1 where there is no depth (NaN included)."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = (z > np.float32(0.0)) & (z <= np.float32(65.0))
    mm = np.rint(np.where(ok, z, np.float32(0.0)) * np.float32(1000.0)).astype(np.int64)
    return np.where(ok, mm, -1)


def chroma_votes(b, g, r, skip_zero=True):
    """The chroma votes of one pixel as [(iu, iv, weight)]; [] when the pixel is dark (s < 48)."""
    b, g, r = int(b), int(g), int(r)
    s = b + g + r
    if s < 48:
        return []
    u, v = (64 * b) // s, (64 * g) // s
    ul, uf, vl, vf = u >> 3, u & 7, v >> 3, v & 7
    out = []
    for du in (0, 1):
        for dv in (0, 1):
            w = (uf if du else 8 - uf) * (vf if dv else 8 - vf)
            if w or not skip_zero:
                out.append((ul + du, vl + dv, w))
    return out


def raw_histogram(bgr):
    """bgr [n,3] integers -> the 104-word row of raw vote sums of these pixels (words 8..98), vectorised."""
    bgr = np.asarray(bgr).astype(np.int64).reshape(-1, 3)
    row = np.zeros(WORDS + 16, dtype=np.int64)      # slack: a zero weight may point past row 8; it adds nothing
    b, g = bgr[:, 0], bgr[:, 1]
    s = bgr.sum(1)
    lit = s >= 48
    sl = np.where(lit, s, 1)
    u, v = np.where(lit, (64 * b) // sl, 0), np.where(lit, (64 * g) // sl, 0)
    ul, uf, vl, vf = u >> 3, u & 7, v >> 3, v & 7
    for du in (0, 1):
        for dv in (0, 1):
            w = (uf if du else 8 - uf) * (vf if dv else 8 - vf) * lit
            np.add.at(row, HIST + (ul + du) * 9 + (vl + dv), w)
    row[DARK] = 64 * int((~lit).sum())
    y = s // 3
    yl, yf = y >> 5, (y & 31) >> 2
    np.add.at(row, INTENSITY + yl, 8 * (8 - yf))
    np.add.at(row, INTENSITY + np.minimum(yl + 1, 8), 8 * yf)       # yf == 0 adds nothing
    return row[:WORDS]


def describe(labels, image, xyz=None):
    """labels [H,W], image [H,W,3] uint8 BGR, xyz [3,H,W] float32 or None -> sig [128,104] int32."""
    ids = object_ids(labels).reshape(-1)
    assert ids.size <= MAX_N
    img = np.asarray(image).reshape(-1, 3)
    zmm = depth_mm(np.asarray(xyz)[2]).reshape(-1) if xyz is not None else np.full(ids.size, -1, dtype=np.int64)
    sig = np.zeros((NUM, WORDS), dtype=np.int64)
    for i in np.unique(ids):
        if i == 0:
            continue
        sel = ids == i
        n = int(sel.sum())
        row = raw_histogram(img[sel])
        z = zmm[sel]
        z = z[z >= 0]
        area = sum(int(v) * int(v) >> 10 for v in z.tolist())
        out = sig[i]
        out[0], out[1], out[2], out[3] = n, z.size, area & 0xFFFFFFFF, area >> 32
        for k in range(HIST, HIST_END):
            h = int(row[k])
            assert h < 2 ** 32
            out[k] = (h * (768 if k <= DARK else 256)) // n
    return as_int32(sig)


def as_int32(a):
    return (np.asarray(a, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def area_of(row):
    return (int(row[2]) & 0xFFFFFFFF) | ((int(row[3]) & 0xFFFFFFFF) << 32)


def similarity(qa, qb):
    """One pair: the histogram intersection, 0 when either has no pixels."""
    if int(qa[0]) <= 0 or int(qb[0]) <= 0:
        return 0
    return int(np.minimum(np.asarray(qa[HIST:HIST_END], dtype=np.int64), np.asarray(qb[HIST:HIST_END], dtype=np.int64)).sum())


def similarity_table(sa, sb):
    sa, sb = np.asarray(sa, dtype=np.int64), np.asarray(sb, dtype=np.int64)
    m = np.minimum(sa[:, None, HIST:HIST_END], sb[None, :, HIST:HIST_END]).sum(2)
    return (m * ((sa[:, 0] > 0)[:, None] & (sb[:, 0] > 0)[None, :])).astype(np.int32)


class ReferenceIdentifier:
    """One stream.  table[e] = [pid, uid, seen, hits, pixels], sigs[e] = the entry's last signature.  events counts what
    happened, for the tests' coverage checks."""

    def __init__(self, min_sim=0.7, min_size=0.25, max_lost=300, q=None, r=None):
        self.q = sim_threshold(min_sim) if q is None else int(q)
        self.r = size_threshold(min_size) if r is None else int(r)
        self.max_lost = int(max_lost)
        self.reset()

    def reset(self):
        self.table = np.zeros((NUM, 5), dtype=np.int64)
        self.sigs = np.zeros((NUM, WORDS), dtype=np.int64)
        self.pids = self.step_index = self.evicted = 0
        self.lut = np.zeros(NUM, dtype=np.int64)
        self.events = dict(reid=0, reid_retired=0, refuse_sim=0, refuse_size=0, forget=0, evict=0, new=0)

    # The decision rules, one method each, so that tests/identity_cases.py can break one at a time (its mutants).
    def passes(self, sim):
        return sim >= self.q

    def areas_agree(self, a_new, a_old):
        if self.r == 0:
            return True
        lo, hi = min(a_new, a_old), max(a_new, a_old)
        return lo != 0 and lo * 256 >= self.r * hi

    def order_key(self, sim, seen, e, s):
        """Larger is better: sim, then seen, then the lower entry, then the lower slot."""
        return (sim, seen, -e, -s)

    def forgotten(self, seen):
        return self.step_index - seen > self.max_lost

    def free_entries(self, freed_now):
        return [e for e in range(1, NUM) if self.table[e, 0] == 0]

    def eviction_key(self, e):
        """Smaller goes first."""
        return (int(self.table[e, 2]), e)

    def step(self, tracks, sig, tracked=None, live_uids=None):
        """tracks [128,5] (uid, age, hits, area, born), sig [128,104]; returns lut [128] (and keeps it).  live_uids: the
        uids of the tracker's live slots, only for the events (a re-identification of a retired track)."""
        tracks, sig = np.asarray(tracks, dtype=np.int64), np.asarray(sig, dtype=np.int64)
        table, sigs = self.table, self.sigs
        self.step_index += 1
        freed = set()
        for e in range(NUM):
            if e == 0 or table[e, 0] == 0:
                table[e], sigs[e] = 0, 0
            elif self.forgotten(int(table[e, 2])):
                table[e], sigs[e] = 0, 0
                freed.add(e)
                self.events["forget"] += 1
        visible = [s for s in range(1, NUM) if tracks[s, 0] != 0 and tracks[s, 1] == 0 and sig[s, 0] > 0]
        ent_of, slot_of = {}, {}
        by_uid = {int(table[e, 1]): e for e in range(1, NUM) if table[e, 0] != 0 and table[e, 1] != 0}
        for s in visible:
            e = by_uid.get(int(tracks[s, 0]))
            if e is not None:
                ent_of[s], slot_of[e] = e, s
        newcomers = [s for s in visible if s not in ent_of]
        lost = [e for e in range(1, NUM) if table[e, 0] != 0 and e not in slot_of]
        cands = []
        for s in newcomers:
            for e in lost:
                sim = similarity(sig[s], sigs[e])
                if not self.passes(sim):
                    if sim > 0:
                        self.events["refuse_sim"] += 1
                    continue
                if not self.areas_agree(area_of(sig[s]), area_of(sigs[e])):
                    self.events["refuse_size"] += 1
                    continue
                cands.append((self.order_key(sim, int(table[e, 2]), e, s), s, e))
        while True:
            open_ = [c for c in cands if c[1] not in ent_of and c[2] not in slot_of]
            if not open_:
                break
            _, s, e = max(open_)
            ent_of[s], slot_of[e] = e, s
            self.events["reid"] += 1
            if live_uids is not None and int(table[e, 1]) not in live_uids:
                self.events["reid_retired"] += 1
            table[e, 1] = tracks[s, 0]
        for s in newcomers:
            if s in ent_of:
                continue
            free = [e for e in self.free_entries(freed) if e not in slot_of]
            if free:
                e = free[0]
            else:
                e = min((e for e in range(1, NUM) if table[e, 0] != 0 and e not in slot_of), key=self.eviction_key)
                self.evicted += 1
                self.events["evict"] += 1
            self.pids += 1
            table[e] = (self.pids, tracks[s, 0], table[e, 2], 0, table[e, 4])
            ent_of[s], slot_of[e] = e, s
            self.events["new"] += 1
        lut = np.zeros(NUM, dtype=np.int64)
        for s, e in ent_of.items():
            table[e, 2] = self.step_index
            table[e, 3] += 1
            table[e, 4] = sig[s, 0]
            sigs[e] = sig[s]
            lut[s] = e
        self.lut = lut
        return lut.astype(np.int32)

    def relabel(self, tracked):
        return self.lut[object_ids(tracked)].astype(np.int32)

    # what the device state must hold
    def state_words(self):
        words = np.zeros(1024 + NUM * WORDS, dtype=np.int64)
        words[:NUM * 5] = self.table.reshape(-1)
        words[640:643] = (self.pids, self.step_index, self.evicted)
        words[1024:] = self.sigs.reshape(-1)
        return as_int32(words)

    def table32(self):
        return as_int32(self.table)
