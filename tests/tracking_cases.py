"""Engineered sequences for the tracker: every decision rule of uoc_track_step (include/uoc_hip.h) on an
input where that rule, and nothing else, decides the result.  Test infrastructure: no torch, no GPU.

A case is a function returning dict(frames=[T,H,W] int32, min_iou, max_age, claim): `claim(run)` asserts on the reference
run (run_case) what the case is for, with the answer written down wherever it can be.  tests/test_tracking_cases_host.py
proves the claims on the CPU and that every mutant of the rules (MutantTracker) is told apart from the true rule by the
cases named for it; tests/test_tracking_cases_gpu.py runs the same frames through the kernels.

All maps are single rows: the tracker is per pixel, geometry does not enter."""
import numpy as np

from tests.tracking_reference import NUM, ReferenceTracker, iou_threshold

INT_MIN = -2 ** 31


def line(n, *spans):
    img = np.zeros((1, n), dtype=np.int32)
    for a, b, v in spans:
        img[0, a:b] = v
    return img


def case(frames, min_iou, max_age, claim):
    frames = np.stack([np.asarray(f, dtype=np.int32) for f in frames])
    assert frames.ndim == 3
    return dict(frames=frames, min_iou=min_iou, max_age=max_age, claim=claim)


def run_case(c, tracker=ReferenceTracker, **kw):
    """Per step (out uint8, lut, table, mem uint8, meta) — what tests.test_tracking_gpu.assert_state takes — and the
    tracker after the last step."""
    ref = tracker(c["min_iou"], c["max_age"], **kw)
    steps = []
    for frame in c["frames"]:
        out = ref.step(frame)
        steps.append((out.astype(np.uint8), ref.lut.astype(np.int32), ref.table32(), ref.mem.astype(np.uint8), ref.meta()))
    return steps, ref


def live(table):
    return {s: int(table[s, 0]) for s in range(NUM) if table[s, 0]}


# ---- the hand-made sequences of tests/test_tracking_host.py (its assertions stay there) -----------------------------------
def tie_larger_inter():
    """Track 1 has 6 pixels; id 5 (2 px, all inside: 2/6) and id 9 (10 px, 4 inside: 4/12) tie at 1/3."""
    def claim(run):
        assert run[1][1][9] == 1 and run[1][1][5] == 2
    return case([line(40, (10, 16, 1)), line(40, (10, 12, 5), (12, 22, 9))], 0.3, 5, claim)


def tie_lower_track():
    """Tracks 1 and 2 (4 px each) against one id covering the inner halves of both (2/6 each, equal inter)."""
    def claim(run):
        assert run[1][1][6] == 1 and run[1][2][2].tolist() == [2, 1, 1, 4, 0]
    return case([line(40, (10, 14, 3), (14, 18, 8)), line(40, (12, 16, 6))], 0.3, 5, claim)


def tie_lower_id():
    """One track (8 px) against ids 4 and 7, each 2 px inside plus 2 outside (2/10 each)."""
    def claim(run):
        assert run[1][1][4] == 1 and run[1][1][7] == 2
    return case([line(40, (10, 18, 1)), line(40, (8, 12, 7), (16, 20, 4))], 0.2, 5, claim)


def threshold_equal_large(area=None):
    """q = 19661: the id covers 65536 pixels and the track's `area` pixels all lie inside, IoU = area / 65536.  area = q is
    exact equality and matches."""
    q = iou_threshold(0.3)
    area = q if area is None else area

    def claim(run):
        matched = area >= q
        assert (run[1][2][1].tolist() == [1, 0, 2, 65536, 0]) == matched
        assert (run[1][2][2, 0] == 2) == (not matched) and run[1][4]["next_uid"] == (2 if matched else 3)
    return case([line(70000, (0, area, 1)), line(70000, (0, 65536, 1))], 0.3, 5, claim)


def threshold_equal_large_miss():
    """One pixel less in the track: 19660 / 65536 is below q / 65536."""
    return threshold_equal_large(iou_threshold(0.3) - 1)


def threshold_half_line():
    """min_iou 0.5, inter 2, union 4."""
    def claim(run):
        assert run[1][4]["next_uid"] == 2
    return case([line(16, (0, 3, 1)), line(16, (1, 4, 1))], 0.5, 5, claim)


def threshold_below_half():
    """min_iou 0.5, inter 66, union 134."""
    def claim(run):
        assert run[1][4]["next_uid"] == 3 and live(run[1][2]) == {1: 1, 2: 2} and run[1][2][1, 1] == 1
    return case([line(300, (0, 100, 1)), line(300, (34, 134, 1))], 0.5, 5, claim)


def overflow_128th():
    """127 live tracks; raw id 127 moves to where it overlaps nothing: a 128th object, dropped until track 127 retires."""
    def frame(moved):
        img = np.zeros((4, 128), dtype=np.int32)
        img[0, 1:128] = np.arange(1, 128)
        if moved:
            img[0, 127] = 0
            img[2, 5] = 127
        return img

    def claim(run):
        assert [s[4]["dropped"] for s in run] == [0, 1, 2, 2]
        assert run[3][2][127].tolist() == [128, 0, 1, 1, 3] and run[3][0][2, 5] == 127
    return case([frame(False), frame(True), frame(True), frame(True)], 0.3, 2, claim)


# ---- ties over all lanes and rows of the wave's arg-max ----------------------------------------------------------------
DOMINO_W = 512


def tie_domino():
    """Step 0: 127 tracks of 4 px, [4k, 4k+4).  Step 1: 126 ids, span j = [4j+2, 4j+6) with id (5j) % 127 + 1, covers the
    upper half of track j+1 and the lower half of track j+2: 252 candidates, every one IoU 2/6 and intersection 2.  The
    lowest track goes first and has one candidate left each time, so span j goes to track j+1 and track 127 stays alone."""
    f0 = line(DOMINO_W, *[(4 * k, 4 * k + 4, k + 1) for k in range(127)])
    ids = [(5 * j) % 127 + 1 for j in range(126)]
    assert len(set(ids)) == 126
    f1 = line(DOMINO_W, *[(4 * j + 2, 4 * j + 6, ids[j]) for j in range(126)])

    def claim(run):
        _, lut, table, mem, meta = run[1]
        want = np.zeros(NUM, dtype=np.int32)
        for j in range(126):
            want[ids[j]] = j + 1
        assert np.array_equal(lut, want)
        assert all(table[t].tolist() == [t, 0, 2, 4, 0] for t in range(1, 127)) and table[127].tolist() == [127, 1, 1, 4, 0]
        assert meta == dict(next_uid=128, step=2, dropped=0)
        assert mem[0, 506:508].tolist() == [127, 127] and mem[0, 502:506].tolist() == [126] * 4
    return case([f0, f1], 0.3, 5, claim)


MANY_TRACKS = (1, 33, 63, 64, 65, 66, 99, 100)
MANY_SMALL = (3, 20, 62, 63, 64, 65, 90, 110)      # 2 px, all inside its track: 2/6
MANY_LARGE = tuple(c + 8 for c in MANY_SMALL)      # 10 px, 4 inside: 4/12; the larger id, so "lower id" would say no


def tie_larger_inter_many():
    """The 2/6 versus 4/12 pattern at eight of 100 tracks on both sides of slot 64 in one frame.  The larger intersection
    takes the track; the small ids are born into slots 101.. in ascending order."""
    f0 = line(1400, *[(14 * k, 14 * k + 6, k + 1) for k in range(100)])
    spans = []
    for t, a, b in zip(MANY_TRACKS, MANY_SMALL, MANY_LARGE):
        p = 14 * (t - 1)
        spans += [(p, p + 2, a), (p + 2, p + 12, b)]
    f1 = line(1400, *spans)

    def claim(run):
        _, lut, table, _, meta = run[1]
        want = np.zeros(NUM, dtype=np.int32)
        for i, (t, a, b) in enumerate(zip(MANY_TRACKS, MANY_SMALL, MANY_LARGE)):
            want[b], want[a] = t, 101 + i
            assert table[t].tolist() == [t, 0, 2, 10, 0] and table[101 + i].tolist() == [101 + i, 0, 1, 2, 1]
        assert np.array_equal(lut, want) and meta == dict(next_uid=109, step=2, dropped=0)
    return case([f0, f1], 0.3, 5, claim)


HIGH_PAIRS = {1: (70, 100), 2: (10, 90), 64: (64, 65), 65: (63, 127), 70: (126, 125)}   # track: (left id, right id)


def tie_lower_id_high():
    """One track of 8 px against two ids, each 2 px inside plus 2 outside (2/10 each, min_iou 0.2), at
    tracks on both sides of 64: both ids >= 64, one below and one above, 63 against 127, and the lower id on the right."""
    f0 = line(840, *[(12 * k + 2, 12 * k + 10, k + 1) for k in range(70)])
    spans = []
    for t, (a, b) in HIGH_PAIRS.items():
        p = 12 * (t - 1)
        spans += [(p, p + 4, a), (p + 8, p + 12, b)]
    f1 = line(840, *spans)

    def claim(run):
        _, lut, table, _, meta = run[1]
        want = np.zeros(NUM, dtype=np.int32)
        losers = sorted(max(p) for p in HIGH_PAIRS.values())
        for t, p in HIGH_PAIRS.items():
            want[min(p)] = t
            want[max(p)] = 71 + losers.index(max(p))
        assert np.array_equal(lut, want) and meta == dict(next_uid=76, step=2, dropped=0)
        assert sorted(live(table)) == list(range(1, 76))
    return case([f0, f1], 0.2, 5, claim)


# ---- the threshold ------------------------------------------------------------------------------------------------------
def threshold_equal_small():
    """min_iou 0.25, q = 16384.  Track 1 = [0,2) against id 7 = [1,4): inter 1, union 4, equality, matches.  Track 2 =
    [8,10) against id 3 = [9,13): one more pixel in the union, no match: track 2 ages and id 3 is born as 3."""
    assert iou_threshold(0.25) == 16384

    def claim(run):
        _, lut, table, _, meta = run[1]
        assert lut[7] == 1 and lut[3] == 3 and lut.sum() == 4 and meta == dict(next_uid=4, step=2, dropped=0)
        assert table[1].tolist() == [1, 0, 2, 3, 0] and table[2].tolist() == [2, 1, 1, 2, 0] and table[3].tolist() == [3, 0, 1, 4, 1]
    return case([line(16, (0, 2, 1), (8, 10, 2)), line(16, (1, 4, 7), (9, 13, 3))], 0.25, 5, claim)


def threshold_equal_half():
    """The same at min_iou 0.5: inter 2, union 4 matches; inter 2, union 5 does not."""
    def claim(run):
        _, lut, table, _, meta = run[1]
        assert lut[7] == 1 and lut[3] == 3 and lut.sum() == 4 and meta == dict(next_uid=4, step=2, dropped=0)
        assert table[1].tolist() == [1, 0, 2, 3, 0] and table[2].tolist() == [2, 1, 1, 3, 0] and table[3].tolist() == [3, 0, 1, 4, 1]
    return case([line(16, (0, 3, 1), (8, 11, 2)), line(16, (1, 4, 7), (9, 13, 3))], 0.5, 5, claim)


# ---- 64-bit products ----------------------------------------------------------------------------------------------------
P64 = dict(T=113258, a=42852, e5=23156, e9=28859)


def products_need_64_bits():
    """One track [0,T); id 5 takes [0,a) and e5 pixels outside, id 9 takes [a,T) and e9 pixels outside.  id 9 has the larger
    IoU, (T-a) * (T+e5) > a * (T+e9), but the same two products taken mod 2^32 compare the other way.  (T-a) * 65536 does
    not fit 32 bits either, so a threshold test in 32 bits loses id 9 as a candidate.  The row is padded to a multiple of 4."""
    T, a, e5, e9 = (P64[k] for k in ("T", "a", "e5", "e9"))
    big, small = (T - a) * (T + e5), a * (T + e9)
    assert big > small and big % 2 ** 32 < small % 2 ** 32 and (T - a) * 65536 >= 2 ** 32
    n = -(-(T + e5 + e9) // 4) * 4
    f1 = line(n, (0, a, 5), (a, T, 9), (T, T + e5, 5), (T + e5, T + e5 + e9, 9))

    def claim(run):
        _, lut, table, _, meta = run[1]
        assert lut[9] == 1 and lut[5] == 2 and meta == dict(next_uid=3, step=2, dropped=0)
        assert table[1].tolist() == [1, 0, 2, T - a + e9, 0] and table[2].tolist() == [2, 0, 1, a + e5, 1]
    return case([line(n, (0, T, 1)), f1], 0.3, 5, claim)


# ---- births ------------------------------------------------------------------------------------------------------------
GONE = (5, 63, 64, 100, 126, 127)      # two below lane 64 of the ballot, four from it up
NEW = (3, 62, 63, 64, 65, 126)          # three and three: the two wave-1 offsets differ


def full_house():
    return line(DOMINO_W, *[(2 * k, 2 * k + 2, k + 1) for k in range(127)])     # id k+1 -> slot k+1, 2 px each


def renumbered(gone, taken):
    """The objects of full_house() whose slot is not in `gone`, in place, under the raw ids that are not in `taken`."""
    ids = [c for c in range(127, 0, -1) if c not in taken]                      # descending: no object keeps its id
    slots = [s for s in range(1, 128) if s not in gone]
    assert len(slots) <= len(ids)
    return [(2 * (s - 1), 2 * s, c) for s, c in zip(slots, ids)]


def births_across_waves():
    """127 live tracks, max_age 0.  The next frame drops the objects of slots 5, 63, 64, 100, 126, 127, which retire in this
    step, and shows the new ids 3, 62, 63, 64, 65, 126 beyond pixel 256 where nothing was.  The new ids in ascending order take
    the free slots in ascending order, uids 128..133: ids and slots on both sides of lane 64 of the ballots."""
    new_at = {3: 300, 62: 330, 63: 260, 64: 500, 65: 270, 126: 400}
    f1 = line(DOMINO_W, *renumbered(GONE, NEW), *[(p, p + 3, c) for c, p in new_at.items()])

    def claim(run):
        _, lut, table, _, meta = run[1]
        for rank, (c, s) in enumerate(zip(NEW, GONE)):
            assert lut[c] == s and table[s].tolist() == [128 + rank, 0, 1, 3, 1]
        assert meta == dict(next_uid=134, step=2, dropped=0) and len(live(table)) == 127
        assert all(table[s].tolist() == [s, 0, 2, 2, 0] for s in range(1, 128) if s not in GONE)
    return case([full_house(), f1], 0.3, 0, claim)


GONE_FIRST = (5, 20, 63, 64, 65, 100, 120, 127)
GONE_LATER = (2, 66, 90, 126)
LATE_NEW = (1, 2, 40, 62, 63, 64, 65, 66, 100, 125, 126, 127)


def births_overflow():
    """More new ids than free slots.  With 127 live tracks this needs max_age >= 1: at most 127 ids are present, so the
    new ones are no more than the tracks left unmatched, and at max_age 0 every one of those is free in the same step.
    max_age 1.  Step 1: eight objects vanish (age 1, not free) and three new ids find no slot: dropped 3.  Step 2: the
    eight retire and are free, four more objects vanish, twelve new ids appear: the lowest eight take the eight slots in
    ascending order with uids 128..135, the highest four are dropped: dropped 7."""
    f1 = line(DOMINO_W, *renumbered(GONE_FIRST, (7, 64, 99)), (300, 303, 99), (310, 313, 7), (320, 323, 64))
    gone = GONE_FIRST + GONE_LATER
    at = [260 + 5 * (7 * i % 12) for i in range(12)]                              # scattered, disjoint
    f2 = line(DOMINO_W, *renumbered(gone, LATE_NEW), *[(p, p + 3, c) for p, c in zip(at, LATE_NEW)])

    def claim(run):
        assert run[1][4] == dict(next_uid=128, step=2, dropped=3) and not run[1][1][[7, 64, 99]].any()
        assert not run[1][0][0, 256:].any()
        out, lut, table, _, meta = run[2]
        for rank, (c, s) in enumerate(zip(LATE_NEW[:8], GONE_FIRST)):
            assert lut[c] == s and table[s].tolist() == [128 + rank, 0, 1, 3, 2]
        assert not lut[list(LATE_NEW[8:])].any() and meta == dict(next_uid=136, step=3, dropped=7)
        assert all(table[s].tolist() == [s, 1, 2, 2, 0] for s in GONE_LATER)
    return case([full_house(), f1, f2], 0.3, 1, claim)


# ---- tiny maps and junk values -----------------------------------------------------------------------------------------------
def tiny(H, W, max_age, a=9, b=4):
    """An object, nothing, the object again under another id, nothing: fewer than 64 pixels, one wave mostly idle."""
    obj = np.zeros((H, W), dtype=np.int32)
    obj.reshape(-1)[:max(1, H * W - 1)] = a
    again = np.where(obj > 0, b, 0).astype(np.int32)

    def claim(run):
        n = int((obj > 0).sum())
        assert run[0][2][1].tolist() == [1, 0, 1, n, 0] and np.array_equal(run[0][0], (obj > 0))
        if max_age:       # kept through the gap, recovered
            assert run[1][2][1].tolist() == [1, 1, 1, n, 0] and np.array_equal(run[1][3], (obj > 0))
            assert run[2][2][1].tolist() == [1, 0, 2, n, 0] and run[3][4] == dict(next_uid=2, step=4, dropped=0)
        else:             # retired in the gap, reborn into the same slot as uid 2
            assert not run[1][2].any() and not run[1][3].any()
            assert run[2][2][1].tolist() == [2, 0, 1, n, 2] and run[3][4] == dict(next_uid=3, step=4, dropped=0)
        assert np.array_equal(run[2][0], (obj > 0)) and not run[3][0].any()
    return case([obj, np.zeros_like(obj), again, np.zeros_like(obj)], 0.3, max_age, claim)


def tiny_1x1():
    return tiny(1, 1, 1)


def tiny_1x3():
    return tiny(1, 3, 0)


def tiny_3x1():
    return tiny(3, 1, 1, a=127, b=64)


def junk_and_edges():
    """Ids 1 and 127 next to the values that must read as background, which then move over the tracks' pixels."""
    J = [-1, 0, 128, 255, INT_MIN, 1 << 20]
    f0 = np.array([[J[0], 1, J[1], J[2], 127, J[3], J[4], 127, J[5], 1, -128, 129]], dtype=np.int64).astype(np.int32)
    f1 = np.array([[1, J[2], J[4], 127, J[5], J[0], 127, J[3], 1, J[1], 256, -127]], dtype=np.int64).astype(np.int32)
    f2 = np.array([[J[4], J[5], J[2], J[3], J[0], 128, 1 << 20, -1, 255, 0, 127, 1]], dtype=np.int64).astype(np.int32)

    def claim(run):
        assert run[0][0].tolist() == [[0, 1, 0, 0, 2, 0, 0, 2, 0, 1, 0, 0]] and run[0][4]["next_uid"] == 3
        # nothing overlaps: both tracks age, ids 1 and 127 are born as 3 and 4, the old footprints stay in the memory map
        assert run[1][0].tolist() == [[3, 0, 0, 4, 0, 0, 4, 0, 3, 0, 0, 0]]
        assert run[1][3].tolist() == [[3, 1, 0, 4, 2, 0, 4, 2, 3, 1, 0, 0]]
        assert run[2][0].tolist() == [[0] * 10 + [6, 5]] and run[2][4] == dict(next_uid=7, step=3, dropped=0)
    return case([f0, f1, f2], 0.3, 5, claim)


MOVED = ("tie_larger_inter", "tie_lower_track", "tie_lower_id", "threshold_equal_large", "threshold_equal_large_miss",
         "threshold_half_line", "threshold_below_half", "overflow_128th")
ENGINEERED = ("tie_domino", "tie_larger_inter_many", "tie_lower_id_high", "threshold_equal_small", "threshold_equal_half",
              "products_need_64_bits", "births_across_waves", "births_overflow", "tiny_1x1", "tiny_1x3", "tiny_3x1",
              "junk_and_edges")
CASES = {name: globals()[name] for name in MOVED + ENGINEERED}


# ---- mutants of the rules --------------------------------------------------------------------------------------------------
M32 = 2 ** 32


class MutantTracker(ReferenceTracker):
    """ReferenceTracker with one rule broken.  Only tests use it: a case that no mutant can tell from the true rule is not
    doing its job."""

    def __init__(self, min_iou=0.3, max_age=5, rule=None):
        assert rule in MUTANTS
        self.rule = rule
        super().__init__(min_iou, max_age)

    def passes(self, inter, union):
        if self.rule == "exclusive_threshold":
            return inter * 65536 > self.q * union
        if self.rule == "threshold_product_mod_2_32":
            return (inter * 65536) % M32 >= (self.q * union) % M32
        return super().passes(inter, union)

    def prefers(self, a, b):
        (inter, union, t, c), (bi, bu, bt, bc) = a, b
        lhs, rhs = inter * bu, bi * union
        if self.rule == "comparison_products_mod_2_32":
            lhs, rhs = lhs % M32, rhs % M32
        if lhs != rhs:
            return lhs > rhs
        if self.rule != "tie_ignores_intersection" and inter != bi:
            return inter > bi
        if self.rule == "tie_to_higher_track":
            return (-t, c) < (-bt, bc)
        if self.rule == "tie_to_higher_id":
            return (t, -c) < (bt, -bc)
        return (t, c) < (bt, bc)

    def free_slots(self, retired):
        free = super().free_slots(retired)
        if self.rule == "births_into_descending_slots":
            return free[::-1]
        if self.rule == "retired_slot_free_next_step":
            return [s for s in free if s not in retired]
        return free


# mutant -> the cases named for it: each of them must come out differently under the mutant
MUTANTS = {
    "exclusive_threshold": ("threshold_equal_small", "threshold_equal_half", "threshold_equal_large"),
    "tie_ignores_intersection": ("tie_larger_inter", "tie_larger_inter_many"),
    "tie_to_higher_track": ("tie_lower_track", "tie_domino"),
    "tie_to_higher_id": ("tie_lower_id", "tie_lower_id_high"),
    "comparison_products_mod_2_32": ("products_need_64_bits",),
    "threshold_product_mod_2_32": ("products_need_64_bits",),
    "births_into_descending_slots": ("births_across_waves", "births_overflow"),
    "retired_slot_free_next_step": ("births_across_waves", "births_overflow", "overflow_128th"),
}
