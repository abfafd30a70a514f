"""The tracker's contract (include/uoc_hip.h) restated in plain Python integers and numpy: what
uoc_track_step must compute, bit for bit.  No torch, no GPU.  Test infrastructure."""
import numpy as np

NUM = 128
FIELDS = ("uid", "age", "hits", "area", "born")


def iou_threshold(min_iou):
    return max(1, int(round(float(min_iou) * 65536)))


def object_ids(labels):
    """Raw label map -> ids 1..127, everything else (negatives, 128 and above, non-finite) background."""
    lab = np.asarray(labels)
    if lab.dtype.kind == "f":
        lab = np.where(np.isfinite(lab), lab, 0)
    lab = lab.astype(np.int64)
    return np.where((lab >= 1) & (lab < NUM), lab, 0)


class ReferenceTracker:
    """One stream.  table[s] = [uid, age, hits, area, born]; events counts what happened, for the tests' coverage
    checks: match, birth (after step 0), retire, recover (a match of a track with age > 0), reuse (a birth into a slot
    that held another track before)."""

    def __init__(self, min_iou=0.3, max_age=5):
        self.q = iou_threshold(min_iou)
        self.max_age = int(max_age)
        self.reset()

    def reset(self):
        self.mem = None
        self.table = np.zeros((NUM, 5), dtype=np.int64)
        self.next_uid, self.step_index, self.dropped = 1, 0, 0
        self.used = np.zeros(NUM, dtype=bool)
        self.events = dict(match=0, birth=0, retire=0, recover=0, reuse=0)

    # The decision rules, one method each, so that tests/tracking_cases.py can break one at a time (its mutants).
    def passes(self, inter, union):
        """The candidate test: inclusive, exact."""
        return inter * 65536 >= self.q * union

    def prefers(self, a, b):
        """Candidate a = (inter, union, t, c) goes before b: larger IoU, larger inter, lower t, lower c."""
        (inter, union, t, c), (bi, bu, bt, bc) = a, b
        lhs, rhs = inter * bu, bi * union               # Python ints: exact
        return lhs > rhs or (lhs == rhs and (inter > bi or (inter == bi and (t, c) < (bt, bc))))

    def free_slots(self, retired):
        """The free slots in the order births take them; `retired` = the slots retired in this very step."""
        return [s for s in range(1, NUM) if self.table[s, 0] == 0]

    def step(self, labels):
        cur = object_ids(labels)
        if self.mem is None or self.mem.shape != cur.shape:
            self.mem = np.zeros(cur.shape, dtype=np.int64)
        mem, table = self.mem, self.table
        assert cur.size < 2 ** 31
        # 1. contingency
        cont = np.bincount((mem * NUM + cur).reshape(-1), minlength=NUM * NUM).reshape(NUM, NUM)
        area_mem, area_cur = cont.sum(1), cont.sum(0)
        live_before = table[:, 0] != 0
        # 2. candidates
        cands = []
        for t, c in zip(*np.nonzero(cont)):
            t, c = int(t), int(c)
            if t < 1 or c < 1 or not live_before[t]:
                continue
            inter = int(cont[t, c])
            union = int(area_mem[t]) + int(area_cur[c]) - inter
            if self.passes(inter, union):
                cands.append((inter, union, t, c))
        # 3. greedy matching on exact rationals
        match_t, match_c = {}, {}
        while True:
            best = None
            for cand in cands:
                inter, union, t, c = cand
                if t in match_t or c in match_c:
                    continue
                if best is None or self.prefers(cand, best):
                    best = cand
            if best is None:
                break
            match_t[best[2]] = best[3]
            match_c[best[3]] = best[2]
        # 4. ageing
        lut = np.zeros(NUM, dtype=np.int64)
        keep = np.zeros(NUM, dtype=bool)
        retired = set()
        for t in range(1, NUM):
            if not live_before[t]:
                continue
            if t in match_t:
                c = match_t[t]
                self.events["match"] += 1
                if table[t, 1] > 0:
                    self.events["recover"] += 1
                table[t, 1] = 0
                table[t, 2] += 1
                table[t, 3] = area_cur[c]
                lut[c] = t
            else:
                table[t, 1] += 1
                if table[t, 1] > self.max_age:
                    table[t] = 0
                    retired.add(t)
                    self.events["retire"] += 1
                else:
                    keep[t] = True
        # 5. births
        for c in range(1, NUM):
            if area_cur[c] == 0 or c in match_c:
                continue
            free = self.free_slots(retired)
            if not free:
                self.dropped += 1
                continue
            s = free[0]
            table[s] = (self.next_uid, 0, 1, area_cur[c], self.step_index)
            self.next_uid += 1
            lut[c] = s
            if self.step_index > 0:
                self.events["birth"] += 1
            if self.used[s]:
                self.events["reuse"] += 1
            self.used[s] = True
        # 6. output, 7. memory
        out = lut[cur]
        self.mem = np.where(out != 0, out, np.where(keep[mem], mem, 0))
        self.step_index += 1
        self.lut = lut
        return out.astype(np.int32)

    # what the device state must hold
    def table32(self):
        return self.table.astype(np.int32)

    def mem32(self):
        return self.mem.astype(np.int32)

    def meta(self):
        return dict(next_uid=self.next_uid, step=self.step_index, dropped=self.dropped)
