"""Named cases for the re-identification stages (include/uoc_hip.h), each with a `claim` that writes the
answer down by hand.  The step cases are authored at the table level — a hand-made identity state, track tables and
signatures — so that one rule alone decides each of them; `mutants` names the broken rules (MUTANTS below) that must
come out differently on the case.  The signature cases are tiny images.  The sequences are generated scenes for the
end-to-end tests.  No torch, no GPU.  Test infrastructure."""
import numpy as np

from tests import identity_reference as ir

NUM, WORDS = ir.NUM, ir.WORDS


# ---- building blocks ------------------------------------------------------------------------------------------------------
def sig_row(pixels, bins=None, area=0):
    """A hand-made signature: `bins` = {word: value} among the histogram words 8..98."""
    row = np.zeros(WORDS, dtype=np.int64)
    row[0], row[1], row[2], row[3] = pixels, (pixels if area else 0), area & 0xFFFFFFFF, area >> 32
    for k, v in (bins or {}).items():
        assert ir.HIST <= k < ir.HIST_END
        row[k] = v
    return row


def sig_table(rows):
    """{slot: row} -> [128,104] int32."""
    t = np.zeros((NUM, WORDS), dtype=np.int64)
    for s, row in rows.items():
        t[s] = row
    return ir.as_int32(t)


def track_table(visible=None, occluded=None):
    """{slot: uid} of the slots matched in this frame (age 0) and of the occluded ones (age 1) -> [128,5] int32."""
    t = np.zeros((NUM, 5), dtype=np.int32)
    for s, uid in (visible or {}).items():
        t[s] = (uid, 0, 1, 10, 0)
    for s, uid in (occluded or {}).items():
        t[s] = (uid, 1, 1, 10, 0)
    return t


def entry(pid, uid, seen, row, hits=1):
    return dict(pid=pid, uid=uid, seen=seen, hits=hits, sig=row)


class StepCase:
    def __init__(self, name, claim, steps, entries=None, counters=(0, 0, 0), q=45875, r=0, max_lost=300, mutants=()):
        self.name, self.claim, self.steps, self.entries, self.counters = name, claim, steps, entries or {}, counters
        self.q, self.r, self.max_lost, self.mutants = q, r, max_lost, tuple(mutants)

    def initial_words(self):
        """The state words the case starts from, as the device keeps them."""
        ref = ir.ReferenceIdentifier(q=self.q, r=self.r, max_lost=self.max_lost)
        self.load(ref)
        return ref.state_words()

    def load(self, ident):
        ident.pids, ident.step_index, ident.evicted = self.counters
        for e, rec in self.entries.items():
            ident.table[e] = (rec["pid"], rec["uid"], rec["seen"], rec["hits"], rec["sig"][0])
            ident.sigs[e] = rec["sig"]

    def run(self, cls=ir.ReferenceIdentifier):
        """Per step: dict(lut, table, words) of a fresh identifier of class `cls` started from the case's state."""
        ident = cls(q=self.q, r=self.r, max_lost=self.max_lost)
        self.load(ident)
        out = []
        for tracks, sig in self.steps:
            lut = ident.step(tracks, sig)
            out.append(dict(lut=lut.copy(), table=ident.table32().copy(), words=ident.state_words().copy(),
                            pids=ident.pids, step=ident.step_index, evicted=ident.evicted))
        return out


# ---- the mutants: one broken rule each ------------------------------------------------------------------------------------
class ExclusiveThreshold(ir.ReferenceIdentifier):
    def passes(self, sim):
        return sim > self.q


class TieSeenReversed(ir.ReferenceIdentifier):
    def order_key(self, sim, seen, e, s):
        return (sim, -seen, -e, -s)


class TieEntryReversed(ir.ReferenceIdentifier):
    def order_key(self, sim, seen, e, s):
        return (sim, seen, e, -s)


class TieSlotReversed(ir.ReferenceIdentifier):
    def order_key(self, sim, seen, e, s):
        return (sim, seen, -e, s)


class Area32(ir.ReferenceIdentifier):
    def areas_agree(self, a_new, a_old):
        return super().areas_agree(a_new & 0xFFFFFFFF, a_old & 0xFFFFFFFF)


class ForgetLate(ir.ReferenceIdentifier):
    def forgotten(self, seen):
        return self.step_index - seen > self.max_lost + 1


class FreedNextStep(ir.ReferenceIdentifier):
    def free_entries(self, freed_now):
        return [e for e in super().free_entries(freed_now) if e not in freed_now]


class EvictNewest(ir.ReferenceIdentifier):
    def eviction_key(self, e):
        return (-int(self.table[e, 2]), e)


MUTANTS = {"exclusive_threshold": ExclusiveThreshold, "tie_seen_reversed": TieSeenReversed, "tie_entry_reversed": TieEntryReversed,
           "tie_slot_reversed": TieSlotReversed, "area_32bit": Area32, "forget_late": ForgetLate, "freed_next_step": FreedNextStep,
           "evict_newest": EvictNewest}
SIGNATURE_MUTANTS = ("chroma_without_zero_skip",)       # ir.chroma_votes(skip_zero=False): the pure-blue case


# ---- step cases -------------------------------------------------------------------------------------------------------------
Q = 40000
RED, BLUE, GREEN = {8: 50000}, {30: 50000}, {60: 50000}        # three "colours" that share no bin: sim 0 to each other


def _threshold():
    steps = [(track_table({1: 1, 2: 2}), sig_table({1: sig_row(9, {8: 40000}), 2: sig_row(9, {9: 50000})})),
             (track_table(), sig_table({})),
             (track_table({3: 3, 4: 4}), sig_table({3: sig_row(9, {8: 41000, 20: 100}), 4: sig_row(9, {9: 39999})}))]

    def claim(res):
        assert res[0]["lut"][1] == 1 and res[0]["lut"][2] == 2 and res[0]["pids"] == 2
        assert not res[1]["lut"].any() and res[1]["pids"] == 2
        assert res[2]["lut"][3] == 1              # sim = min(41000, 40000) = 40000 == q: inclusive
        assert res[2]["lut"][4] == 3              # sim = 39999: one less, a new identity in the first free entry
        assert res[2]["pids"] == 3 and res[2]["table"][1].tolist() == [1, 3, 3, 2, 9] and res[2]["table"][3].tolist() == [3, 4, 3, 1, 9]
        assert res[2]["table"][2].tolist() == [2, 2, 1, 1, 9]          # the lost entry stays as it was
    return StepCase("threshold_inclusive", claim, steps, q=Q, mutants=["exclusive_threshold"])


def _tie_seen():
    entries = {3: entry(1, 11, 5, sig_row(9, RED)), 100: entry(2, 12, 7, sig_row(9, RED))}
    steps = [(track_table({2: 50}), sig_table({2: sig_row(9, RED)}))]

    def claim(res):
        assert res[0]["lut"][2] == 100            # equal sim: the entry seen later
        assert res[0]["table"][100].tolist() == [2, 50, 11, 2, 9] and res[0]["table"][3].tolist() == [1, 11, 5, 1, 9]
        assert res[0]["pids"] == 2
    return StepCase("tie_by_seen", claim, steps, entries, counters=(2, 10, 0), q=Q, mutants=["tie_seen_reversed"])


def _tie_entry():
    entries = {30: entry(1, 11, 7, sig_row(9, RED)), 90: entry(2, 12, 7, sig_row(9, RED))}
    steps = [(track_table({2: 50}), sig_table({2: sig_row(9, RED)}))]

    def claim(res):
        assert res[0]["lut"][2] == 30 and res[0]["table"][30, 1] == 50 and res[0]["table"][90, 1] == 12
    return StepCase("tie_by_entry", claim, steps, entries, counters=(2, 10, 0), q=Q, mutants=["tie_entry_reversed"])


def _tie_slot():
    entries = {65: entry(1, 11, 7, sig_row(9, RED))}
    steps = [(track_table({10: 50, 80: 51}), sig_table({10: sig_row(9, RED), 80: sig_row(9, RED)}))]

    def claim(res):
        assert res[0]["lut"][10] == 65 and res[0]["lut"][80] == 1      # the lower slot wins, the other is a new identity
        assert res[0]["table"][1].tolist() == [2, 51, 11, 1, 9] and res[0]["pids"] == 2
    return StepCase("tie_by_slot", claim, steps, entries, counters=(1, 10, 0), q=Q, mutants=["tie_slot_reversed"])


def _domino():
    entries = {e: entry(e, 1000 + e, 7, sig_row(9, RED)) for e in range(1, 127)}
    steps = [(track_table({s: s for s in range(1, 128)}), sig_table({s: sig_row(9, RED) for s in range(1, 128)}))]

    def claim(res):
        assert res[0]["lut"][1:].tolist() == list(range(1, 128))       # round k takes (entry k, slot k); slot 127 is left over
        assert res[0]["table"][127].tolist() == [127, 127, 11, 1, 9] and res[0]["pids"] == 127 and res[0]["evicted"] == 0
        assert res[0]["table"][1:127, 0].tolist() == list(range(1, 127))
    return StepCase("domino_127_against_126", claim, steps, entries, counters=(126, 10, 0), q=Q,
                    mutants=["tie_entry_reversed", "tie_slot_reversed"])


def _size_gate_equality():
    entries = {5: entry(1, 11, 7, sig_row(9, RED, area=1024)), 6: entry(2, 12, 7, sig_row(9, BLUE, area=1024))}
    steps = [(track_table({1: 50, 2: 51}), sig_table({1: sig_row(9, RED, area=256), 2: sig_row(9, BLUE, area=255)}))]

    def claim(res):
        assert res[0]["lut"][1] == 5              # 256 * 256 == 64 * 1024: equality passes
        assert res[0]["lut"][2] == 1              # 255 * 256 < 64 * 1024: refused, a new identity
    return StepCase("size_gate_equality", claim, steps, entries, counters=(2, 10, 0), q=Q, r=64)


def _size_gate_zero_area(r):
    entries = {5: entry(1, 11, 7, sig_row(9, RED, area=1024)), 6: entry(2, 12, 7, sig_row(9, BLUE, area=0))}
    steps = [(track_table({1: 50, 2: 51}), sig_table({1: sig_row(9, RED, area=0), 2: sig_row(9, BLUE, area=500)}))]

    def claim(res):
        if r > 0:                                 # an area of 0 on either side never passes the gate
            assert res[0]["lut"][1] == 1 and res[0]["lut"][2] == 2 and res[0]["pids"] == 4
        else:                                     # r == 0: there is no gate
            assert res[0]["lut"][1] == 5 and res[0]["lut"][2] == 6 and res[0]["pids"] == 2
    return StepCase(f"size_gate_zero_area_r{r}", claim, steps, entries, counters=(2, 10, 0), q=Q, r=r)


def _size_gate_64bit():
    big, small = (1 << 32) + 10, (1 << 32) - 100       # big > small, but big's low word 10 < small's low word
    entries = {5: entry(1, 11, 7, sig_row(9, RED, area=small))}
    steps = [(track_table({1: 50}), sig_table({1: sig_row(9, RED, area=big)}))]

    def claim(res):
        assert res[0]["lut"][1] == 5              # the two areas are nearly equal
        assert res[0]["words"][1024 + 5 * WORDS + 2] == 10 and res[0]["words"][1024 + 5 * WORDS + 3] == 1
    return StepCase("size_gate_needs_64_bits", claim, steps, entries, counters=(1, 10, 0), q=Q, r=128, mutants=["area_32bit"])


def _forget_boundary():
    # all 127 entries taken: 1..125 bound to their slots, 126 lost for exactly max_lost steps, 127 for one more
    entries = {e: entry(e, e, 10, sig_row(9, GREEN)) for e in range(1, 126)}
    entries[126] = entry(126, 900, 6, sig_row(9, BLUE))
    entries[127] = entry(127, 901, 5, sig_row(9, RED))
    vis = {s: s for s in range(1, 126)}
    vis[126] = 500
    sigs = {s: sig_row(9, GREEN) for s in range(1, 126)}
    sigs[126] = sig_row(9, RED)
    steps = [(track_table(vis), sig_table(sigs))]

    def claim(res):
        assert res[0]["step"] == 11
        assert res[0]["table"][126].tolist() == [126, 900, 6, 1, 9]    # 11 - 6 == max_lost: kept
        assert res[0]["lut"][126] == 127                               # 11 - 5 > max_lost: forgotten, and its entry taken at once
        assert res[0]["table"][127].tolist() == [128, 500, 11, 1, 9] and res[0]["pids"] == 128 and res[0]["evicted"] == 0
    return StepCase("forget_boundary_and_reuse", claim, steps, entries, counters=(127, 10, 0), q=Q, max_lost=5,
                    mutants=["forget_late", "freed_next_step"])


def _eviction():
    entries = {e: entry(e, e, 10, sig_row(9, GREEN)) for e in range(1, 125)}
    entries[125] = entry(125, 900, 3, sig_row(9, BLUE))
    entries[126] = entry(126, 901, 3, sig_row(9, BLUE))
    entries[127] = entry(127, 902, 9, sig_row(9, BLUE))
    vis = {s: s for s in range(1, 125)}
    vis[125] = 500
    sigs = {s: sig_row(9, GREEN) for s in range(1, 125)}
    sigs[125] = sig_row(7, RED)
    steps = [(track_table(vis), sig_table(sigs))]

    def claim(res):
        assert res[0]["lut"][125] == 125 and res[0]["evicted"] == 1    # the oldest sighting goes; of two equally old, the lower entry
        assert res[0]["table"][125].tolist() == [128, 500, 11, 1, 7]
        assert res[0]["table"][126].tolist() == [126, 901, 3, 1, 9] and res[0]["table"][127].tolist() == [127, 902, 9, 1, 9]
    return StepCase("eviction_when_full", claim, steps, entries, counters=(127, 10, 0), q=Q, mutants=["evict_newest"])


def _orphaned_uid():
    steps = [(track_table({1: 10}), sig_table({1: sig_row(9, RED)})),
             (track_table({2: 11}, occluded={1: 10}), sig_table({1: sig_row(9, RED), 2: sig_row(9, RED)})),
             (track_table({1: 10, 2: 11}), sig_table({1: sig_row(9, RED), 2: sig_row(9, RED)}))]

    def claim(res):
        assert res[0]["lut"][1] == 1
        assert res[1]["lut"][2] == 1 and res[1]["lut"][1] == 0 and res[1]["table"][1, 1] == 11      # the entry was taken over
        assert res[2]["lut"][2] == 1 and res[2]["lut"][1] == 2 and res[2]["pids"] == 2              # uid 10 comes back as a newcomer
    return StepCase("orphaned_uid_returns", claim, steps, q=Q)


def _never_visible():
    entries = {4: entry(1, 11, 9, sig_row(9, RED))}
    tracks = track_table({1: 20, 3: 22}, occluded={2: 21})
    tracks[5] = (0, 0, 0, 0, 0)
    sigs = sig_table({1: sig_row(0, RED), 2: sig_row(9, RED), 5: sig_row(9, RED), 70: sig_row(9, RED)})       # slot 3 has no row at all
    steps = [(tracks, sigs)]

    def claim(res):
        assert not res[0]["lut"].any() and res[0]["pids"] == 1 and res[0]["step"] == 11
        assert res[0]["table"][4].tolist() == [1, 11, 9, 1, 9] and np.count_nonzero(res[0]["table"][:, 0]) == 1
    return StepCase("never_visible", claim, steps, entries, counters=(1, 10, 0), q=Q)


STEP_CASES = [_threshold(), _tie_seen(), _tie_entry(), _tie_slot(), _domino(), _size_gate_equality(), _size_gate_zero_area(64),
              _size_gate_zero_area(0), _size_gate_64bit(), _forget_boundary(), _eviction(), _orphaned_uid(), _never_visible()]


# ---- signature cases ----------------------------------------------------------------------------------------------------------
class SignatureCase:
    def __init__(self, name, claim, labels, image, xyz=None):
        self.name, self.claim = name, claim
        self.labels = np.asarray(labels, dtype=np.int32)
        self.image = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
        self.xyz = None if xyz is None else np.ascontiguousarray(np.asarray(xyz, dtype=np.float32))


def _flat(labels, colour):
    lab = np.asarray(labels, dtype=np.int32)
    return lab, np.broadcast_to(np.asarray(colour, dtype=np.uint8), lab.shape + (3,)).copy()


def _sig_ids():
    lab, img = _flat([[0, 1, 127, 128, -1, 1]], (90, 90, 90))

    def claim(sig):
        assert sig[1, 0] == 2 and sig[127, 0] == 1 and np.count_nonzero(sig[:, 0]) == 2 and not sig[0].any()
    return SignatureCase("ids_0_1_127_128_minus1", claim, lab, img)


def _sig_dark():
    lab = np.array([[1, 2]], dtype=np.int32)
    img = np.array([[[16, 16, 15], [16, 16, 16]]], dtype=np.uint8)

    def claim(sig):
        assert sig[1, ir.DARK] == 49152 and not sig[1, ir.HIST:ir.DARK].any()          # s = 47: dark, 64 * 768 / 1
        assert sig[2, ir.DARK] == 0 and sig[2, ir.HIST:ir.DARK].sum() == 49152          # s = 48: chroma
        # u = v = 21: ul = vl = 2, uf = vf = 5: weights 9, 15, 15, 25 on bins (2,2), (2,3), (3,2), (3,3)
        assert [sig[2, 8 + 2 * 9 + 2], sig[2, 8 + 2 * 9 + 3], sig[2, 8 + 3 * 9 + 2], sig[2, 8 + 3 * 9 + 3]] == [9 * 768, 15 * 768, 15 * 768, 25 * 768]
        assert sig[1, ir.INTENSITY] == (64 - 24) * 256 and sig[1, ir.INTENSITY + 1] == 24 * 256       # y = 15: yf = 3
    return SignatureCase("s_47_against_48", claim, lab, img)


def _sig_blue():
    lab, img = _flat([[1]], (255, 0, 0))

    def claim(sig):
        assert sig[1, 8 + 8 * 9 + 0] == 49152 and sig[1, ir.HIST:ir.INTENSITY].sum() == 49152       # u = 64: ul = 8, uf = 0
        assert sig[1, ir.INTENSITY + 2] == 24 * 256 and sig[1, ir.INTENSITY + 3] == 40 * 256            # y = 85: yl = 2, yf = 5
    return SignatureCase("pure_blue", claim, lab, img)


def _sig_white():
    lab, img = _flat([[1]], (255, 255, 255))

    def claim(sig):
        assert sig[1, ir.INTENSITY + 7] == 8 * 256 and sig[1, ir.INTENSITY + 8] == 56 * 256             # y = 255: yl = 7, yf = 7
        assert sig[1, ir.INTENSITY:ir.HIST_END].sum() == 16384
    return SignatureCase("y_255", claim, lab, img)


def _sig_floors():
    lab = np.array([[1, 1, 1]], dtype=np.int32)
    img = np.array([[[200, 30, 30], [30, 200, 60], [10, 30, 200]]], dtype=np.uint8)

    def claim(sig):
        # y = 86, 96, 80: intensity votes 24 + 32 = 56 on bin 2 and 40 + 64 + 32 = 136 on bin 3; 768 / 3 is whole, 256 / 3 is not
        assert sig[1, ir.INTENSITY + 2] == (56 * 256) // 3 == 4778 and sig[1, ir.INTENSITY + 3] == (136 * 256) // 3 == 11605
        total = int(sig[1, ir.HIST:ir.HIST_END].sum())
        assert total == 65535 and 65536 - 91 <= total and sig[1, 0] == 3
    return SignatureCase("n_3_floors", claim, lab, img)


def _sig_depth():
    lab, img = _flat([[1, 1, 1, 1, 1, 2]], (90, 120, 150))
    z = np.array([[0.0, np.nan, -1.0, 65.0, np.float32(65.001), 0.5]], dtype=np.float32)
    xyz = np.stack([np.zeros_like(z), np.zeros_like(z), z])

    def claim(sig):
        assert sig[1, 0] == 5 and sig[1, 1] == 1                       # only z = 65 counts
        assert sig[1, 2] == (65000 * 65000) >> 10 and sig[1, 3] == 0
        assert sig[2, 1] == 1 and sig[2, 2] == (500 * 500) >> 10
    return SignatureCase("depth_edges", claim, lab, img, xyz)


def _sig_one_pixel():
    lab = np.zeros((5, 13), dtype=np.int32)
    lab[2, 7] = 9
    img = np.full((5, 13, 3), 60, dtype=np.uint8)
    img[2, 7] = (10, 200, 90)

    def claim(sig):
        assert sig[9, 0] == 1 and np.count_nonzero(sig[:, 0]) == 1 and sig[9, ir.HIST:ir.HIST_END].sum() == 65536
    return SignatureCase("one_pixel_object", claim, lab, img)


def _sig_high_word():
    lab, img = _flat(np.full((40, 50), 3), (90, 120, 150))
    xyz = np.zeros((3, 40, 50), dtype=np.float32)
    xyz[2] = 65.0

    def claim(sig):
        area = 2000 * ((65000 * 65000) >> 10)
        assert area >> 32 == 1 and ir.area_of(sig[3]) == area and sig[3, 3] == 1 and sig[3, 1] == 2000
    return SignatureCase("area_needs_the_high_word", claim, lab, img, xyz)


SIGNATURE_CASES = [_sig_ids(), _sig_dark(), _sig_blue(), _sig_white(), _sig_floors(), _sig_depth(), _sig_one_pixel(), _sig_high_word()]


# ---- generated sequences ------------------------------------------------------------------------------------------------------
def render(H, W, objs, rng, z_table=1.0):
    """objs: [(raw id, y0, x0, h, w, (b, g, r))], later ones cover earlier ones.  A grey table at z_table metres, the
    objects 5 cm nearer; +-6 of noise on every byte."""
    lab = np.zeros((H, W), dtype=np.int32)
    img = np.full((H, W, 3), 90, dtype=np.int64)
    z = np.full((H, W), z_table, dtype=np.float32)
    for rid, y0, x0, h, w, colour in objs:
        lab[y0:y0 + h, x0:x0 + w] = rid
        img[y0:y0 + h, x0:x0 + w] = colour
        z[y0:y0 + h, x0:x0 + w] = z_table - 0.05
    img = np.clip(img + rng.integers(-6, 7, size=img.shape), 0, 255).astype(np.uint8)
    xyz = np.stack([np.zeros_like(z), np.zeros_like(z), z]).astype(np.float32)
    return lab, img, xyz


class Sequence:
    """frames: [(labels, image, xyz)]; where[name][t] = a pixel (y, x) of the named object in frame t, or None."""

    def __init__(self, name, frames, where, tracker, ident):
        self.name, self.frames, self.where, self.tracker, self.ident = name, frames, where, tracker, ident


def tabletop_sequence():
    """A drifting object, one that jumps (IoU 0), one that is hidden until its track has retired, one that is replaced by
    another colour (refused by similarity) and one replaced by a much smaller object of its colour (refused by size)."""
    rng = np.random.default_rng(2611)
    H, W, T = 48, 64, 14
    frames, where = [], {k: [] for k in ("drift", "jump", "hidden", "recolour", "shrunk")}
    for t in range(T):
        objs, at = [], {}
        objs.append((0, 2, 2 + t, 10, 10, (40, 40, 200)))
        at["drift"] = (6, 6 + t)
        x = 4 if t < 5 else 40
        objs.append((0, 16, x, 10, 10, (200, 60, 40)))
        at["jump"] = (20, x + 4)
        if t < 3 or t >= 9:
            objs.append((0, 36, 4, 8, 8, (40, 200, 60)))
            at["hidden"] = (40, 8)
        if t < 4:
            objs.append((0, 36, 24, 8, 8, (40, 200, 200)))
            at["recolour"] = (40, 28)
        elif t >= 7:
            objs.append((0, 36, 24, 8, 8, (200, 40, 200)))
            at["recolour"] = (40, 28)
        if t < 6:
            objs.append((0, 30, 48, 12, 12, (200, 200, 40)))
            at["shrunk"] = (34, 52)
        elif t >= 10:
            objs.append((0, 30, 40, 4, 4, (200, 200, 40)))
            at["shrunk"] = (31, 41)
        ids = [1 + (k * 7 + t * 3) % 11 for k in range(len(objs))]          # the raw numbering changes every frame
        assert len(set(ids)) == len(ids)
        frames.append(render(H, W, [(i,) + o[1:] for i, o in zip(ids, objs)], rng))
        for k in where:
            where[k].append(at.get(k))
    return Sequence("tabletop", frames, where, tracker=dict(min_iou=0.3, max_age=2), ident=dict(min_sim=0.7, min_size=0.25, max_lost=300))


def forget_sequence():
    """One object stays, one is away for longer than max_lost and comes back as somebody new."""
    rng = np.random.default_rng(2612)
    H, W, T = 24, 40, 10
    frames, where = [], {"stays": [], "away": []}
    for t in range(T):
        objs, at = [(3, 2, 2, 8, 8, (40, 40, 200))], {"stays": (5, 5)}
        if t < 2 or t >= 8:
            objs.append((5, 12, 20, 8, 8, (200, 60, 40)))
            at["away"] = (15, 23)
        frames.append(render(H, W, objs, rng))
        for k in where:
            where[k].append(at.get(k))
    return Sequence("forget", frames, where, tracker=dict(min_iou=0.3, max_age=1), ident=dict(min_sim=0.7, min_size=0.25, max_lost=3))


def crowd_sequence():
    """Thirteen new objects of their own colours in every frame, at places that never overlap the frame before: 156
    identities for 127 entries."""
    rng = np.random.default_rng(2613)
    H, W, T = 32, 80, 12
    frames = []
    for t in range(T):
        objs = []
        for k in range(13):
            i = t * 13 + k
            colour = (30 + (i * 37) % 200, 30 + (i * 91) % 200, 30 + (i * 53) % 200)
            objs.append((1 + k, 4 + 16 * (t % 2), 2 + 6 * k, 5, 4, colour))
        frames.append(render(H, W, objs, rng))
    return Sequence("crowd", frames, {}, tracker=dict(min_iou=0.3, max_age=0), ident=dict(min_sim=0.9, min_size=0.25, max_lost=1000))


SEQUENCES = [tabletop_sequence, forget_sequence, crowd_sequence]


def run_reference(seq):
    """The sequence through tests/tracking_reference.py and then the identity reference.  Per frame: dict(tracked, tracks,
    sig, out, lut, words); and the identifier, for its events."""
    from tests import tracking_reference as tr
    tracker = tr.ReferenceTracker(**seq.tracker)
    ident = ir.ReferenceIdentifier(**seq.ident)
    frames = []
    for labels, image, xyz in seq.frames:
        tracked = tracker.step(labels)
        tracks = tracker.table32()
        sig = ir.describe(tracked, image, xyz)
        lut = ident.step(tracks, sig, live_uids=set(int(u) for u in tracks[:, 0] if u))
        frames.append(dict(tracked=tracked, tracks=tracks.copy(), sig=sig, out=ident.relabel(tracked), lut=lut.copy(),
                           words=ident.state_words().copy()))
    return frames, ident
