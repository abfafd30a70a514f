"""The re-identification cases (tests/identity_cases.py) without a GPU: every claim holds on the plain-integer reference
(tests/identity_reference.py); a reference with one rule broken comes out differently on every case named for that
rule, so each case really decides its rule; and the generated sequences contain what the GPU tests rely on — a
re-identification after a jump with IoU 0 and one after the track was retired, a refusal by similarity and one by size,
a forget and an eviction."""
import numpy as np
import pytest

from tests import identity_cases as IC
from tests import identity_reference as ir


@pytest.mark.parametrize("case", IC.STEP_CASES, ids=lambda c: c.name)
def test_step_claim_holds_on_the_reference(case):
    res = case.run()
    case.claim(res)
    for step in res:                              # the invariants of every state
        table = step["table"]
        pids = table[1:, 0][table[1:, 0] != 0]
        assert len(set(pids.tolist())) == pids.size and (pids <= step["pids"]).all() and not table[0].any()
        uids = table[1:, 1][table[1:, 0] != 0]
        assert len(set(uids.tolist())) == uids.size
        bound = step["lut"][step["lut"] != 0]
        assert len(set(bound.tolist())) == bound.size and (table[bound, 2] == step["step"]).all()


def test_every_mutant_has_a_case_and_fails_each_of_its_cases():
    named = {m for c in IC.STEP_CASES for m in c.mutants}
    assert named == set(IC.MUTANTS)
    for case in IC.STEP_CASES:
        good = case.run()
        for m in case.mutants:
            bad = case.run(IC.MUTANTS[m])
            assert any(not np.array_equal(a["words"], b["words"]) or not np.array_equal(a["lut"], b["lut"])
                       for a, b in zip(good, bad)), (case.name, m)
            with pytest.raises(AssertionError):
                case.claim(bad)


def test_case_names_cover_what_the_kernel_can_get_wrong():
    names = {c.name for c in IC.STEP_CASES}
    assert {"threshold_inclusive", "tie_by_seen", "tie_by_entry", "tie_by_slot", "domino_127_against_126", "size_gate_equality",
            "size_gate_zero_area_r64", "size_gate_zero_area_r0", "size_gate_needs_64_bits", "forget_boundary_and_reuse",
            "eviction_when_full", "orphaned_uid_returns", "never_visible"} <= names
    both_sides = [c for c in IC.STEP_CASES if c.name.startswith("tie_by")]
    for c in both_sides:                          # entries / slots on both sides of the wave boundary at 64
        idx = set(c.entries) | {s for tracks, _ in c.steps for s in np.nonzero(tracks[:, 0])[0].tolist()}
        assert min(idx) < 64, c.name
    assert any(max(c.entries) >= 64 for c in both_sides) and any(max(np.nonzero(c.steps[0][0][:, 0])[0]) >= 64 for c in both_sides)
    domino = next(c for c in IC.STEP_CASES if c.name.startswith("domino"))
    assert len(domino.entries) == 126 and np.count_nonzero(domino.steps[0][0][:, 0]) == 127
    sims = {ir.similarity(domino.steps[0][1][s], domino.entries[e]["sig"]) for s in (1, 64, 127) for e in (1, 64, 126)}
    assert len(sims) == 1 and sims.pop() >= domino.q


@pytest.mark.parametrize("case", IC.SIGNATURE_CASES, ids=lambda c: c.name)
def test_signature_claim_holds_on_the_reference(case):
    sig = ir.describe(case.labels, case.image, case.xyz)
    case.claim(sig)
    assert sig.dtype == np.int32 and sig.shape == (128, 104) and not sig[0].any()
    assert not sig[:, 4:8].any() and not sig[:, 99:].any()
    total = sig[:, ir.HIST:ir.HIST_END].astype(np.int64).sum(1)
    present = sig[:, 0] > 0
    assert (total[present] <= 65536).all() and (total[present] >= 65536 - 91).all() and not total[~present].any()


def test_the_vectorised_votes_are_the_per_pixel_votes():
    rng = np.random.default_rng(5)
    px = np.concatenate([rng.integers(0, 256, size=(300, 3)), rng.integers(0, 20, size=(60, 3)),
                         [[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [16, 16, 15], [16, 16, 16]]])
    row = np.zeros(ir.WORDS, dtype=np.int64)
    for b, g, r in px.tolist():
        votes = ir.chroma_votes(b, g, r)
        assert sum(w for _, _, w in votes) == (64 if b + g + r >= 48 else 0)
        for iu, iv, w in votes:
            assert 0 <= iu <= 8 and 0 <= iv <= 8 and w > 0
            row[ir.HIST + iu * 9 + iv] += w
        if b + g + r < 48:
            row[ir.DARK] += 64
        y = (b + g + r) // 3
        row[ir.INTENSITY + (y >> 5)] += 8 * (8 - ((y & 31) >> 2))
        if (y & 31) >> 2:
            row[ir.INTENSITY + (y >> 5) + 1] += 8 * ((y & 31) >> 2)
    assert np.array_equal(row, ir.raw_histogram(px))
    assert row[ir.HIST:ir.INTENSITY].sum() == 64 * len(px) == row[ir.INTENSITY:ir.HIST_END].sum()


def test_chroma_vote_without_the_zero_weight_skip_leaves_the_table():
    """The signature mutant: pure blue has u = 64, ul = 8; without the skip its zero-weight votes address a row 9."""
    assert IC.SIGNATURE_MUTANTS == ("chroma_without_zero_skip",)
    assert ir.chroma_votes(255, 0, 0) == [(8, 0, 64)]
    bad = ir.chroma_votes(255, 0, 0, skip_zero=False)
    assert bad != ir.chroma_votes(255, 0, 0) and any(iu == 9 for iu, _, _ in bad) and any(w == 0 for _, _, w in bad)
    assert ir.chroma_votes(16, 16, 15) == [] and len(ir.chroma_votes(16, 16, 16)) == 4


def at(frame, key, pixel):
    return int(frame[key][pixel])


def test_sequences_contain_what_the_gpu_tests_rely_on():
    runs = {}
    for make in IC.SEQUENCES:
        seq = make()
        runs[seq.name] = (seq,) + IC.run_reference(seq)
    events = {name: r[2].events for name, r in runs.items()}
    assert events["tabletop"]["reid"] >= 2 and events["tabletop"]["reid_retired"] >= 1
    assert events["tabletop"]["refuse_sim"] >= 1 and events["tabletop"]["refuse_size"] >= 1
    assert events["forget"]["forget"] >= 1 and events["crowd"]["evict"] >= 1 and runs["crowd"][2].evicted >= 1
    assert runs["crowd"][2].pids > 127

    seq, frames, ident = runs["tabletop"]

    def identity_and_uid(name, t):
        p = seq.where[name][t]
        slot = at(frames[t], "tracked", p)
        entry = at(frames[t], "out", p)
        assert slot > 0 and entry > 0
        return entry, int(frames[t]["words"][entry * 5]), int(frames[t]["tracks"][slot, 0])

    # the jump: no pixel in common with the frame before, a new track uid, the same identity and pid
    before, after = identity_and_uid("jump", 4), identity_and_uid("jump", 5)
    raw4 = frames[4]["tracked"] == at(frames[4], "tracked", seq.where["jump"][4])
    raw5 = frames[5]["tracked"] == at(frames[5], "tracked", seq.where["jump"][5])
    assert not (raw4 & raw5).any() and before[2] != after[2] and before[:2] == after[:2]
    # the hidden object: its track was retired while it was away
    before, after = identity_and_uid("hidden", 2), identity_and_uid("hidden", 9)
    assert before[2] != after[2] and before[:2] == after[:2]
    assert before[2] not in frames[8]["tracks"][:, 0].tolist()
    # every object keeps one identity for as long as the test follows it, except the two that were replaced
    for name in ("drift", "jump", "hidden"):
        seen = {identity_and_uid(name, t)[:2] for t, p in enumerate(seq.where[name]) if p is not None}
        assert len(seen) == 1, name
    for name in ("recolour", "shrunk"):
        seen = [identity_and_uid(name, t)[1] for t, p in enumerate(seq.where[name]) if p is not None]
        assert len(set(seen)) == 2 and seen == sorted(seen), name

    seq, frames, ident = runs["forget"]
    p = seq.where["away"]
    pid_before = int(frames[1]["words"][at(frames[1], "out", p[1]) * 5])
    pid_after = int(frames[9]["words"][at(frames[9], "out", p[9]) * 5])
    assert pid_before != pid_after and pid_after == ident.pids
