"""uoc_scene_step without a GPU: the numpy restatement (tests/scene_reference.py) against hand-written claims at G = 8,
one claim per rule; a reference with one rule broken fails the claim named for that rule; every error path of the C
entries and of the wrapper (they are refused before any device work)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import placement_reference as P15
from tests import scene_reference as R
from unseenobjectclustering_amd import _native, placement, scene

EINVAL = -22
G = 8
ROW = dict(zip(R.ID_FIELDS, range(8)))
INFO = dict(zip(R.INFO_FIELDS, range(8)))


def run(frames, max_age=5, unknown_blocks=1, broken=None, record=None, queries=(), st=None):
    """Steps one stream through `frames` = [(state, owner) or (state, owner, drop ids)]; returns (outputs per step, state)."""
    st = R.new_state(1, G)[0] if st is None else st
    outs = []
    for fr in frames:
        drop = R.drop_words(fr[2]) if len(fr) > 2 and fr[2] is not None else None
        outs.append(R.step_one(st, fr[0], fr[1], record, drop, max_age, unknown_blocks, queries, broken))
    return outs, st


def scene8():
    """A table with an unknown corner, an obstacle of id 5 (2 x 2) and one without an id."""
    g = R.blank(R.table(G), (0, 2, 0, 2))
    g = R.put(g, (3, 5, 3, 5), 5)
    return R.put(g, (6, 7, 1, 3), 0)


# ---- the claims, one function per rule: each takes `broken` so that the mutants can run it ------------------------------------
def claim_first_step(broken=None):
    s, o = scene8()
    (out,), st = run([(s, o)], broken=broken)
    assert np.array_equal(out["state"], s) and np.array_equal(out["owner"], o)
    assert np.array_equal(out["age"], np.where(s != 0, 0, -1)) and not out["change"].any()
    assert np.array_equal(out["dist2"], P15.edt((s == 2) | (s == 0)))
    assert out["info"].tolist() == [1, 1, 60, 0, 0, 0, 0, 0]
    assert out["ids"][5].tolist() == [4, 0, 0, 0, 0, 0, 0, 0] and out["ids"][0].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert st[R.META_WORD:R.MEM_WORD].tolist() == [1, 0] + [0] * 14
    assert np.array_equal(st[R.MEM_WORD:].reshape(G, G), R.pack(s, o, 0).reshape(G, G)) and (st[R.MEM_WORD:] >= 0).all()


def claim_same_frame_twice(broken=None):
    s, o = scene8()
    (a, b), _ = run([(s, o), (s, o)], broken=broken)
    for k in ("state", "owner", "dist2", "age", "change", "ids"):
        assert np.array_equal(a[k], b[k]), k
    assert b["info"].tolist() == [1, 2, 60, 0, 0, 0, 0, 0]


def claim_blank_rectangle_is_remembered_then_forgotten(broken=None, max_age=3):
    full = scene8()
    hid = R.blank(full, (2, 6, 2, 6))                              # hides the whole of id 5 and 12 table cells
    outs, st = run([full] + [hid] * (max_age + 2), max_age=max_age, broken=broken)
    box = np.zeros((G, G), bool)
    box[2:6, 2:6] = True
    for t in range(1, max_age + 1):
        out = outs[t]
        assert np.array_equal(out["state"], full[0]) and np.array_equal(out["owner"], full[1]) and np.array_equal(out["dist2"], outs[0]["dist2"])
        assert (out["age"][box] == t).all() and np.array_equal(out["age"][~box], outs[0]["age"][~box])
        assert out["info"].tolist() == [1, t + 1, 44, 16, 0, 0, 0, 0]
        assert out["ids"][5].tolist() == [0, 4, t, 0, 0, 0, 0, 0] and not out["change"].any()
    gone = outs[max_age + 1]
    assert np.array_equal(gone["state"], hid[0]) and (gone["age"][box] == -1).all() and np.array_equal(gone["owner"], hid[1])
    assert gone["info"].tolist() == [1, max_age + 2, 44, 0, 16, 0, 0, 0] and gone["ids"][5].tolist() == [0, 0, 0, 0, 0, 0, 0, 4]
    after = outs[max_age + 2]                                       # forgotten is counted once
    assert after["info"][INFO["forgotten"]] == 0 and after["ids"][5, ROW["forgotten"]] == 0
    assert (st[R.MEM_WORD:].reshape(G, G)[box] == 0).all()


def claim_max_age_zero_is_frame_differencing(broken=None):
    full = scene8()
    hid = R.blank(full, (2, 6, 2, 6))
    moved = R.put(R.put(full, (3, 5, 3, 5), 0, state=1), (3, 5, 4, 6), 5)         # id 5 one column on
    (a, b, c), _ = run([full, hid, moved], max_age=0, broken=broken)
    assert np.array_equal(b["state"], hid[0]) and b["info"].tolist() == [1, 2, 44, 0, 16, 0, 0, 0]
    assert np.array_equal(c["state"], moved[0]) and not c["change"].any()          # nothing is remembered: nothing to contradict
    (a, c), _ = run([full, moved], max_age=0, broken=broken)
    assert c["change"][3:5, 3:6].tolist() == [[R.VANISHED, R.SAME, R.APPEARED]] * 2 and c["info"][5:].tolist() == [2, 2, 0]


def claim_moved_object_and_drop(broken=None):
    full = scene8()
    # id 5 now stands at rows 0..1, columns 5..6, and its old place is hidden; so is the obstacle without an id
    moved = R.blank(R.blank(R.put(full, (0, 2, 5, 7), 5), (3, 5, 3, 5)), (6, 7, 1, 3))
    (_, keep), _ = run([full, moved], broken=broken)
    assert (keep["state"][3:5, 3:5] == 2).all() and (keep["owner"][3:5, 3:5] == 5).all() and (keep["owner"][0:2, 5:7] == 5).all()
    assert keep["ids"][5].tolist() == [4, 4, 1, 4, 0, 0, 0, 0] and keep["ids"][0, ROW["cells_kept"]] == 2
    (_, drop5), _ = run([full, moved + ([5],)], broken=broken)
    assert (drop5["state"][3:5, 3:5] == 0).all() and (drop5["age"][3:5, 3:5] == -1).all() and (drop5["owner"][0:2, 5:7] == 5).all()
    assert drop5["ids"][5].tolist() == [4, 0, 0, 4, 0, 0, 0, 4] and drop5["ids"][0, ROW["cells_kept"]] == 2
    assert drop5["info"][INFO["forgotten"]] == 4
    (_, drop0), _ = run([full, moved + ([0],)], broken=broken)      # bit 0: the obstacles without an id, never table cells
    assert (drop0["state"][6, 1:3] == 0).all() and drop0["ids"][0].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]
    assert (drop0["state"][3:5, 3:5] == 2).all() and drop0["info"][INFO["kept"]] == 4 and drop0["info"][INFO["forgotten"]] == 2
    hid_table = R.blank(full, (7, 8, 4, 8))
    (_, t0), _ = run([full, hid_table + (list(range(128)),)], broken=broken)
    assert (t0["state"][7, 4:8] == 1).all() and t0["info"][INFO["kept"]] == 4 and t0["info"][INFO["forgotten"]] == 0


def claim_change_codes(broken=None):
    """Row 0: memory table; row 1: memory obstacle of id 3; row 2: memory unknown.  Columns: now table, obstacle 3,
    obstacle 4, obstacle without id, unknown."""
    before = R.put(R.table(G), (1, 2, 0, G), 3)
    before = R.blank(before, (2, 3, 0, G))
    now = before
    for j, (state, ident) in enumerate([(1, 0), (2, 3), (2, 4), (2, 0), (0, 0)]):
        now = R.put(now, (0, 3, j, j + 1), ident, state=state)
    (_, out), _ = run([before, now], broken=broken)
    assert out["change"][0, :5].tolist() == [R.SAME, R.APPEARED, R.APPEARED, R.APPEARED, R.SAME]
    assert out["change"][1, :5].tolist() == [R.VANISHED, R.SAME, R.REOWNED, R.REOWNED, R.SAME]
    assert out["change"][2, :5].tolist() == [R.SAME] * 5                        # the four ms == 0 cases, and unknown on unknown
    assert out["state"][2, :5].tolist() == [1, 2, 2, 2, 0] and out["age"][2, :5].tolist() == [0, 0, 0, 0, -1]
    assert out["state"][1, 4] == 2 and out["owner"][1, 4] == 3 and out["age"][1, 4] == 1 and out["age"][0, 4] == 1
    assert not out["change"][3:].any() and out["info"][5:].tolist() == [3, 1, 2]
    return out


def claim_id_rows(broken=None):
    out = claim_change_codes(broken)
    want = {3: [6, 1, 1, 1, 1, 0, 2, 0], 4: [3, 0, 0, 1, 0, 1, 0, 0], 0: [3, 0, 0, 1, 0, 1, 0, 0]}
    for a in range(128):
        assert out["ids"][a].tolist() == want.get(a, [0] * 8), a
    # oldest is a maximum: two cells of id 9 hidden for 1 and for 3 steps
    g = R.put(R.table(G), (4, 5, 2, 4), 9)
    seq = [g, R.blank(g, (4, 5, 2, 3)), R.blank(g, (4, 5, 2, 3)), R.blank(g, (4, 5, 2, 4))]
    outs, _ = run(seq, broken=broken)
    assert outs[3]["ids"][9].tolist() == [0, 2, 3, 0, 0, 0, 0, 0] and outs[3]["age"][4, 2:4].tolist() == [3, 1]


def claim_normalisation(broken=None):
    s, o = R.table(G)
    s[0, :6] = [3, -1, 2, 2, 2, 2]
    o[0, :6] = [7, 7, 0, 128, -5, 127]
    o[1, 0] = 9                                                     # an owner on a table cell
    (out,), st = run([(s, o)], broken=broken)
    assert out["state"][0, :6].tolist() == [0, 0, 2, 2, 2, 2] and out["owner"][0, :6].tolist() == [0, 0, 0, 0, 0, 127]
    assert out["owner"][1, 0] == 0 and out["age"][0, :2].tolist() == [-1, -1]
    assert out["ids"][0, 0] == 3 and out["ids"][127, 0] == 1 and (st[R.MEM_WORD:] >= 0).all()


def claim_age_limit(broken=None):
    g = R.put(R.table(G), (2, 3, 2, 3), 6)
    hid = R.blank(g, (2, 3, 2, 4))
    st = R.new_state(1, G)[0]
    run([g], st=st)
    mem = st[R.MEM_WORD:].reshape(G, G)
    mem[2, 2], mem[2, 3] = R.pack(2, 6, R.MAX_AGE - 1), R.pack(1, 0, R.MAX_AGE)
    (out,), _ = run([hid], max_age=R.MAX_AGE, st=st, broken=broken)
    assert out["age"][2, 2:4].tolist() == [R.MAX_AGE, -1] and out["state"][2, 2:4].tolist() == [2, 0]
    assert mem[2, 2] == R.pack(2, 6, R.MAX_AGE) and mem[2, 3] == 0 and (st[R.MEM_WORD:] >= 0).all()
    (out,), _ = run([hid], max_age=R.MAX_AGE, st=st, broken=broken)
    assert out["age"][2, 2] == -1 and out["ids"][6].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]


def claim_no_lattice(broken=None):
    g = scene8()
    for found in (0, 2):
        st = R.new_state(1, G)[0]
        run([g], record=R.record(), st=st, broken=broken)
        before = st.copy()
        (out,), _ = run([g], record=R.record(found=found), st=st, queries=[(0, 0, 0, P15.WIDEST)], broken=broken)
        assert np.array_equal(st, before)
        for k in ("state", "owner", "dist2", "change", "ids"):
            assert not out[k].any(), k
        assert (out["age"] == -1).all() and out["info"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and out["answers"].tolist() == [[-1, -1, 0, 0]]


def claim_restart(broken=None):
    full = scene8()
    hid = R.blank(full, (2, 6, 2, 6))
    for word in range(16):
        st = R.new_state(1, G)[0]
        run([full], record=R.record(), st=st, broken=broken)
        assert np.array_equal(R.lattice(st), R.record())            # stored on the first step
        other = R.record()
        other[word] += 1 if word != 13 else 0
        if word == 13:
            continue                                                # found must stay 1: that is rule L's other branch
        (out,), _ = run([hid], record=other, st=st, broken=broken)
        assert out["info"].tolist() == [2, 2, 44, 0, 0, 0, 0, 0], word
        assert np.array_equal(out["state"], hid[0]) and not out["change"].any() and not out["ids"][:, 1:].any()
        assert st[R.META_WORD:R.META_WORD + 2].tolist() == [2, 1] and np.array_equal(R.lattice(st), other)
        (out,), _ = run([hid], record=other, st=st, broken=broken)  # the new record was stored: no second restart
        assert out["info"][:2].tolist() == [1, 3] and st[R.META_WORD + 1] == 1
    st = R.new_state(1, G)[0]
    run([full, hid], record=R.record(), st=st, broken=broken)       # the same record: the memory holds
    assert st[R.META_WORD:R.META_WORD + 2].tolist() == [2, 0]


def claim_null_frame(broken=None):
    full = scene8()
    hid = R.blank(full, (2, 6, 2, 6))
    (a, b), st = run([full, hid], record=None, broken=broken)
    assert b["info"].tolist() == [1, 2, 44, 16, 0, 0, 0, 0] and not R.lattice(st).any()
    (out,), _ = run([hid], record=R.record(), st=st, broken=broken)  # a record after steps without one differs from zeros
    assert out["info"][0] == 2


def claim_clearance(broken=None):
    g = scene8()
    for ub in (0, 1):
        (out,), _ = run([g], unknown_blocks=ub, broken=broken)
        assert np.array_equal(out["dist2"], P15.edt_brute((g[0] == 2) | ((g[0] == 0) & bool(ub)))), ub
    assert out["dist2"][0, 0] == 0 and out["dist2"][7, 7] == 1


def claim_queries(broken=None):
    full = scene8()
    hid = R.blank(full, (2, 6, 2, 6))
    qs = [(1, 0, 0, P15.WIDEST), (1, 3, 3, P15.NEAREST), (4, 3, 3, P15.NEAREST), (1 << 30, 0, 0, P15.NEAREST)]
    (a, b), _ = run([full, hid], queries=qs, broken=broken)
    d2 = P15.edt((full[0] != 1))
    want = [P15.answer(full[0].astype(np.int64), d2, q) for q in qs]
    assert a["answers"].tolist() == [list(w) for w in want] == b["answers"].tolist()
    assert a["answers"][3].tolist() == [-1, -1, 0, 0] and a["answers"][1, 3] == 1 and full[0][tuple(a["answers"][1, :2])] == 1


CLAIMS = {
    "lattice_found": claim_no_lattice, "lattice_compare": claim_restart, "lattice_store": claim_restart,
    "normalise_state": claim_normalisation, "normalise_owner": claim_normalisation, "age_limit": claim_age_limit,
    "drop": claim_moved_object_and_drop, "drop_owner0": claim_moved_object_and_drop, "appeared": claim_change_codes,
    "vanished": claim_change_codes, "reowned": claim_change_codes, "unknown_memory": claim_change_codes, "oldest": claim_id_rows,
    "forgotten_once": claim_blank_rectangle_is_remembered_then_forgotten, "clearance": claim_clearance, "query": claim_queries,
}
ALL_CLAIMS = sorted(set(CLAIMS.values()) | {claim_first_step, claim_same_frame_twice, claim_max_age_zero_is_frame_differencing,
                                            claim_null_frame}, key=lambda f: f.__name__)


@pytest.mark.parametrize("claim", ALL_CLAIMS, ids=lambda f: f.__name__)
def test_reference_meets_the_claim(claim):
    claim()


def test_blank_rectangle_at_other_ages():
    for max_age in (1, 2, 6):
        claim_blank_rectangle_is_remembered_then_forgotten(max_age=max_age)


@pytest.mark.parametrize("rule", R.BREAKS)
def test_a_broken_rule_fails_its_claim(rule):
    assert set(CLAIMS) == set(R.BREAKS)
    with pytest.raises(AssertionError):
        CLAIMS[rule](broken=rule)


def test_brute_and_separable_transforms_agree_and_sequences_hold_what_they_are_for():
    for seed in range(3):
        s, _ = R.blobs(64, seed)
        for ub in (0, 1):
            assert np.array_equal(R.clearance(s, ub, brute=True), R.clearance(s, ub, brute=False))
    frames = R.sequence(64, 0)
    st = R.new_state(1, 64)[0]
    infos, ids1 = [], []
    for s, o, drop in frames:
        out = R.step_one(st, s, o, R.record(), R.drop_words(drop), 30, 1)
        infos.append(out["info"].tolist())
        ids1.append(out["ids"][1].tolist())
    assert all(i[INFO["kept"]] > 0 for i in infos[1:]) and frames[3][2] == [1]
    assert ids1[2][ROW["cells_kept"]] > 0 and ids1[2][ROW["cells_now"]] > 0          # both places of the moved blob
    assert ids1[3][ROW["forgotten"]] == ids1[2][ROW["cells_kept"]] and ids1[3][ROW["cells_kept"]] == 0
    assert drop_matches_reference()


def drop_matches_reference():
    for ids in ([], [0], [31, 32], [127], [5, 64, 96]):
        assert np.array_equal(scene.drop_mask(ids, 2), np.stack([R.drop_words(ids)] * 2))
    assert np.array_equal(scene.drop_mask([[1], [2, 127]], 2), np.stack([R.drop_words([1]), R.drop_words([2, 127])]))
    return True


# ---- the mirrored constants -----------------------------------------------------------------------------------------------
def test_constants_agree():
    assert (R.META_WORD, R.MEM_WORD, R.MAX_AGE) == (_native.SCENE_META_WORD, _native.SCENE_MEM_WORD, _native.SCENE_MAX_AGE)
    assert (R.SAME, R.APPEARED, R.VANISHED, R.REOWNED) == tuple(scene.CODES[k] for k in ("same", "appeared", "vanished", "reowned"))
    assert R.ID_FIELDS == scene.ID_FIELDS and R.INFO_FIELDS == scene.INFO_FIELDS
    assert scene.state_words(8) == R.new_state(1, 8).shape[1]


# ---- error paths ----------------------------------------------------------------------------------------------------------
def test_bytes_functions():
    lib = _native.lib()
    assert lib.uoc_scene_state_bytes(1, 8) == 192 + 4 * 64 and lib.uoc_scene_state_bytes(3, 512) == 3 * (192 + 4 * 512 * 512)
    assert lib.uoc_scene_state_bytes(3, 40) // 3 % 16 == 0
    assert lib.uoc_scene_workspace_bytes(2, 64) >= 2 * (128 * 8 + 8) * 4 + 2 * 16 * 8
    for shape in ((0, 64), (-1, 64), (65536, 64), (1, 0), (1, 12), (1, 520), (1, 4), (1, -8)):
        assert lib.uoc_scene_state_bytes(*shape) == 0 and lib.uoc_scene_workspace_bytes(*shape) == 0, shape


def test_every_einval_path_is_refused_before_device_work():
    lib = _native.lib()
    B, G_, Q = 2, 64, 2
    nws = lib.uoc_scene_workspace_bytes(B, G_)
    good_q = [4, 0, 0, 0, 1, -4096, 4095, 1]
    fake = lambda n: ctypes.c_void_p(4096 * n)          # noqa: E731  never dereferenced: every call below is refused first
    names = ("state_cur", "owner_cur", "frame", "drop", "mem", "state", "owner", "dist2", "age", "change", "ids", "info", "answers", "ws")

    def call(B_=B, G_=G_, max_age=30, ub=1, queries=good_q, Q_=Q, nws_=nws, drop=(), **ptrs):
        hq = (ctypes.c_int32 * max(len(queries), 1))(*queries)
        p = {k: fake(i + 1) for i, k in enumerate(names)}
        p["queries"] = ctypes.cast(hq, ctypes.c_void_p)
        p.update(ptrs)
        for k in drop:
            p[k] = None
        return lib.uoc_scene_step(p["state_cur"], p["owner_cur"], p["frame"], p["drop"], B_, G_, max_age, ub, p["queries"], Q_, p["mem"],
                                  p["state"], p["owner"], p["dist2"], p["age"], p["change"], p["ids"], p["info"], p["answers"], p["ws"],
                                  nws_, None)

    cases = [dict(drop=(k,)) for k in names if k not in ("frame", "drop")] + [dict(drop=("queries",))] + [
        dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(G_=4), dict(max_age=-1), dict(max_age=32768),
        dict(ub=2), dict(ub=-1), dict(Q_=-1), dict(Q_=17), dict(queries=[-1, 0, 0, 0] + good_q[4:]), dict(queries=[(1 << 30) + 1, 0, 0, 0] + good_q[4:]),
        dict(queries=good_q[:4] + [1, 4096, 0, 1]), dict(queries=good_q[:4] + [1, 0, -4097, 1]), dict(queries=good_q[:4] + [1, 0, 0, 2]),
        dict(nws_=nws - 1), dict(nws_=0), dict(ws=ctypes.c_void_p(4096 * 14 + 4)), dict(mem=ctypes.c_void_p(4096 * 5 + 4)),
        dict(mem=ctypes.c_void_p(4096 * 5 + 8))]
    for kw in cases:
        assert call(**kw) == EINVAL, kw
        assert b"uoc_scene_step" in lib.uoc_last_error(), kw
    assert b"aligned" in lib.uoc_last_error()
    # without queries neither the table nor the answers are needed; that call is refused only for what is still wrong
    assert call(Q_=0, drop=("queries", "answers"), nws_=0) == EINVAL and b"workspace" in lib.uoc_last_error()
    reset = lambda st=fake(1), B_=2, G_=64, which=-1: lib.uoc_scene_reset(st, B_, G_, which, None)      # noqa: E731
    for kw in (dict(st=None), dict(B_=0), dict(B_=65536), dict(G_=12), dict(G_=520), dict(which=-2), dict(which=2),
               dict(st=ctypes.c_void_p(4100))):
        assert reset(**kw) == EINVAL, kw
        assert b"uoc_scene_reset" in lib.uoc_last_error(), kw


def test_wrapper_refuses_bad_arguments():
    z = torch.zeros((1, 8, 8), dtype=torch.int32)
    mem = torch.zeros((1, scene.state_words(8)), dtype=torch.int32)
    with pytest.raises(_native.NativeError):
        scene.scene_records(z, z, None, None, mem, 30, 1)                       # no CPU fallback
    with pytest.raises(_native.NativeError):
        scene.Memory(8, device="cpu")
    for kw in (dict(grid=12), dict(grid=0), dict(grid=520), dict(grid=8, max_age=-1), dict(grid=8, max_age=32768), dict(grid=8, streams=0),
               dict(grid=8, streams=65536)):
        with pytest.raises(ValueError):
            scene.Memory(**kw)
    for bad in ([128], [-1], [[1], [2], [3]]):
        with pytest.raises(ValueError):
            scene.drop_mask(bad, 2)
    # update's own checks come before any device work: a Memory made without its constructor stands in for one on a GPU
    m = scene.Memory.__new__(scene.Memory)
    m.grid, m.max_age, m.unknown_blocks, m.streams, m.state = 8, 30, None, 1, mem
    ok = placement.PlacementResult(state=z, owner=z, grid=8, cell_mm=10, unknown_blocks=True)
    for other in (placement.PlacementResult(state=z, owner=z, grid=16, cell_mm=10), placement.PlacementResult(state=z[:, :, :4], owner=z, grid=8, cell_mm=10),
                  placement.PlacementResult(state=torch.zeros((2, 8, 8), dtype=torch.int32), owner=z, grid=8, cell_mm=10)):
        with pytest.raises(ValueError):
            m.update(other)
    for q in ([(0, 0, 0, 2)], [(-1, 0, 0, 0)], [(0, 0, 0, 0)] * 17):
        with pytest.raises(ValueError):
            m.update(ok, queries=q)
    with pytest.raises(ValueError):
        m.reset(1)
    with pytest.raises(_native.NativeError):
        m.update(ok)                                                            # CPU tensors are refused


def test_changed_and_remembered_on_records():
    ids = np.zeros((1, 128, 8), np.int32)
    ids[0, 3, 3], ids[0, 4, 3], ids[0, 4, 4], ids[0, 0, 4] = 4, 3, 9, 4
    res = scene.SceneResult(ids=torch.from_numpy(ids), age=torch.tensor([[[0, 2], [-1, 1]]]))
    app, van = scene.changed(res)
    assert torch.nonzero(app[0]).flatten().tolist() == [3] and torch.nonzero(van[0]).flatten().tolist() == [0, 4]
    app, _ = scene.changed(res, min_cells=3)
    assert torch.nonzero(app[0]).flatten().tolist() == [3, 4]
    assert scene.remembered_mask(res).tolist() == [[[False, True], [False, True]]]
