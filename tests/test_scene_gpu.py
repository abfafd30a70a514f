"""uoc_scene_step / scene.Memory on the GPU against the numpy restatement (tests/scene_reference.py).

The stage has no floating-point output.  After every step of every sequence all eight outputs and the whole state of
every stream, header included, are compared with np.array_equal.  The sequences are generated in the reference module
and tests/test_scene_host.py asserts on the CPU that they contain what they are used for here.

Sizes: G = 8 (the hand sequences), 64 with B = 3 (seeded, two blocks per frame), 40 (the second strip of the column pass
holds 8 of its 32 columns) and 512 (all 8 row segments of the column scan and 8 ballot words are live; an index of the
state above 2^18).

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import ctypes
import faulthandler
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import placement_reference as P15
from tests import scene_reference as R
from unseenobjectclustering_amd import _native, footprint, placement, routes, scene

pytestmark = pytest.mark.gpu
EINVAL = -22
KEYS = ("state", "owner", "dist2", "age", "change", "ids", "info", "answers")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def up(device, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def compare(got, want, where):
    for k in want:
        g = got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (where, k, g.dtype, g.shape, want[k].shape)
        bad = g != want[k]
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6], want[k][bad][:6])


def both(device, mem, ref, s, o, frame, drop, max_age, ub, queries, where):
    """One step on the device and in the reference; compares the outputs and the whole state.  s, o [B,G,G]; frame [B,16]
    or None; drop [B,4] or None (numpy).  Returns the device outputs as numpy."""
    out = scene.scene_records(up(device, s), up(device, o), up(device, frame), up(device, drop), mem, max_age, ub, queries)
    got = {k: t.cpu().numpy() for k, t in zip(KEYS, out)}
    want = R.step(ref, s, o, frame, drop, max_age, ub, queries)
    compare(got, want, where)
    compare({"mem": mem.cpu().numpy()}, {"mem": ref}, where)
    return got


def fresh(device, B, G):
    return torch.zeros((B, scene.state_words(G)), dtype=torch.int32, device=device), R.new_state(B, G)


def stack_frames(frames, B):
    """[(state, owner, drop ids, record)] * B of one step -> the batched numpy inputs of `both`."""
    s, o = np.stack([f[0] for f in frames]).astype(np.int32), np.stack([f[1] for f in frames]).astype(np.int32)
    recs = [f[3] for f in frames]
    frame = None if all(r is None for r in recs) else np.stack(recs)
    drop = None if all(f[2] is None for f in frames) else np.stack([R.drop_words(f[2] or []) for f in frames])
    return s, o, frame, drop


QUERIES8 = [(1, 0, 0, P15.WIDEST), (1, 3, 3, P15.NEAREST), (4, 6, 1, P15.NEAREST)]


@pytest.mark.parametrize("name", list(R.hand_sequences()))
def test_hand_sequences_match_reference(device, name):
    frames, kw = R.hand_sequences()[name]
    mem, ref = fresh(device, 1, 8)
    for t, fr in enumerate(frames):
        s, o, frame, drop = stack_frames([fr], 1)
        both(device, mem, ref, s, o, frame, drop, kw["max_age"], kw.get("unknown_blocks", 1), QUERIES8, (name, t))


@pytest.mark.parametrize("max_age", [0, 1, 32767])
def test_age_limits(device, max_age):
    """A cell hidden for three steps at each limit; and a memory word one step short of 32767 and one at it."""
    G = 8
    g = R.put(R.table(G), (2, 3, 2, 4), 6)
    hid = R.blank(g, (2, 4, 1, 5))
    mem, ref = fresh(device, 1, G)
    for t, fr in enumerate([g, hid, hid, hid, g]):
        got = both(device, mem, ref, fr[0][None], fr[1][None], None, None, max_age, 1, (), (max_age, t))
        if t in (1, 2, 3):
            assert got["age"][0, 2, 2] == (t if t <= max_age else -1)
    idx = R.MEM_WORD + 2 * G
    for words in (ref[0], mem[0]):
        words[idx + 2], words[idx + 3] = int(R.pack(2, 6, R.MAX_AGE - 1)), int(R.pack(1, 0, R.MAX_AGE))
    got = both(device, mem, ref, hid[0][None], hid[1][None], None, None, max_age, 1, (), (max_age, "old"))
    assert got["age"][0, 2, 2:4].tolist() == ([R.MAX_AGE, -1] if max_age == R.MAX_AGE else [-1, -1])
    assert int(mem.min()) >= 0


@functools.lru_cache(maxsize=None)
def seeded(G, B, steps=6):
    """Per step the B frames of R.sequence(G, seed = b); stream 1 gets another record from step 3 on: a restart."""
    seqs = [R.sequence(G, b, steps) for b in range(B)]
    out = []
    for t in range(steps):
        out.append([(seqs[b][t][0], seqs[b][t][1], seqs[b][t][2], R.record(seed=7 if (b == 1 and t >= 3) else 0)) for b in range(B)])
    return out


def scene_queries(G):
    return [(4, 0, 0, P15.WIDEST), (9, G // 2, G // 2, P15.NEAREST), (1, -5, G + 3, P15.NEAREST)]


def test_seeded_sequences_of_three_streams_match_reference(device):
    G, B = 64, 3
    mem, ref = fresh(device, B, G)
    infos = []
    for t, frames in enumerate(seeded(G, B)):
        got = both(device, mem, ref, *stack_frames(frames, B), 30, 1, scene_queries(G), ("seeded", t))
        infos.append(got["info"])
    assert [int(i[1, 0]) for i in infos] == [1, 1, 1, 2, 1, 1] and all((i[[0, 2], 0] == 1).all() for i in infos)
    assert ref[:, R.META_WORD + 1].tolist() == [0, 1, 0] and infos[3][0, 4] > 0          # stream 0 dropped id 1 at step 3


def test_a_stream_alone_equals_the_stream_among_two_others_and_two_runs_agree(device):
    G, B = 64, 3
    runs = []
    for _ in range(2):
        mem = torch.zeros((B, scene.state_words(G)), dtype=torch.int32, device=device)
        outs = []
        for frames in seeded(G, B):
            s, o, frame, drop = stack_frames(frames, B)
            outs.append(scene.scene_records(up(device, s), up(device, o), up(device, frame), up(device, drop), mem, 30, 1, scene_queries(G)))
        runs.append((outs, mem))
    for a, b in zip(*(r[0] for r in runs)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(runs[0][1], runs[1][1])
    for b in range(B):
        mem = torch.zeros((1, scene.state_words(G)), dtype=torch.int32, device=device)
        for t, frames in enumerate(seeded(G, B)):
            s, o, frame, drop = stack_frames(frames[b:b + 1], 1)
            alone = scene.scene_records(up(device, s), up(device, o), up(device, frame), up(device, drop), mem, 30, 1, scene_queries(G))
            for k, x, y in zip(KEYS, alone, runs[0][0][t]):
                assert torch.equal(x[0], y[b]), (b, t, k)
        assert torch.equal(mem[0], runs[0][1][b])


def test_partial_strip_matches_reference(device):
    """G = 40: the second strip of the column pass holds 8 of its 32 columns and a row segment 5 rows."""
    G = 40
    mem, ref = fresh(device, 1, G)
    for t, fr in enumerate(R.sequence(G, 5, 4)):
        assert (fr[0][:, 32:] == 2).any() or t > 0
        both(device, mem, ref, fr[0][None], fr[1][None], R.record()[None], R.drop_words(fr[2])[None], 2, t % 2, scene_queries(G), ("G40", t))


def test_largest_grid_matches_reference(device):
    """G = 512, three steps: an object on the last row and column, a blank band across the borders of the row segments
    (rows 60..70 and 250..260 span the borders at 64 and 256) that is remembered, then moved."""
    G = 512
    full = R.put(R.blobs(G, 11, n=12), (G - 3, G, G - 2, G), 9)
    frames = [full, R.blank(R.blank(full, (60, 70, 0, G)), (250, 260, 17, 400)), R.blank(full, (120, 135, 0, G))]
    assert full[0][G - 1, G - 1] == 2 and full[1][G - 1, G - 1] == 9
    mem, ref = fresh(device, 1, G)
    qs = [(16, 0, 0, P15.WIDEST), (100, G - 1, G - 1, P15.NEAREST)]
    for t, fr in enumerate(frames):
        got = both(device, mem, ref, fr[0][None], fr[1][None], R.record()[None], None, 30, 1, qs, ("G512", t))
        assert np.array_equal(got["state"][0], full[0]) and int(got["dist2"].max()) > 64
    assert int(got["age"][0, 125, 7]) == 1 and int(got["age"][0, 65, 7]) == 0


@pytest.mark.parametrize("Q", [0, 1, 16])
def test_queries_on_a_first_step_equal_placements(device, Q):
    """Memory.update on a fresh memory: the fused grids, the clearance and the answers of both query modes are those
    uoc_placement gave on the same grid."""
    c = P15.case_single_block()
    qs = c["queries"][:Q]
    assert Q < 16 or {q[3] for q in qs} == {P15.WIDEST, P15.NEAREST}
    plane = tuple(c["plane"][k] for k in ("normal", "d", "centroid", "u", "v"))
    placed = placement.free_space(up(device, c["lab"]), up(device, c["xyz"]), plane, grid=c["G"], cell=0.01, h_obs=0.02, tau=0.01, queries=qs)
    mem = scene.Memory(c["G"], device=device)
    res = mem.update(placed, queries=qs)
    for k in ("state", "owner", "dist2", "answers"):
        assert torch.equal(getattr(res, k), getattr(placed, k)) and torch.equal(getattr(res.placed, k), getattr(placed, k)), k
    assert res.answers.shape == (1, Q, 4) and torch.equal(res.placed.cells, placed.cells) and int(mem.steps()[0]) == 1
    assert res.placed.frame is placed.frame and res.placed.planes is placed.planes and res.placed.unknown_blocks is True
    assert not bool(res.change.any()) and torch.equal(res.age, torch.where(placed.state != 0, 0, -1).to(torch.int32))
    if Q == 1:                                                  # the other mode alone
        other = scene.Memory(c["G"], device=device).update(placed, queries=[c["queries"][2]])
        again = placement.free_space(up(device, c["lab"]), up(device, c["xyz"]), plane, grid=c["G"], cell=0.01, h_obs=0.02, tau=0.01,
                                     queries=[c["queries"][2]])
        assert c["queries"][2][3] == P15.NEAREST and torch.equal(other.answers, again.answers)


def test_reset_which(device):
    G, B = 8, 3
    frames = R.hand_sequences()["blank_then_forgotten"][0]
    mem = scene.Memory(G, max_age=5, streams=B, device=device)
    ref = R.new_state(B, G)
    placed = lambda fr: placement.PlacementResult(state=up(device, np.stack([fr[0]] * B)), owner=up(device, np.stack([fr[1]] * B)),      # noqa: E731
                                                  frame=up(device, np.stack([fr[3]] * B)), cells=torch.zeros((B, 128), dtype=torch.int32, device=device),
                                                  planes=None, grid=G, cell_mm=10, h_obs_mm=10, tau_mm=10, min_pts=1, unknown_blocks=True)
    for t, fr in enumerate(frames[:3]):
        res = mem.update(placed(fr))
        want = R.step(ref, np.stack([fr[0]] * B), np.stack([fr[1]] * B), np.stack([fr[3]] * B), None, 5, 1)
        compare({k: getattr(res, k).cpu().numpy() for k in KEYS}, want, ("reset", t))
    assert mem.steps().tolist() == [3, 3, 3]
    mem.reset(1)
    R.reset(ref, 1)
    assert np.array_equal(mem.state.cpu().numpy(), ref) and mem.steps().tolist() == [3, 0, 3]
    res = mem.update(placed(frames[3]))
    want = R.step(ref, np.stack([frames[3][0]] * B), np.stack([frames[3][1]] * B), np.stack([frames[3][3]] * B), None, 5, 1)
    compare({k: getattr(res, k).cpu().numpy() for k in KEYS}, want, "after reset")
    assert res.info[:, 3].tolist() == [16, 0, 16] and np.array_equal(mem.state.cpu().numpy(), ref)
    mem.reset()
    assert not bool(mem.state.any())
    for bad in (-2, 3):
        with pytest.raises(ValueError):
            mem.reset(bad)


def test_non_contiguous_int64_inputs_and_device_drop_masks(device):
    G, B = 64, 2
    frames = seeded(G, 3)
    a_mem, b_mem = (torch.zeros((B, scene.state_words(G)), dtype=torch.int32, device=device) for _ in range(2))
    for t in range(4):
        s, o, frame, _ = stack_frames(frames[t][:B], B)
        ids = [[1, 31, 32], [127, 0]] if t == 3 else [[], []]
        plain = scene.scene_records(up(device, s), up(device, o), up(device, frame), up(device, scene.drop_mask(ids, B)), a_mem, 30, 1)
        wide_s = torch.zeros((B, G, 2 * G), dtype=torch.int64, device=device)
        wide_o = torch.zeros((B, G, 2 * G), dtype=torch.int64, device=device)
        wide_s[:, :, ::2], wide_o[:, :, ::2] = up(device, s).long(), up(device, o).long()
        bits = torch.zeros((B, 128), dtype=torch.bool, device=device)
        for b, row in enumerate(ids):
            if row:
                bits[b, row] = True
        packed = scene._pack_drop(bits, B, torch.device(device))
        assert np.array_equal(packed.cpu().numpy(), scene.drop_mask(ids, B)) and packed.dtype == torch.int32
        assert not wide_s[:, :, ::2].is_contiguous()
        other = scene.scene_records(wide_s[:, :, ::2], wide_o[:, :, ::2], up(device, frame), packed, b_mem, 30, 1)
        assert all(torch.equal(x, y) for x, y in zip(plain, other)) and torch.equal(a_mem, b_mem)
    every = torch.ones((B, 128), dtype=torch.bool, device=device)
    assert scene._pack_drop(every, B, torch.device(device)).tolist() == [[-1] * 4] * B


def test_rejected_calls_leave_outputs_state_and_workspace_alone(device):
    lib = _native.lib()
    B, G, Q = 2, 16, 2
    nws = lib.uoc_scene_workspace_bytes(B, G)
    nst = lib.uoc_scene_state_bytes(B, G)
    assert nws > 0 and nst == B * 4 * scene.state_words(G)
    shapes = dict(state=(B, G, G), owner=(B, G, G), dist2=(B, G, G), age=(B, G, G), change=(B, G, G), ids=(B, 128, 8), info=(B, 8), answers=(B, Q, 4))
    outs = {k: torch.full(shape, -7, dtype=torch.int32, device=device) for k, shape in shapes.items()}
    ws = torch.full((nws + 16,), 0x55, dtype=torch.uint8, device=device)
    mem = torch.full((nst // 4 + 4,), 0x01010101, dtype=torch.int32, device=device)
    cur = torch.ones((B, G, G), dtype=torch.int32, device=device)
    frame = up(device, np.stack([R.record()] * B))
    P, st = _native.ptr, _native.stream_ptr(device)
    good_q = [(4, 0, 0, 0), (1, 3, 3, 1)]
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)         # noqa: E731
    assert ws.data_ptr() % 16 == 0 and mem.data_ptr() % 16 == 0

    def call(B_=B, G_=G, max_age=30, ub=1, qs=good_q, Q_=None, ws_=None, nws_=nws, mem_=None, drop=None, null_q=False, cur_=cur):
        hq = (ctypes.c_int32 * (4 * max(len(qs), 1)))(*[x for q in qs for x in q])
        o = {k: (None if k == drop else v) for k, v in outs.items()}
        return lib.uoc_scene_step(P(cur_), P(cur), P(frame), None, B_, G_, max_age, ub, None if null_q else ctypes.cast(hq, ctypes.c_void_p),
                                  len(qs) if Q_ is None else Q_, P(mem) if mem_ is None else mem_, P(o["state"]), P(o["owner"]), P(o["dist2"]),
                                  P(o["age"]), P(o["change"]), P(o["ids"]), P(o["info"]), P(o["answers"]), P(ws) if ws_ is None else ws_, nws_, st)

    for kw in (dict(B_=0), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(max_age=-1), dict(max_age=32768), dict(ub=2), dict(Q_=-1),
               dict(Q_=17), dict(null_q=True), dict(qs=[(-1, 0, 0, 0)]), dict(qs=[(1, 4096, 0, 1)]), dict(qs=[(1, 0, 0, 2)]), dict(nws_=nws - 1),
               dict(ws_=off(ws, 4)), dict(mem_=off(mem, 4)), dict(mem_=ctypes.c_void_p(0)), dict(ws_=ctypes.c_void_p(0)), dict(cur_=None),
               *[dict(drop=k) for k in shapes]):
        assert call(**kw) == EINVAL, kw
        assert b"uoc_scene_step" in lib.uoc_last_error()
    for kw in (dict(which=-2), dict(which=B), dict(G_=12), dict(mem_=off(mem, 4))):
        assert lib.uoc_scene_reset(kw.get("mem_", P(mem)), B, kw.get("G_", G), kw.get("which", -1), st) == EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs.values()) and bool((ws == 0x55).all()) and bool((mem == 0x01010101).all())
    assert lib.uoc_scene_reset(P(mem), B, G, 1, st) == 0          # stream 1 alone, and not a word past the state
    torch.cuda.synchronize()
    per = scene.state_words(G)
    assert bool((mem[:per] == 0x01010101).all()) and not bool(mem[per:2 * per].any()) and bool((mem[2 * per:] == 0x01010101).all())
    assert lib.uoc_scene_reset(P(mem), B, G, -1, st) == 0 and call() == 0 and call(qs=[], null_q=True, drop="answers") == 0
    torch.cuda.synchronize()
    assert outs["info"][:, :4].tolist() == [[1, 2, G * G, 0]] * B and bool((mem[2 * per:] == 0x01010101).all()) and bool((ws[nws:] == 0x55).all())
    with pytest.raises(_native.NativeError):
        scene.scene_records(cur.cpu(), cur, None, None, mem[:2 * per].view(B, per), 30, 1)
    with pytest.raises(_native.NativeError):
        scene.scene_records(cur, cur, None, None, mem[:per].view(1, per), 30, 1)          # one stream's state for two frames
    with pytest.raises(_native.NativeError):
        scene.scene_records(cur, cur, frame[:1], None, mem[:2 * per].view(B, per), 30, 1)
    with pytest.raises(ValueError):
        scene.scene_records(cur, cur, None, None, mem[:2 * per].view(B, per), 32768, 1)


def test_a_hidden_band_of_the_image_changes_no_route_and_no_put_down_pose(device):
    """The reason the stage exists.  The placement generator's scene; in the second frame the points of an image band are
    gone (an arm over the table).  On that frame alone the routes and the put-down poses differ; on the fused grid they are
    those of the full first frame."""
    lab, xyz = P15.tabletop(122, 166, 1, holes=0.02)
    hidden = xyz.copy()
    hidden[:, 60:80, :] = 0.0
    plane = tuple(P15.true_plane()[k] for k in ("normal", "d", "centroid", "u", "v"))
    dl = up(device, lab)
    full = placement.free_space(dl, up(device, xyz), plane, grid=64)
    part = placement.free_space(dl, up(device, hidden), plane, grid=64)
    mem = scene.Memory(64, max_age=30, device=device)
    first, second = mem.update(full), mem.update(part)
    ref = R.new_state(1, 64)
    for res, placed in ((first, full), (second, part)):
        want = R.step(ref, placed.state.cpu().numpy(), placed.owner.cpu().numpy(), placed.frame.cpu().numpy(), None, 30, 1)
        compare({k: getattr(res, k).cpu().numpy() for k in KEYS}, want, "band")
    assert np.array_equal(mem.state.cpu().numpy(), ref)
    assert int(second.info[0, 3]) > 400 and int(second.ids[0, :, 1].sum()) > 50 and not bool(second.change.any())
    assert torch.equal(second.state, full.state) and torch.equal(second.owner, full.owner) and torch.equal(second.dist2, full.dist2)
    assert not torch.equal(part.state, full.state)
    assert torch.equal(second.placed.cells[:, 1:], full.cells[:, 1:]) and torch.equal(second.placed.cells[:, 0], part.cells[:, 0])
    assert torch.equal(scene.remembered_mask(second), (part.state == 0) & (full.state != 0))
    st = full.state[0].cpu().numpy()
    free = np.argwhere((st == 1) & (full.dist2[0].cpu().numpy() >= 4))
    src = tuple(int(x) for x in free[0])
    field = routes.plan(full, [routes.query(0.01, src, None, 10)]).cost[0, 0].cpu().numpy()
    dst = tuple(int(x) for x in np.unravel_index(np.argmax(field), field.shape))          # the farthest cell the disc reaches
    q = [routes.query(0.01, src, dst, 10), routes.query(0.01, dst, None, 10)]
    rects = [footprint.rect(0.06, 0.03, 10), footprint.rect(0.04, 0.04, 10, near=src)]
    r_full, r_part, r_mem = (routes.plan(p, q) for p in (full, part, second.placed))
    f_full, f_part, f_mem = (footprint.fit(p, rects) for p in (full, part, second.placed))
    for k in ("cost", "info", "path"):
        assert torch.equal(getattr(r_mem, k), getattr(r_full, k)), k
    for k in ("fits", "count", "best"):
        assert torch.equal(getattr(f_mem, k), getattr(f_full, k)), k
    assert r_full.info[0, 0, :2].tolist() == [1, 1] and r_part.info[0, 0, :2].tolist() == [1, 0]      # the band alone closes the route ...
    assert not torch.equal(f_part.count, f_full.count)                                               # ... and takes put-down poses away


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_demo_frame_against_itself(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out0, ref0, objs0, fitted0, placed0 = O.segment_objects(sample, net, net_crop, placement=True)
    mem = scene.Memory(256, device=device)
    results = []
    for _ in range(2):
        np.random.seed(3)
        out1, ref1, objs1, fitted, placed, res = O.segment_objects(sample, net, net_crop, memory=mem)
        assert torch.equal(out0, out1) and torch.equal(ref0, ref1) and torch.equal(placed.state, placed0.state)
        results.append((placed, res))
    ref = R.new_state(1, 256)
    for t, (placed, res) in enumerate(results):
        want = R.step(ref, placed.state.cpu().numpy(), placed.owner.cpu().numpy(), placed.frame.cpu().numpy(), None, 30, 1)
        compare({k: getattr(res, k).cpu().numpy() for k in KEYS}, want, ("demo", t))
    assert np.array_equal(mem.state.cpu().numpy(), ref)
    a, b = results[0][1], results[1][1]
    assert b.info[0].tolist() == [1, 2, int(a.info[0, 2]), 0, 0, 0, 0, 0] and int(a.info[0, 2]) > 100
    for k in ("state", "owner", "dist2", "age", "change", "ids"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(b.state, results[1][0].state) and torch.equal(b.placed.cells, results[1][0].cells)
