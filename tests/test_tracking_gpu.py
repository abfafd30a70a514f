"""uoc_track_step / Tracker on the GPU against the plain-integer reference (tests/tracking_reference.py), bit for bit:
the tracker has no float arithmetic, so every comparison is np.array_equal / torch.equal.

The sequences are generated here (seeded): 6-12 ellipses and rectangles that drift a few pixels per frame, pass in front
of each other, start outside or leave the image, appear late, disappear for 1..8 frames, with raw ids re-drawn every
frame.  Before any GPU work each test checks on the CPU that the reference run of its sequences really contains the
events it claims to cover (matches, births after step 0, retirements, recoveries after an occlusion, slot reuse).

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import faulthandler
import functools
import sys

import numpy as np
import pytest
import torch

from tests.tracking_reference import ReferenceTracker
from unseenobjectclustering_amd import _native, tracking
from unseenobjectclustering_amd import objects as O

pytestmark = pytest.mark.gpu

T_FRAMES = 40
SIZES = [(480, 640), (224, 224), (37, 53)]
SEEDS = (1, 2, 3, 4)
META = _native.TRACK_META_WORD


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def make_sequence(seed, H, W, T=T_FRAMES):
    """[T,H,W] int32 raw label maps of one stream."""
    rng = np.random.default_rng(1000 * seed + H)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    S = float(min(H, W))
    n = int(rng.integers(6, 13))
    speed = max(0.8, S / 90.0)
    objs = []
    for k in range(n):
        hide = np.zeros(T, dtype=bool)
        for _ in range(int(rng.integers(0, 3))):                  # up to two absences of 1..8 frames
            a = int(rng.integers(1, T - 2))
            hide[a:a + int(rng.integers(1, 9))] = True
        if rng.random() < 0.35:                                   # appears late
            hide[:int(rng.integers(2, T // 2))] = True
        objs.append(dict(rect=bool(rng.random() < 0.5), a=rng.uniform(S / 14, S / 5), b=rng.uniform(S / 14, S / 5),
                         cx=rng.uniform(-0.1 * W, 1.1 * W), cy=rng.uniform(-0.1 * H, 1.1 * H),
                         vx=rng.uniform(-speed, speed), vy=rng.uniform(-speed, speed), hide=hide))
    frames = np.zeros((T, H, W), dtype=np.int32)
    for t in range(T):
        ids = rng.choice(np.arange(1, 128), size=n, replace=False)      # raw ids re-drawn every frame
        img = frames[t]
        junk = rng.random((H, W)) < 0.01                          # values that must read as background
        img[junk] = rng.choice(np.array([-1, 128, 255, -1000, 1 << 20], dtype=np.int32), size=int(junk.sum()))
        for k, o in enumerate(objs):                              # painted back to front: later objects occlude earlier ones
            if o["hide"][t]:
                continue
            dx, dy = np.abs(xs - (o["cx"] + t * o["vx"])), np.abs(ys - (o["cy"] + t * o["vy"]))
            mask = ((dx <= o["a"]) & (dy <= o["b"])) if o["rect"] else ((dx / o["a"]) ** 2 + (dy / o["b"]) ** 2 <= 1.0)
            img[mask] = ids[k]
    return frames


def run_reference(frames, min_iou, max_age, reset_at=None):
    """Per step: out, lut, table, mem (the maps as uint8: slots are <= 127), meta; and the event counts."""
    ref = ReferenceTracker(min_iou, max_age)
    steps, events = [], dict(match=0, birth=0, retire=0, recover=0, reuse=0)
    for t in range(frames.shape[0]):
        if reset_at is not None and t == reset_at:
            for k, v in ref.events.items():
                events[k] += v
            ref.reset()
        out = ref.step(frames[t])
        steps.append((out.astype(np.uint8), ref.lut.astype(np.int32), ref.table32(), ref.mem.astype(np.uint8), ref.meta()))
    for k, v in ref.events.items():
        events[k] += v
    return steps, events


def assert_state(tr, want, stream=0, where=""):
    out8, lut, table, mem8, meta = want
    assert np.array_equal(tr.lut[stream].cpu().numpy(), lut), where
    assert np.array_equal(tr.table[stream].cpu().numpy(), table), where
    words = tr.state_words[stream].cpu().numpy()
    assert np.array_equal(words[:128 * 5].reshape(128, 5), table), where       # the state's own copy of the table
    assert (int(words[META]) + 1, int(words[META + 1]), int(words[META + 2])) == (meta["next_uid"], meta["step"], meta["dropped"]), where
    assert np.array_equal(tr.memory[stream].cpu().numpy(), mem8.astype(np.int32)), where
    hdr, cont = _native.TRACK_HEADER_WORDS, _native.TRACK_CONT_WORDS
    assert not words[hdr:hdr + cont].any(), where                              # the contingency scratch is left zero


@pytest.mark.parametrize("max_age", [0, 2, 5])
@pytest.mark.parametrize("min_iou", [0.1, 0.3, 0.6])
@pytest.mark.parametrize("H,W", SIZES)
def test_sequences_match_reference(device, H, W, min_iou, max_age):
    # CPU first: the reference runs, and they must contain what this test claims to cover
    runs, total = [], dict(match=0, birth=0, retire=0, recover=0, reuse=0)
    for seed in SEEDS:
        frames = make_sequence(seed, H, W)
        steps, events = run_reference(frames, min_iou, max_age)
        runs.append((seed, frames, steps))
        for k, v in events.items():
            total[k] += v
    needed = ("match", "birth", "retire", "reuse") + (("recover",) if max_age > 0 else ())
    for k in needed:
        assert total[k] > 0, f"the generated sequences contain no '{k}' event: {total}"
    # then the device, step by step
    for seed, frames, steps in runs:
        tr = tracking.Tracker(min_iou=min_iou, max_age=max_age)
        dev_frames = torch.from_numpy(frames).to(device)
        for t in range(frames.shape[0]):
            out = tr.update(dev_frames[t])
            where = f"seed {seed} step {t}"
            assert out.dtype == torch.int32 and out.shape == (H, W)
            assert np.array_equal(out.cpu().numpy(), steps[t][0].astype(np.int32)), where
            assert_state(tr, steps[t], 0, where)
        live = tr.tracks()
        table = steps[-1][2]
        assert np.array_equal(live["slot"], np.nonzero(table[:, 0])[0]) and np.array_equal(live["uid"], table[live["slot"], 0])
        assert live["dropped"] == 0 and live["step"] == T_FRAMES and live["next_uid"] == steps[-1][4]["next_uid"]


def test_label_dtypes_and_shapes(device):
    frames = make_sequence(1, 37, 53)[:6]
    steps, _ = run_reference(frames, 0.3, 5)
    for conv in (lambda x: x, lambda x: x.long(), lambda x: x.float(), lambda x: x[None]):
        tr = tracking.Tracker()
        for t in range(6):
            lab = conv(torch.from_numpy(frames[t]).to(device))
            out = tr.update(lab)
            assert out.shape == lab.shape and out.dtype == torch.int32
            assert np.array_equal(out.reshape(37, 53).cpu().numpy(), steps[t][0].astype(np.int32))
    tr = tracking.Tracker(streams=2)
    with pytest.raises(_native.NativeError):
        tr.update(torch.zeros(37, 53, dtype=torch.int32, device=device))
    # a change of size re-allocates and resets
    tr = tracking.Tracker()
    tr.update(torch.from_numpy(frames[0]).to(device))
    out = tr.update(torch.from_numpy(make_sequence(1, 224, 224)[0]).to(device))
    first, _ = run_reference(make_sequence(1, 224, 224)[:1], 0.3, 5)
    assert np.array_equal(out.cpu().numpy(), first[0][0].astype(np.int32)) and tr.tracks()["step"] == 1


@pytest.mark.parametrize("H,W", [(224, 224), (37, 53)])
def test_streams_in_a_batch_equal_streams_alone(device, H, W):
    B, reset_stream, reset_at = 5, 2, 17
    seqs = [make_sequence(10 + b, H, W) for b in range(B)]
    events = dict(match=0, birth=0, retire=0, recover=0, reuse=0)
    for b in range(B):                                             # CPU: the streams are not trivial
        _, ev = run_reference(seqs[b], 0.3, 2, reset_at if b == reset_stream else None)
        for k, v in ev.items():
            events[k] += v
    assert all(v > 0 for v in events.values()), events
    dev = [torch.from_numpy(s).to(device) for s in seqs]
    batch = tracking.Tracker(min_iou=0.3, max_age=2, streams=B)
    alone = [tracking.Tracker(min_iou=0.3, max_age=2) for _ in range(B)]
    for t in range(T_FRAMES):
        if t == reset_at:
            batch.reset(reset_stream)
            alone[reset_stream].reset()
        out = batch.update(torch.stack([d[t] for d in dev]))
        for b in range(B):
            o1 = alone[b].update(dev[b][t])
            assert torch.equal(out[b], o1), (t, b)
            assert torch.equal(batch.state_words[b], alone[b].state_words[0]), (t, b)
            assert torch.equal(batch.lut[b], alone[b].lut[0]) and torch.equal(batch.table[b], alone[b].table[0]), (t, b)
    # ... and the reset stream is what the reference computes with a reset at the same frame
    steps, _ = run_reference(seqs[reset_stream], 0.3, 2, reset_at)
    assert_state(batch, steps[-1], reset_stream, "batch, reset stream")
    assert batch.tracks(reset_stream)["step"] == T_FRAMES - reset_at
    batch.reset()
    assert not batch.state_words.any() and not batch.lut.any() and not batch.table.any()


@pytest.mark.parametrize("H,W", [(224, 224), (37, 53)])
def test_track_sequence_equals_updates(device, H, W):
    frames = torch.from_numpy(make_sequence(3, H, W)).to(device)
    tr = tracking.Tracker(min_iou=0.3, max_age=2)
    outs, uids = [], []
    for t in range(T_FRAMES):
        outs.append(tr.update(frames[t]))
        uids.append(tr.table[0, :, 0].clone())
    seq_out, seq_uid = tracking.track_sequence(frames, min_iou=0.3, max_age=2)
    assert seq_out.shape == (T_FRAMES, H, W) and seq_uid.shape == (T_FRAMES, 128) and seq_uid.dtype == torch.int32
    assert torch.equal(seq_out, torch.stack(outs)) and torch.equal(seq_uid, torch.stack(uids))
    # float maps, and a block continued through the same tracker
    tr2 = tracking.Tracker(min_iou=0.3, max_age=2)
    a, ua = tracking.track_sequence(frames[:15].float(), tracker=tr2)
    b, ub = tracking.track_sequence(frames[15:], tracker=tr2)
    assert torch.equal(torch.cat([a, b]), seq_out) and torch.equal(torch.cat([ua, ub]), seq_uid)
    assert torch.equal(tr2.state_words, tr.state_words) and torch.equal(tr2.table, tr.table)


def test_overflow_drops_the_128th_object(device):
    def frame(moved):
        img = np.zeros((9, 140), dtype=np.int32)
        img[1:8, 1:128] = np.arange(1, 128)[None, :]               # 127 objects, one pixel wide
        if moved:
            img[:, 127] = 0
            img[1:8, 135] = 127                                    # raw id 127 somewhere else: a 128th object
        return img
    seq = np.stack([frame(False), frame(True), frame(True), frame(True)])
    ref = ReferenceTracker(0.3, 2)
    tr = tracking.Tracker(min_iou=0.3, max_age=2)
    dropped = []
    for t in range(4):
        want = ref.step(seq[t])
        out = tr.update(torch.from_numpy(seq[t]).to(device))
        assert np.array_equal(out.cpu().numpy(), want), t
        assert_state(tr, (None, ref.lut.astype(np.int32), ref.table32(), ref.mem.astype(np.uint8), ref.meta()), 0, f"step {t}")
        dropped.append(tr.tracks()["dropped"])
    assert dropped == [0, 1, 2, 2] and ref.dropped == 2
    assert len(tr.tracks()["slot"]) == 127 and tr.tracks()["uid"].max() == 128


def test_composition_with_segmentation_and_objects(device):
    from unseenobjectclustering_amd import networks, synth
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    net = networks.seg_resnet34_8s_embedding(2, 64, sd).eval()
    fr = synth.palette_frame(1, 240, 320, 3)
    sample = dict(image_color=torch.from_numpy(fr["image_color"]), depth=torch.from_numpy(fr["depth"]))
    np.random.seed(3)
    out_label, refined, objs = O.segment_objects(sample, net, net, min_points=0)
    final = (refined if refined is not None else out_label)[0].to(device)
    present = sorted(set(torch.unique(final).cpu().tolist()) - {0.0})
    assert len(present) >= 2
    permuted = torch.where(final > 0, (final * 5) % 127 + 1, final)          # a bijection of 1..127
    assert not torch.equal(permuted, final)
    tr = tracking.Tracker()
    a = tr.update(final)
    b = tr.update(permuted)
    assert torch.equal(a, b) and torch.equal((a > 0), (final > 0))
    live = tr.tracks()
    assert live["slot"].tolist() == list(range(1, len(present) + 1)) and live["uid"].tolist() == live["slot"].tolist()
    assert (live["hits"] == 2).all() and (live["age"] == 0).all()
    tracked_objs = O.extract_objects(a, sample["depth"].to(device), min_points=0)
    assert tracked_objs.label.cpu().tolist() == live["slot"].tolist()
    assert tracked_objs.pixels.cpu().tolist() == live["area"].tolist()
    assert sorted(tracked_objs.pixels.cpu().tolist()) == sorted(objs.pixels.cpu().tolist())
