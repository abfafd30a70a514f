"""Re-identification on the GPU, bit for bit against the plain-integer reference (tests/identity_reference.py): signatures
and similarities at shapes on both pixel paths, every case of tests/identity_cases.py through uoc_ident_step with the
whole state compared after every step, the generated sequences end to end through Tracker and Identifier against both
references, a three-stream batch against each stream alone, and two calls in a row giving the same bits (the vote
accumulators are left zero).  tests/test_identity_cases_host.py proves on the CPU that the cases and sequences contain
what they are for.

Every test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)); nothing is retried."""
import faulthandler
import functools
import sys

import numpy as np
import pytest
import torch

from tests import identity_cases as IC
from tests import identity_reference as ir
from unseenobjectclustering_amd import _native, identity, tracking

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- signatures -----------------------------------------------------------------------------------------------------------
def scene(seed, H, W):
    """Rectangles of flat colour plus noise on a noisy table; ids 1, 127 and others, 128 and -1 as background; depths that
    are valid, zero, NaN, negative and beyond 65 m."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), dtype=np.int32)
    img = rng.integers(60, 120, size=(H, W, 3))
    for k, rid in enumerate([1, 127, 5, 64, 128, -1, 77]):
        h, w = max(1, H // 3), max(1, W // 4)
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        lab[y0:y0 + h, x0:x0 + w] = rid
        img[y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, size=3) if k != 3 else (5, 6, 7)       # id 64 is dark
        if k % 2:
            img[y0:y0 + h, x0:x0 + w] += rng.integers(-8, 9, size=(h, w, 3))
    z = rng.uniform(0.3, 3.0, size=(H, W)).astype(np.float32)
    bad = rng.integers(0, 12, size=(H, W))
    for code, value in ((0, 0.0), (1, np.nan), (2, -0.5), (3, 65.5), (4, 65.0)):
        z[bad == code] = value
    xyz = np.stack([rng.normal(size=(H, W)), rng.normal(size=(H, W)), z]).astype(np.float32)
    return lab, np.clip(img, 0, 255).astype(np.uint8), xyz


SHAPES = [(5, 13), (2, 64), (4, 64), (37, 53), (96, 96), (224, 224), (480, 640)]


@functools.lru_cache(maxsize=None)
def scenes(H, W):
    frames = [scene(1000 * H + W + k, H, W) for k in range(1 if H * W > 100000 else 2)]
    return frames, [ir.describe(*f) for f in frames]


@pytest.mark.parametrize("H,W", SHAPES)
def test_describe_and_similarity_equal_the_reference(device, H, W):
    frames, want = scenes(H, W)
    lab = torch.from_numpy(np.stack([f[0] for f in frames])).to(device)
    img = torch.from_numpy(np.stack([f[1] for f in frames])).to(device)
    xyz = torch.from_numpy(np.stack([f[2] for f in frames])).to(device)
    got = identity.describe(lab, img, xyz)
    ref = torch.from_numpy(np.stack(want)).to(device)
    assert got.sig.dtype == torch.int32 and torch.equal(got.sig, ref)
    assert torch.equal(got.pixels, ref[..., 0]) and torch.equal(got.valid, ref[..., 1]) and tuple(got.hist.shape) == (len(frames), 128, 91)
    assert got.area[0, 1].item() == ir.area_of(want[0][1]) and (got.valid[0] > 0).any()
    bare = identity.describe(lab, img)                                  # without xyz: the same but valid and area
    ref_bare = ref.clone()
    ref_bare[..., 1:4] = 0
    assert torch.equal(bare.sig, ref_bare)
    if H * W % 4 == 0:
        assert H * W % 4 == 0 and lab.data_ptr() % 16 == 0             # these shapes take the int4 path
    again = identity.describe(lab, img, xyz)                            # the accumulators were left zero
    assert torch.equal(again.sig, ref)
    other = torch.roll(ref, 1, dims=0) if len(frames) > 1 else ref.flip(1).contiguous()
    sim = identity.similarity(got, other)
    want_sim = np.stack([ir.similarity_table(a, b) for a, b in zip(ref.cpu().numpy(), other.cpu().numpy())])
    assert sim.dtype == torch.int32 and np.array_equal(sim.cpu().numpy(), want_sim)
    self_sim = identity.similarity(got, got).cpu().numpy()
    present = want[0][:, 0] > 0
    assert (np.diag(self_sim[0])[present] >= 65536 - 91).all() and not np.diag(self_sim[0])[~present].any()


@pytest.mark.parametrize("case", IC.SIGNATURE_CASES, ids=lambda c: c.name)
def test_signature_case(device, case):
    want = ir.describe(case.labels, case.image, case.xyz)
    case.claim(want)
    xyz = None if case.xyz is None else torch.from_numpy(case.xyz).to(device)
    got = identity.describe(torch.from_numpy(case.labels).to(device), torch.from_numpy(case.image).to(device), xyz)
    assert np.array_equal(got.sig[0].cpu().numpy(), want)
    case.claim(got.sig[0].cpu().numpy())


def test_labels_at_a_4_byte_offset_take_the_scalar_path(device):
    (lab, img, xyz), want = scenes(4, 64)[0][0], scenes(4, 64)[1][0]
    lib = _native.lib()
    n = lab.size
    buf = torch.zeros(n + 8, dtype=torch.int32, device=device)
    shifted = buf[1:1 + n]
    shifted.copy_(torch.from_numpy(lab.reshape(-1)).to(device))
    assert _native.ptr(buf).value % 16 == 0 and _native.ptr(shifted).value % 16 == 4
    acc = torch.zeros(lib.uoc_signature_workspace_bytes(1), dtype=torch.uint8, device=device)
    sig = torch.empty((128, 104), dtype=torch.int32, device=device)
    _native.call("uoc_signature", device, shifted, torch.from_numpy(img).to(device), torch.from_numpy(xyz).to(device), 1, 4, 64, sig,
                 acc, acc.numel())
    assert np.array_equal(sig.cpu().numpy(), want) and not acc.any()
    assert not buf[:1].any() and not buf[1 + n:].any()


def test_two_calls_in_a_row_give_the_same_bits(device):
    frames, want = scenes(96, 96)
    a, b = ([torch.from_numpy(x).to(device) for x in f] for f in frames)
    first = identity.describe(*a).sig.clone()
    assert torch.equal(identity.describe(*a).sig, first)
    second = identity.describe(*b).sig.clone()
    assert torch.equal(identity.describe(*a).sig, first) and not torch.equal(first, second)
    assert np.array_equal(first[0].cpu().numpy(), want[0]) and np.array_equal(second[0].cpu().numpy(), want[1])
    assert all(not acc.any() for acc in identity._acc.of_device(device))


# ---- identity steps --------------------------------------------------------------------------------------------------------
ALL_IDS = np.arange(-2, 130, dtype=np.int32).reshape(2, 66)           # a map holding every id once, and four non-ids


@functools.lru_cache(maxsize=None)
def reference(name):
    case = next(c for c in IC.STEP_CASES if c.name == name)
    run = case.run()
    case.claim(run)
    return case, run


@pytest.mark.parametrize("name", [c.name for c in IC.STEP_CASES])
def test_step_case_matches_reference_at_every_step(device, name):
    case, run = reference(name)
    ident = identity.Identifier()
    ident.q, ident.r, ident.max_lost = case.q, case.r, case.max_lost
    words = ident.allocate(device, *ALL_IDS.shape)
    words[0].copy_(torch.from_numpy(case.initial_words()).to(device))
    tracked = torch.from_numpy(ALL_IDS[None]).to(device)
    got = []
    for t, (tracks, sig) in enumerate(case.steps):
        out = ident.step_tables(torch.from_numpy(tracks[None]).to(device), torch.from_numpy(sig[None]).to(device), tracked)
        where = f"{name} step {t}"
        lut = ident.lut[0].cpu().numpy()
        assert np.array_equal(lut, run[t]["lut"]), where
        assert np.array_equal(out[0].cpu().numpy(), run[t]["lut"][ir.object_ids(ALL_IDS)]), where
        assert np.array_equal(ident.table[0].cpu().numpy(), run[t]["table"]), where
        assert np.array_equal(ident.state_words[0].cpu().numpy(), run[t]["words"]), where
        rec = ident.identities()
        assert (rec["next_pid"], rec["step"], rec["evicted"]) == (run[t]["pids"] + 1, run[t]["step"], run[t]["evicted"]), where
        got.append(dict(lut=lut, table=ident.table[0].cpu().numpy(), words=ident.state_words[0].cpu().numpy(), pids=rec["next_pid"] - 1,
                        step=rec["step"], evicted=rec["evicted"]))
    case.claim(got)


def test_lut_and_table_outputs_are_optional(device):
    """uoc_ident_step without its lut and table outputs steps the same state and writes the same map."""
    case, run = reference("forget_boundary_and_reuse")
    lib = _native.lib()
    state = torch.from_numpy(case.initial_words()).to(device)
    ws = torch.empty(lib.uoc_ident_workspace_bytes(1), dtype=torch.uint8, device=device)
    tracks, sig = (torch.from_numpy(x).to(device) for x in case.steps[0])
    tracked = torch.from_numpy(ALL_IDS).to(device)
    out = torch.empty_like(tracked)
    _native.call("uoc_ident_step", device, tracked, tracks, sig, 1, ALL_IDS.shape[0], ALL_IDS.shape[1], case.q, case.r, case.max_lost, state,
                 out, None, None, ws, ws.numel())
    assert np.array_equal(state.cpu().numpy(), run[0]["words"])
    assert np.array_equal(out.cpu().numpy(), run[0]["lut"][ir.object_ids(ALL_IDS)])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sequence(name):
    seq = next(make for make in IC.SEQUENCES if make.__name__ == name)()
    frames, ref = IC.run_reference(seq)
    return seq, frames, ref


def device_frames(seq, device):
    return [tuple(torch.from_numpy(x).to(device) for x in f) for f in seq.frames]


@pytest.mark.parametrize("name", [make.__name__ for make in IC.SEQUENCES])
def test_sequence_end_to_end_matches_both_references(device, name):
    seq, frames, ref = sequence(name)
    tracker, ident = tracking.Tracker(**seq.tracker), identity.Identifier(**seq.ident)
    for t, (lab, img, xyz) in enumerate(device_frames(seq, device)):
        tracked = tracker.update(lab)
        out = ident.update(tracked, tracker, img, xyz)
        where = f"{name} frame {t}"
        assert np.array_equal(tracked.cpu().numpy(), frames[t]["tracked"]), where
        assert np.array_equal(tracker.table[0].cpu().numpy(), frames[t]["tracks"]), where
        assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), frames[t]["out"]), where
        assert np.array_equal(ident.lut[0].cpu().numpy(), frames[t]["lut"]), where
        assert np.array_equal(ident.state_words[0].cpu().numpy(), frames[t]["words"]), where
    rec = ident.identities()
    assert (rec["next_pid"] - 1, rec["step"], rec["evicted"]) == (ref.pids, ref.step_index, ref.evicted)
    assert np.array_equal(rec["pid"], ref.table[rec["entry"], 0]) and np.array_equal(rec["pixels"], ref.table[rec["entry"], 4])
    ident.reset()
    assert not ident.state_words.any() and not ident.lut.any() and not ident.table.any()


def test_three_streams_equal_their_single_runs(device):
    """The tabletop sequence, its mirror image and the same with blue and red swapped: one batch against three runs."""
    seq, frames, _ = sequence("tabletop_sequence")
    base = device_frames(seq, device)
    streams = [base, [(l.flip(1).contiguous(), i.flip(1).contiguous(), x.flip(2).contiguous()) for l, i, x in base],
               [(l, i.flip(2).contiguous(), x) for l, i, x in base]]
    batch_t, batch_i = tracking.Tracker(streams=3, **seq.tracker), identity.Identifier(streams=3, **seq.ident)
    alone = [(tracking.Tracker(**seq.tracker), identity.Identifier(**seq.ident)) for _ in range(3)]
    for t in range(len(base)):
        lab, img, xyz = (torch.stack([s[t][k] for s in streams]) for k in range(3))
        tracked = batch_t.update(lab)
        out = batch_i.update(tracked, batch_t, img, xyz)
        for b, (tr, idn) in enumerate(alone):
            one = idn.update(tr.update(streams[b][t][0]), tr, streams[b][t][1], streams[b][t][2])
            assert torch.equal(out[b], one), (t, b)
            assert torch.equal(batch_i.state_words[b], idn.state_words[0]), (t, b)
            assert torch.equal(batch_i.lut[b], idn.lut[0]) and torch.equal(batch_i.table[b], idn.table[0]), (t, b)
        assert np.array_equal(out[0].cpu().numpy(), frames[t]["out"]), t
    assert not torch.equal(batch_i.state_words[0], batch_i.state_words[2])
    batch_i.reset(1)
    assert not batch_i.state_words[1].any() and torch.equal(batch_i.state_words[0], alone[0][1].state_words[0])
