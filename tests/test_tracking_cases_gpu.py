"""The engineered tracker sequences (tests/tracking_cases.py) on the GPU, bit for bit against the plain-integer reference:
exact IoU ties over every lane and row of the wave's arg-max, exact threshold equality, products that need 64 bits, births
whose ranks cross the wave boundary, maps of fewer than 64 pixels, junk values; the three-stream batch; and the raw C entry
with a label pointer that is 4-byte but not 16-byte aligned, and without the optional outputs.
tests/test_tracking_cases_host.py proves on the CPU that each case contains what it is for.

Every test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)); nothing is retried."""
import faulthandler
import functools
import sys

import numpy as np
import pytest
import torch

from tests import tracking_cases as TC
from tests.test_tracking_gpu import assert_state
from tests.tracking_reference import iou_threshold
from unseenobjectclustering_amd import _native, tracking

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def reference(name):
    c = TC.CASES[name]()
    run, _ = TC.run_case(c)
    c["claim"](run)
    return c, run


@pytest.mark.parametrize("name", list(TC.CASES))
def test_case_matches_reference_at_every_step(device, name):
    c, run = reference(name)
    frames = torch.from_numpy(c["frames"]).to(device)
    tr = tracking.Tracker(min_iou=c["min_iou"], max_age=c["max_age"])
    for t in range(frames.shape[0]):
        out = tr.update(frames[t])
        where = f"{name} step {t}"
        assert out.dtype == torch.int32 and out.shape == frames.shape[1:]
        assert np.array_equal(out.cpu().numpy(), run[t][0].astype(np.int32)), where
        assert_state(tr, run[t], 0, where)


def test_three_streams_equal_their_single_runs(device):
    """Streams 1 and 2 are the domino and the births across the wave boundary; stream 0 is the domino mirrored, another
    sequence of the same shape.  Parameters are per tracker, so all three run at the births' max_age 0."""
    domino, births = TC.tie_domino()["frames"], TC.births_across_waves()["frames"]
    seqs = [np.ascontiguousarray(domino[:, :, ::-1]), domino, births]
    assert domino.shape == births.shape == (2, 1, TC.DOMINO_W) and not np.array_equal(seqs[0], seqs[1])
    dev = [torch.from_numpy(s).to(device) for s in seqs]
    batch = tracking.Tracker(min_iou=0.3, max_age=0, streams=3)
    alone = [tracking.Tracker(min_iou=0.3, max_age=0) for _ in range(3)]
    refs = [TC.run_case(dict(frames=s, min_iou=0.3, max_age=0))[0] for s in seqs]
    for t in range(2):
        out = batch.update(torch.stack([d[t] for d in dev]))
        for b in range(3):
            o1 = alone[b].update(dev[b][t])
            assert torch.equal(out[b], o1), (t, b)
            assert torch.equal(batch.state_words[b], alone[b].state_words[0]), (t, b)
            assert torch.equal(batch.lut[b], alone[b].lut[0]) and torch.equal(batch.table[b], alone[b].table[0]), (t, b)
            assert np.array_equal(out[b].cpu().numpy(), refs[b][t][0].astype(np.int32)), (t, b)
            assert_state(batch, refs[b][t], b, f"batch stream {b} step {t}")
    TC.births_across_waves()["claim"](refs[2])


def raw_run(device, c, label_offset=0, outputs=True):
    """The frames of a case through uoc_track_step itself.  label_offset: int32 words between a 16-byte aligned address and
    the labels.  Returns per step (out, state words, lut or None, tracks or None) as host arrays."""
    lib = _native.lib()
    frames = c["frames"]
    T, H, W = frames.shape
    n = H * W
    state = torch.zeros(lib.uoc_track_state_bytes(1, H, W), dtype=torch.uint8, device=device)
    ws = torch.empty(max(lib.uoc_track_workspace_bytes(1), 16), dtype=torch.uint8, device=device)
    buf = torch.zeros(n + 8, dtype=torch.int32, device=device)
    lab = buf[label_offset:label_offset + n]
    out = torch.empty(n, dtype=torch.int32, device=device)
    lut = torch.zeros(128, dtype=torch.int32, device=device) if outputs else None
    tracks = torch.zeros((128, 5), dtype=torch.int32, device=device) if outputs else None
    assert _native.ptr(buf).value % 16 == 0 and _native.ptr(out).value % 16 == 0 and _native.ptr(state).value % 16 == 0
    assert _native.ptr(lab).value % 16 == 4 * label_offset
    steps = []
    for t in range(T):
        lab.copy_(torch.from_numpy(frames[t].reshape(-1)).to(device))
        _native.call("uoc_track_step", device, lab, 1, H, W, iou_threshold(c["min_iou"]), c["max_age"], state, out, lut, tracks, ws, ws.numel())
        steps.append((out.cpu().numpy().reshape(H, W), state.view(torch.int32).cpu().numpy(),
                      lut.cpu().numpy() if outputs else None, tracks.cpu().numpy() if outputs else None))
    assert not buf[:label_offset].any() and not buf[label_offset + n:].any()
    return steps


@pytest.mark.parametrize("name", ["tie_domino", "products_need_64_bits"])
def test_labels_at_a_4_byte_offset_take_the_scalar_path(device, name):
    c, run = reference(name)
    assert c["frames"].shape[1] * c["frames"].shape[2] % 4 == 0        # only the pointer keeps it off the int4 path
    aligned, shifted = raw_run(device, c, 0), raw_run(device, c, 1)
    for t, (a, s) in enumerate(zip(aligned, shifted)):
        assert all(np.array_equal(x, y) for x, y in zip(a, s)), t
        assert np.array_equal(a[0], run[t][0].astype(np.int32)) and np.array_equal(a[2], run[t][1]), t
        assert np.array_equal(a[3], run[t][2]) and np.array_equal(a[1][:128 * 5].reshape(128, 5), run[t][2]), t


def test_lut_and_tracks_are_optional(device):
    c, run = reference("births_overflow")
    full, bare = raw_run(device, c), raw_run(device, c, outputs=False)
    for t, (a, s) in enumerate(zip(full, bare)):
        assert s[2] is None and s[3] is None
        assert np.array_equal(a[0], s[0]) and np.array_equal(a[1], s[1]), t
        assert np.array_equal(s[0], run[t][0].astype(np.int32)) and np.array_equal(s[1][:128 * 5].reshape(128, 5), run[t][2]), t
