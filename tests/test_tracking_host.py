"""Object tracking without a GPU: the plain-integer reference (tests/tracking_reference.py) pinned by hand-made known
answers, so that the GPU comparison in tests/test_tracking_gpu.py is not merely "whatever the kernel does"; the
validation of the C ABI before any HIP call; and the refusal of CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tracking_cases as TC
from tests.tracking_cases import line
from tests.tracking_reference import ReferenceTracker, iou_threshold, object_ids
from unseenobjectclustering_amd import _native, tracking


def canvas(H=24, W=32):
    return np.zeros((H, W), dtype=np.int32)


def rect(img, y0, x0, h, w, val):
    img[y0:y0 + h, x0:x0 + w] = val
    return img


def live(tr):
    return {s: int(tr.table[s, 0]) for s in range(128) if tr.table[s, 0]}


def test_threshold_is_rounded_once_on_the_host():
    assert iou_threshold(0.3) == 19661 == tracking.iou_threshold(0.3)
    assert iou_threshold(1.0) == 65536 == tracking.iou_threshold(1.0)
    assert iou_threshold(1e-9) == 1 == tracking.iou_threshold(1e-9)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            tracking.iou_threshold(bad)
    with pytest.raises(ValueError):
        tracking.Tracker(max_age=-1)
    with pytest.raises(ValueError):
        tracking.Tracker(streams=0)


def test_first_step_numbers_present_ids_in_ascending_order():
    tr = ReferenceTracker()
    img = rect(rect(rect(canvas(), 1, 1, 4, 4, 9), 10, 10, 5, 5, 3), 1, 20, 3, 3, 100)
    out = tr.step(img)
    assert out.dtype == np.int32
    assert np.array_equal(out, rect(rect(rect(canvas(), 1, 1, 4, 4, 2), 10, 10, 5, 5, 1), 1, 20, 3, 3, 3))
    assert tr.lut[3] == 1 and tr.lut[9] == 2 and tr.lut[100] == 3 and tr.lut.sum() == 6
    assert tr.table[1].tolist() == [1, 0, 1, 25, 0] and tr.table[2].tolist() == [2, 0, 1, 16, 0]
    assert tr.table[3].tolist() == [3, 0, 1, 9, 0] and not tr.table[4:].any() and not tr.table[0].any()
    assert tr.meta() == dict(next_uid=4, step=1, dropped=0)
    assert np.array_equal(tr.mem, out)


def test_swapping_raw_ids_keep_slots_and_uids():
    tr = ReferenceTracker(min_iou=0.3, max_age=5)
    for f in range(8):
        a, b = (1, 2) if f % 2 == 0 else (2, 1)
        img = rect(rect(canvas(), 2, 2 + f, 6, 6, a), 12, 20 - f, 6, 8, b)      # both drift one pixel per frame
        out = tr.step(img)
        assert np.array_equal(out, rect(rect(canvas(), 2, 2 + f, 6, 6, 1), 12, 20 - f, 6, 8, 2)), f
        assert live(tr) == {1: 1, 2: 2}
        assert tr.table[1].tolist() == [1, 0, f + 1, 36, 0] and tr.table[2].tolist() == [2, 0, f + 1, 48, 0]
        assert np.array_equal(tr.mem, out)                                      # stale pixels of a matched track vanish
    assert tr.meta() == dict(next_uid=3, step=8, dropped=0)
    assert tr.events == dict(match=14, birth=0, retire=0, recover=0, reuse=0)


@pytest.mark.parametrize("max_age", [0, 1, 3])
def test_occlusion_up_to_max_age_keeps_the_uid_and_one_more_frame_loses_it(max_age):
    def frame(with_a, ax=2):
        img = rect(canvas(), 14, 20, 5, 5, 7)                                   # B is always there
        return rect(img, 2, ax, 6, 6, 4) if with_a else img

    # hidden for exactly max_age frames: the same slot and uid come back
    tr = ReferenceTracker(max_age=max_age)
    tr.step(frame(True))
    assert live(tr) == {1: 1, 2: 2}
    for k in range(max_age):
        out = tr.step(frame(False))
        assert live(tr) == {1: 1, 2: 2} and tr.table[1, 1] == k + 1 and not (out == 1).any()
        assert np.array_equal(tr.mem == 1, frame(True) == 4)                    # the footprint waits in the memory map
    out = tr.step(frame(True, ax=3))
    assert np.array_equal(out == 1, frame(True, ax=3) == 4) and live(tr) == {1: 1, 2: 2}
    assert tr.table[1].tolist() == [1, 0, 2, 36, 0] and tr.meta()["next_uid"] == 3
    assert np.array_equal(tr.mem, out)
    assert tr.events["recover"] == (1 if max_age else 0)

    # hidden for max_age + 1 frames: retired, returns as a new object in the lowest free slot, which inherits nothing
    tr = ReferenceTracker(max_age=max_age)
    tr.step(frame(True))
    for k in range(max_age + 1):
        tr.step(frame(False))
    assert live(tr) == {2: 2} and not tr.table[1].any() and not (tr.mem == 1).any()
    out = tr.step(frame(True, ax=5))
    assert live(tr) == {1: 3, 2: 2}
    assert tr.table[1].tolist() == [3, 0, 1, 36, max_age + 2]
    assert np.array_equal(out == 1, frame(True, ax=5) == 4) and np.array_equal(tr.mem == 1, out == 1)
    assert tr.events["retire"] == 1 and tr.events["reuse"] == 1 and tr.events["birth"] == 1


def begin(c):
    """A fresh reference tracker with the case's parameters, and the case's frames (tests/tracking_cases.py)."""
    return ReferenceTracker(min_iou=c["min_iou"], max_age=c["max_age"]), c["frames"]


def test_exact_iou_ties_go_to_larger_intersection_then_lower_track_then_lower_id():
    # larger intersection: track 1 has 6 pixels; id 5 (2 px, all inside: 2/6) and id 9 (10 px, 4 inside: 4/12) tie at 1/3
    tr, frames = begin(TC.tie_larger_inter())
    tr.step(frames[0])
    out = tr.step(frames[1])
    assert tr.lut[9] == 1 and tr.lut[5] == 2
    assert tr.table[1].tolist() == [1, 0, 2, 10, 0] and tr.table[2].tolist() == [2, 0, 1, 2, 1]
    assert np.array_equal(out, line(40, (10, 12, 2), (12, 22, 1)))
    # lower track: tracks 1 and 2 (4 px each) against one id covering the inner halves of both (2/6 each, equal inter)
    tr, frames = begin(TC.tie_lower_track())
    tr.step(frames[0])
    assert live(tr) == {1: 1, 2: 2}
    out = tr.step(frames[1])
    assert tr.lut[6] == 1 and tr.table[1].tolist() == [1, 0, 2, 4, 0] and tr.table[2].tolist() == [2, 1, 1, 4, 0]
    assert np.array_equal(tr.mem, line(40, (12, 16, 1), (16, 18, 2)))      # track 2 keeps what was not covered
    # lower id: one track (8 px) against ids 4 and 7, each 2 px inside plus 2 outside (2/10 each)
    tr, frames = begin(TC.tie_lower_id())
    tr.step(frames[0])
    out = tr.step(frames[1])
    assert tr.lut[4] == 1 and tr.lut[7] == 2
    assert np.array_equal(out, line(40, (8, 12, 2), (16, 20, 1)))
    assert np.array_equal(tr.mem, out)                                      # a matched track's stale pixels vanish


def test_threshold_is_inclusive_and_exact():
    q = iou_threshold(0.3)
    assert q == 19661
    # the id covers 65536 pixels, the track's pixels all lie inside: IoU = area_track / 65536
    for area, matched, c in ((q, True, TC.threshold_equal_large()), (q - 1, False, TC.threshold_equal_large_miss())):
        tr, frames = begin(c)
        assert tr.q == q and frames.shape == (2, 1, 70000) and (frames[0] == 1).sum() == area and (frames[1] == 1).sum() == 65536
        tr.step(frames[0])
        tr.step(frames[1])
        assert (tr.table[1, 0] == 1 and tr.table[1, 2] == 2) == matched
        assert (tr.table[2, 0] == 2) == (not matched)
    # one half exactly, and just under it
    for inter, matched in ((2, True),):
        tr, frames = begin(TC.threshold_half_line())
        assert tr.q == 32768
        tr.step(frames[0])
        tr.step(frames[1])                                                     # inter 2, union 4
        assert (tr.meta()["next_uid"] == 2) == matched
    tr, frames = begin(TC.threshold_below_half())
    assert tr.q == 32768
    tr.step(frames[0])
    tr.step(frames[1])                                                         # inter 66, union 134
    assert tr.meta()["next_uid"] == 3 and live(tr) == {1: 1, 2: 2} and tr.table[1, 1] == 1


def test_values_outside_1_to_127_are_background():
    raw = np.array([[0, -1, 128, 255, 1, 127, -128, 1 << 20]], dtype=np.int64)
    assert object_ids(raw).tolist() == [[0, 0, 0, 0, 1, 127, 0, 0]]
    assert object_ids(np.array([[0.0, 1.0, 127.0, 128.0, -3.0, np.nan]], dtype=np.float32)).tolist() == [[0, 1, 127, 0, 0, 0]]
    tr = ReferenceTracker()
    out = tr.step(raw)
    assert out.tolist() == [[0, 0, 0, 0, 1, 2, 0, 0]] and live(tr) == {1: 1, 2: 2}


def test_a_128th_object_is_dropped():
    tr, frames = begin(TC.overflow_128th())                                    # raw id 127 shows up somewhere else

    def frame(moved):
        return frames[1 if moved else 0]
    assert tr.max_age == 2 and np.array_equal(frames[2], frames[1]) and np.array_equal(frames[3], frames[1])
    out = tr.step(frame(False))
    assert np.array_equal(out, frame(False)) and len(live(tr)) == 127 and tr.dropped == 0
    out = tr.step(frame(True))
    assert tr.dropped == 1 and out[2, 5] == 0 and tr.lut[127] == 0 and tr.meta()["next_uid"] == 128
    assert np.array_equal(out[0, 1:127], np.arange(1, 127)) and out[0, 127] == 0
    assert tr.table[127].tolist() == [127, 1, 1, 1, 0] and tr.mem[0, 127] == 127  # the occluded track keeps its pixel
    tr.step(frame(True))
    assert tr.dropped == 2
    out = tr.step(frame(True))                                                 # track 127 retires; its slot is free in this very step
    assert tr.dropped == 2 and out[2, 5] == 127 and tr.table[127].tolist() == [128, 0, 1, 1, 3]
    assert tr.mem[0, 127] == 0


# ---- C ABI: validation before any HIP call -------------------------------------------------------------------------------
def last_error():
    return _native.lib().uoc_last_error().decode().lower()


def test_state_and_workspace_sizes():
    lib = _native.lib()
    a = lib.uoc_track_state_bytes(1, 480, 640)
    assert a >= 480 * 640 * 4 + 128 * 5 * 4
    assert lib.uoc_track_state_bytes(2, 480, 640) == 2 * a
    assert lib.uoc_track_state_bytes(12, 480, 640) == 12 * a
    assert lib.uoc_track_state_bytes(1, 224, 224) < a < lib.uoc_track_state_bytes(1, 960, 1280)
    assert lib.uoc_track_state_bytes(1, 37, 53) > 37 * 53 * 4
    for bad in ((0, 480, 640), (1, 0, 640), (1, 480, -1), (1, 65536, 32768)):
        assert lib.uoc_track_state_bytes(*bad) == 0
    assert lib.uoc_track_workspace_bytes(5) > lib.uoc_track_workspace_bytes(1) > 0 == lib.uoc_track_workspace_bytes(0)
    assert ctypes.sizeof(_native.UocTrack) == 20 and _native.TRACK_FIELDS == ("uid", "age", "hits", "area", "born")


def test_step_and_reset_validate_without_a_device():
    lib = _native.lib()
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its validation first
    ws = lib.uoc_track_workspace_bytes(2)

    def step(labels=p, B=2, H=48, W=64, q=19661, max_age=5, state=p, out=p, lut=None, tracks=None, d_ws=p, nws=ws):
        return lib.uoc_track_step(labels, B, H, W, q, max_age, state, out, lut, tracks, d_ws, nws, None)

    for kw in (dict(labels=None), dict(state=None), dict(out=None), dict(d_ws=None)):
        assert step(**kw) == -22 and "null" in last_error(), kw
    for kw in (dict(B=0), dict(H=0), dict(W=-3)):
        assert step(**kw) == -22 and "shape" in last_error(), kw
    assert step(H=65536, W=32768) == -22 and "31 bits" in last_error()
    for q in (0, -1, 65537):
        assert step(q=q) == -22 and "q =" in last_error()
    assert step(max_age=-1) == -22 and "max_age" in last_error()
    assert step(nws=ws - 1) == -22 and "workspace" in last_error()
    assert step(state=ctypes.c_void_p((1 << 20) + 4)) == -22 and "aligned" in last_error()

    assert lib.uoc_track_reset(None, 1, 48, 64, -1, None) == -22 and "null" in last_error()
    assert lib.uoc_track_reset(p, 0, 48, 64, -1, None) == -22 and "shape" in last_error()
    assert lib.uoc_track_reset(p, 1, 65536, 32768, -1, None) == -22 and "31 bits" in last_error()
    for which in (-2, 3):
        assert lib.uoc_track_reset(p, 3, 48, 64, which, None) == -22 and "stream" in last_error()


def test_cpu_tensors_are_refused():
    tr = tracking.Tracker()
    with pytest.raises(_native.NativeError):
        tr.update(torch.zeros(8, 8, dtype=torch.int32))
    with pytest.raises(_native.NativeError):
        tr.update(np.zeros((8, 8), dtype=np.int32))
    with pytest.raises(_native.NativeError):
        tracking.track_sequence(torch.zeros(3, 8, 8, dtype=torch.int32))
    assert tr.tracks()["slot"].size == 0 and tr.tracks()["next_uid"] == 1 and tr.lut is None
