"""What include/uoc_hip.h promises about caller-supplied scratch and state, on a call that succeeds, for every entry point
that takes either (the table of tests/workspace_cases.py; tests/test_workspace_contract_host.py holds it to the header):

  (a) content    the scratch pre-filled 0x00, then 0xFF, then 0x55: all outputs bit-identical, and the 0x00 run passes the
                 stage's own reference comparison.  uoc_signature, whose scratch has a stated precondition (all zero before,
                 all zero after), runs three different maps on one zeroed buffer, which is all zero after each
  (b) extent     the scratch is a view of exactly the size function's value inside a larger allocation whose canaries are
                 intact after every run (tests/scratch_guard.py)
  (c) alignment  the 0x55 run again with the view at base + 16 (base + 256 where the entry asks for 256-byte alignment):
                 the same bits
  (d) state      uoc_track_*, uoc_ident_*, uoc_scene_*: a state filled 0xFF or 0x55 and reset steps exactly as an all-zero
                 one, a reset of stream 1 leaves stream 0's words alone, and the optional outputs the wrappers allocate with
                 torch.zeros are written in every word

profiles/workspace_regions.md records which launch writes and reads which region of every carve: it was read before this
file first ran, because a kernel that took an unwritten scratch word for an index would fault under the poison."""
import faulthandler
import sys

import numpy as np
import pytest
import torch

from tests import scratch_guard as SG
from tests import workspace_cases as WC

pytestmark = pytest.mark.gpu

SCRATCH = [name for name, case in WC.CASES.items() if case.kind != "state"]
RUNS = [(0x00, False), (0xFF, False), (0x55, False), (0x55, True)]      # (fill, view shifted off the allocator's alignment)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def record(device, case, fill, shifted):
    if case.align == 16:
        return SG.Record(device, fill, 16 if shifted else 0)
    return SG.Record(device, fill, 256 if shifted else 0, align=512)       # 256- but not 512-byte aligned


def same_bits(a, b, where):
    assert sorted(a) == sorted(b), where
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (where, k, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            diff = np.flatnonzero(np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8))
            raise AssertionError(f"{where}: output {k} differs in {diff.size} bytes, the first at byte {int(diff[0])}")


@pytest.mark.parametrize("entry", SCRATCH)
def test_scratch_content_extent_and_alignment(device, entry):
    case = WC.CASES[entry]
    runs = RUNS if case.kind == "scratch" else [(0x00, False), (0x00, True)]      # "signature": the precondition is all zero
    for shape in case.shapes:
        first = None
        for fill, shifted in runs:
            where = f"{entry} {shape} fill 0x{fill:02x}" + (" shifted" if shifted else "")
            rec = record(device, case, fill, shifted)
            bits, raw = case.run(device, shape, rec)
            torch.cuda.synchronize(device)
            assert rec.items, where + ": no guarded buffer reached the entry"
            assert all(g.address % rec.align == rec.offset and g.buf.device.type == "cuda" for g in rec.items), where
            print(where, rec.table())
            rec.check()                                                 # (b)
            if first is None:
                case.check(shape, bits, raw)                            # (a): the fresh-allocation run against the reference
                first = bits
            else:
                same_bits(first, bits, where)                           # (a) under poison, (c) off the allocator's alignment


# ---- (d) persistent state ------------------------------------------------------------------------------------------------
class Stream:
    """One state stage on the device: the guarded state, and steps whose scratch is guarded too."""

    def __init__(self, device, stage, fill):
        self.device, self.stage = device, stage
        self.rec = SG.Record(device, 0x55)
        n = int(getattr(WC._native.lib(), stage.state_size)(*stage.size_args()))
        self.state = self.rec.take(stage.state_size, n, fill)
        self.per = stage.stream_bytes()
        assert n == WC.B * self.per

    def step(self, inputs, out_fill):
        out = self.stage.step(self.device, self.state, inputs, self.rec, out_fill)
        torch.cuda.synchronize(self.device)
        self.rec.check()
        return out

    def words(self, b=None):
        w = self.state.cpu().numpy().view(np.int32).reshape(WC.B, -1)
        return w if b is None else w[b]


def run_sequence(device, stage, fill, reset, out_fill):
    """Three steps of both streams from a state filled `fill` (and reset when `reset`) -> (outputs per step, state after
    every step)."""
    s = Stream(device, stage, fill)
    if reset:
        stage.reset(device, s.state, -1)
    outs, states = [], []
    for t in range(3):
        outs.append(s.step([stage.frames[b][t] for b in range(WC.B)], out_fill))
        states.append(s.words().copy())
    return outs, states


@pytest.mark.parametrize("entry", sorted(WC.STATE_STAGES))
def test_state_reset_and_optional_outputs(device, entry):
    stage = WC.STATE_STAGES[entry]()
    base_outs, base_states = run_sequence(device, stage, 0x00, False, 0)        # what a torch.zeros state does
    assert any(w.any() for w in base_states) and set(stage.optional) <= set(base_outs[0])
    for fill in (0xFF, 0x55):                                                   # which = -1 on a poisoned state
        outs, states = run_sequence(device, stage, fill, True, -1 if stage.optional else 0)
        for t in range(3):
            same_bits(base_outs[t], outs[t], f"{entry} fill 0x{fill:02x} step {t}")      # the optional outputs too: every word written
            assert np.array_equal(base_states[t], states[t]), (entry, fill, t, "state")
    for fill in (0xFF, 0x55):                                                   # which = 1 with stream 0 left running
        s = Stream(device, stage, 0x00)
        for t in range(2):
            s.step([stage.frames[b][t] for b in range(WC.B)], 0)
        before = s.words(0).copy()
        s.state[s.per:2 * s.per] = fill
        stage.reset(device, s.state, 1)
        torch.cuda.synchronize(device)
        assert np.array_equal(s.words(0), before) and before.any(), (entry, fill, "stream 0 was touched")
        assert not s.words(1).any(), (entry, fill, "stream 1 is not all zero")
        s.rec.check()
        out = s.step([stage.frames[0][2], stage.frames[1][0]], 0)               # stream 0 goes on, stream 1 starts again
        for k in stage.outputs:
            assert np.array_equal(out[k][0], base_outs[2][k][0]), (entry, fill, k, "stream 0")
            assert np.array_equal(out[k][1], base_outs[0][k][1]), (entry, fill, k, "stream 1 is not as fresh")
        assert np.array_equal(s.words(0), base_states[2][0]) and np.array_equal(s.words(1), base_states[0][1]), (entry, fill)
