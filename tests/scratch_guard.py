"""Guarded scratch for the workspace contract tests (tests/test_workspace_contract_*.py).

guarded(device, nbytes, fill, offset) cuts a uint8 view of exactly `nbytes` out of one larger allocation: its address is
offset mod 256 (mod `align` where an entry asks for more than the allocator's 256: offset 256 with align 512 is a pointer
that is 256- but not 512-byte aligned), it is pre-filled with the byte `fill`, and at least GUARD bytes on either side hold
a canary pattern that differs from every fill.  check() asserts that both canaries are intact.  A guard band inside an
ordinary allocation is the only overrun check that runs on the device: a kernel that writes past its carve, or a
*_workspace_bytes that under-reports, lands in the canary instead of in the allocator's slack.

guard_workspaces(fill, offset) patches _native.workspace so that every wrapper which takes its scratch (or its state) from
it receives such a view of exactly the size function's value; it records what it handed out and verifies every canary on
exit.  Works on CPU tensors too."""
import contextlib

import torch

from unseenobjectclustering_amd import _native

GUARD = 4096                    # canary bytes on either side, at least
ALIGN = 256                     # the view's address is `offset` modulo this, unless the caller names a larger power of two
FILLS = (0x00, 0xFF, 0x55)      # fresh allocation; -1 / NaN / the top of every counter; an odd pattern that is neither
CANARY_BASE, CANARY_PERIOD = 0xA0, 16       # canary byte at buffer index i = 0xA0 + i % 16: never a fill


def canary(lo, hi, device):
    """The canary bytes of buffer indices lo..hi-1."""
    return (torch.arange(lo, hi, device=device) % CANARY_PERIOD + CANARY_BASE).to(torch.uint8)


class GuardError(AssertionError):
    pass


class Guarded:
    """One guarded view: .view (uint8, nbytes long), .address, .nbytes, .name; check() raises GuardError naming the first
    changed canary byte and its distance from the view (1 = the byte next to it)."""

    def __init__(self, device, nbytes, fill, offset=0, name="scratch", align=ALIGN):
        nbytes, offset = int(nbytes), int(offset)
        assert nbytes >= 0 and align >= ALIGN and align & (align - 1) == 0 and 0 <= offset < align and 0 <= fill <= 0xFF
        total = 2 * (GUARD + align) + nbytes
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        self.start = GUARD + (offset - (self.buf.data_ptr() + GUARD)) % align
        self.end = self.start + nbytes
        self.name, self.nbytes, self.fill, self.offset = name, nbytes, fill, offset
        self.buf[:self.start] = canary(0, self.start, self.buf.device)
        self.buf[self.end:] = canary(self.end, total, self.buf.device)
        self.view = self.buf[self.start:self.end]
        self.view.fill_(fill)
        self.address = self.view.data_ptr() if nbytes else self.buf.data_ptr() + self.start
        assert self.address % align == offset and self.start >= GUARD and total - self.end >= GUARD

    def refill(self, fill):
        self.fill = fill
        self.view.fill_(fill)
        return self.view

    def damage(self):
        """None, or (side, distance, found, expected) of the first changed canary byte in address order."""
        total = self.buf.numel()
        for side, lo, hi in (("before", 0, self.start), ("after", self.end, total)):
            bad = torch.nonzero(self.buf[lo:hi] != canary(lo, hi, self.buf.device))
            if bad.numel():
                i = lo + int(bad[0])
                dist = self.start - i if side == "before" else i - self.end + 1
                return side, dist, int(self.buf[i]), CANARY_BASE + i % CANARY_PERIOD
        return None

    def check(self):
        d = self.damage()
        if d is not None:
            side, dist, found, want = d
            raise GuardError(f"{self.name}: canary changed {dist} byte(s) {side} the {self.nbytes}-byte view at offset "
                             f"{self.offset} (found 0x{found:02x}, expected 0x{want:02x})")


def guarded(device, nbytes, fill, offset=0, name="scratch", align=ALIGN):
    return Guarded(device, nbytes, fill, offset, name, align)


class Record:
    """The guarded buffers of one run: .items, a list of Guarded in hand-out order.  take(name, nbytes) hands one out
    directly, for a test that calls a C entry itself; guard_workspaces(record=...) hands them to the wrappers."""

    def __init__(self, device=None, fill=0, offset=0, align=ALIGN, state_fill=None):
        self.device, self.fill, self.offset, self.align, self.state_fill = device, fill, offset, align, state_fill
        self.items = []

    def take(self, name, nbytes, fill=None, device=None):
        g = Guarded(self.device if device is None else device, nbytes, self.fill if fill is None else fill, self.offset, name,
                    self.align)
        self.items.append(g)
        return g.view

    def names(self):
        return [g.name for g in self.items]

    def table(self):
        return [(g.name, g.nbytes, g.address) for g in self.items]

    def check(self):
        for g in self.items:
            g.check()


@contextlib.contextmanager
def guard_workspaces(fill=0, offset=0, state_fill=None, record=None):
    """Patches _native.workspace: every hand-out is a guarded view of exactly the size function's value, filled `fill`
    (a *_state_bytes hand-out with `state_fill` when given; a zero=True request with 0, its contract).  Yields the Record
    (`record` when given: its fill, offset and alignment hold); on a clean exit every canary is verified."""
    rec = Record(None, fill, offset, ALIGN, state_fill) if record is None else record
    real = _native.workspace

    def workspace(name, device, *shape, who, hint, floor=0, zero=False):
        nbytes = getattr(_native.lib(), name)(*shape)
        if nbytes == 0 and floor == 0:
            raise _native.NativeError(f"{who}: bad shape {hint}")
        f = 0 if zero else rec.state_fill if (rec.state_fill is not None and name.endswith("_state_bytes")) else rec.fill
        return rec.take(name, max(nbytes, floor), f, device)

    _native.workspace = workspace
    try:
        yield rec
    finally:
        _native.workspace = real
    if any(g.buf.device.type == "cuda" for g in rec.items):
        torch.cuda.synchronize()
    rec.check()
