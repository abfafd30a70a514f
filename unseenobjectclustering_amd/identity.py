"""Re-identification on the device (uoc_signature, uoc_sig_similarity, uoc_ident_step, include/uoc_hip.h):
an appearance signature per object and, per stream, identities that survive what the tracker cannot follow.

    tracker, ident = Tracker(), Identifier()
    tracked = tracker.update(refined)                              # track slots: lost after a jump or a long occlusion
    who = ident.update(tracked, tracker, image_u8(sample), xyz)    # int32 map of identities 1..127
    ident.identities()                                             # the one host read: entry, pid, uid, seen, hits, pixels

The tracker keeps an id while masks overlap.  A pushed or picked-and-placed object comes back with IoU 0 and gets a new
slot and uid, and so does one that was hidden for more than `max_age` frames.  `describe` turns every object of a label
map into a signature of 104 integers — a 9x9 chromaticity histogram with bilinear votes, a dark bin, a 9-bin intensity
histogram, the pixel count and a metric area from the depth — and `Identifier` binds a track that appears to the lost
identity whose last signature it resembles (histogram intersection >= min_sim, areas within min_size of each other),
greedily on exact integers.  `pid` numbers the identities of a stream 1, 2, 3, ... and is never reused.  Nothing copies
to the host or synchronises.  Out of scope: position or motion costs, telling two look-alike objects apart (the tie
rule decides deterministically), blending signatures over time.  No CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _native, synth

NUM_IDS = 128
WORDS = _native.SIG_WORDS
_HDR, _META, _NF = _native.IDENT_HEADER_WORDS, _native.IDENT_META_WORD, _native.IDENT_WORDS

# the vote accumulators of uoc_signature: zeroed once, every call leaves them zero
_ACC_BYTES = NUM_IDS * WORDS * 4            # per frame: uoc_signature_workspace_bytes(B) = B times this
_acc = _native.PerStream(lambda dev, B: _native.workspace("uoc_signature_workspace_bytes", dev, B, who="describe", hint=f"B={B}",
                                                          zero=True), size=lambda t: t.numel() // _ACC_BYTES)


class Signatures(_native.Fields):
    """Device tensors.  sig [B,128,104] int32, the rows as include/uoc_hip.h lays them out, and views of it: pixels, valid
    [B,128] int32; hist [B,128,91] int32 = the 81 chroma bins, the dark bin and the 9 intensity bins; area [B,128] int64
    (the 64-bit sum, a visible metric area up to a constant), put together from its two words when it is asked for."""

    @property
    def area(self):
        lo, hi = self.sig[..., _native.SIG_AREA].long(), self.sig[..., _native.SIG_AREA + 1].long()
        return (lo & 0xFFFFFFFF) | (hi << 32)


def sim_threshold(min_sim) -> int:
    """q = round(min_sim * 65536), the integer threshold of the candidate test sim >= q."""
    min_sim = float(min_sim)
    if not 0.0 < min_sim <= 1.0:
        raise ValueError(f"min_sim = {min_sim} outside (0, 1]")
    return max(1, int(round(min_sim * 65536)))


def size_threshold(min_size) -> int:
    """r = round(min_size * 256) in 0..256: min(area) * 256 >= r * max(area); 0 switches the size gate off."""
    min_size = float(min_size)
    if not 0.0 <= min_size <= 1.0:
        raise ValueError(f"min_size = {min_size} outside [0, 1]")
    return int(round(min_size * 256))


def image_u8(sample):
    """The uint8 BGR image [H,W,3] of a sample: sample["image_u8"] when the loader kept it, else recovered from the float
    image_color [1,3,H,W] = BGR/255 - PIXEL_MEANS/255, exactly (every byte value of every channel comes back)."""
    if "image_u8" in sample:
        return sample["image_u8"]
    img = sample["image_color"]
    if img.dim() == 4:
        img = img[0]
    mean = torch.tensor((synth.PIXEL_MEANS / 255.0).astype(np.float32), device=img.device).view(3, 1, 1)
    return torch.clamp(torch.round((img.float() + mean) * 255.0), 0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def image_input(who, image, B, H, W, device):
    """The one check this module adds: a uint8 BGR image [B,H,W,3] ([H,W,3] for B = 1), contiguous, on the labels' GPU;
    else `who`'s NativeError."""
    if not isinstance(image, torch.Tensor):
        raise _native.NativeError(f"{who}: image_u8 must be a tensor on the GPU (there is no CPU fallback)")
    if image.dtype != torch.uint8:
        raise _native.NativeError(f"{who}: image_u8 is {image.dtype}, not torch.uint8 (BGR bytes, [H,W,3])")
    if image.dim() == 3:
        image = image[None]
    if tuple(image.shape) != (B, H, W, 3):
        raise _native.NativeError(f"{who}: image_u8 {tuple(image.shape)} does not match the labels: [{B},{H},{W},3]")
    if not image.is_contiguous():
        raise _native.NativeError(f"{who}: image_u8 is not contiguous (a channel-first view?): pass [H,W,3] bytes as they lie in memory")
    if not _native.on_gpu(image):
        raise _native.NativeError(f"{who}: image_u8 must be a tensor on the GPU (there is no CPU fallback)")
    if image.device != device:
        raise _native.NativeError(f"{who}: labels and image_u8 are on different devices")
    return image


def signature_table(labels, image, xyz=None):
    """The raw uoc_signature call: sig [B,128,104] int32 on the device, no synchronisation.  labels int32 [B,H,W], image
    uint8 [B,H,W,3] and, when given, xyz float32 [B,3,H,W], contiguous on one GPU."""
    B, H, W = (int(v) for v in labels.shape)
    if H * W > _native.SIG_MAX_N:
        raise _native.NativeError(f"describe: H*W = {H * W} above {_native.SIG_MAX_N} pixels (a vote counter is 32 bits)")
    dev = labels.device
    need = _native.lib().uoc_signature_workspace_bytes(B)
    if need == 0:
        raise _native.NativeError(f"describe: bad shape B={B}")
    acc = _acc.get(dev, B)
    sig = torch.empty((B, NUM_IDS, WORDS), dtype=torch.int32, device=dev)
    _native.call("uoc_signature", dev, labels, image, xyz, B, H, W, sig, acc, acc.numel())
    return sig


def describe(labels, image_u8, xyz=None) -> Signatures:
    """labels: device tensor [B,H,W] or [H,W] of int32 / int64 / float ids (1..127 are objects); image_u8: uint8 BGR
    [B,H,W,3] / [H,W,3]; xyz: [B,3,H,W] / [3,H,W] float metres or None (then valid and area are 0 and a size gate never
    passes).  Returns the Signatures of every id."""
    if xyz is None:
        lab = _native.label_input("describe", labels)
        if lab.dim() == 2:
            lab = lab[None]
        if lab.dim() != 3:
            raise _native.NativeError(f"describe: labels {tuple(labels.shape)} must be [H,W] or [B,H,W]")
    else:
        lab, xyz = _native.frame_inputs("describe", labels, xyz)
    B, H, W = (int(v) for v in lab.shape)
    image = image_input("describe", image_u8, B, H, W, lab.device)
    sig = signature_table(lab, image, xyz)
    return Signatures(sig=sig, pixels=sig[..., _native.SIG_PIXELS], valid=sig[..., _native.SIG_VALID],
                      hist=sig[..., _native.SIG_HIST:_native.SIG_INTENSITY + 9])


def similarity(a, b):
    """sim [B,128,128] int32 in 0..65536: the histogram intersection of a's row i and b's row j (Signatures or raw
    [B,128,104] / [128,104] int32 tables), 0 when either id has no pixels."""
    sa, sb = (getattr(t, "sig", t) for t in (a, b))
    for t in (sa, sb):
        if not _native.on_gpu(t) or t.dtype != torch.int32:
            raise _native.NativeError("similarity: signatures must be int32 tensors on the GPU (there is no CPU fallback)")
    sa, sb = (t[None] if t.dim() == 2 else t for t in (sa, sb))
    if sa.dim() != 3 or tuple(sa.shape[1:]) != (NUM_IDS, WORDS) or tuple(sb.shape) != tuple(sa.shape) or sa.device != sb.device:
        raise _native.NativeError(f"similarity: {tuple(sa.shape)} and {tuple(sb.shape)} are not two [B,128,{WORDS}] tables on one device")
    sa, sb = sa.contiguous(), sb.contiguous()
    sim = torch.empty((sa.shape[0], NUM_IDS, NUM_IDS), dtype=torch.int32, device=sa.device)
    _native.call("uoc_sig_similarity", sa.device, sa, sb, int(sa.shape[0]), sim)
    return sim


class Identifier:
    """Identifier(min_sim=0.7, min_size=0.25, max_lost=300, streams=1).  The defaults are design choices (a similarity
    that synthetic colours keep under a gain change of 0.8 and that different synthetic objects stay below, a 4:1 area
    band, ten seconds at 30 Hz), not measurements on real scenes.  The device state is allocated at the first update and
    re-allocated (which resets it) when H, W, the device or the number of streams of the input change."""

    def __init__(self, min_sim=0.7, min_size=0.25, max_lost=300, streams=1):
        self.q, self.r = sim_threshold(min_sim), size_threshold(min_size)
        self.min_sim, self.min_size = float(min_sim), float(min_size)
        self.max_lost, self.streams = int(max_lost), int(streams)
        if self.max_lost < 0:
            raise ValueError(f"max_lost = {max_lost} is negative")
        if self.streams < 1:
            raise ValueError(f"streams = {streams} must be at least 1")
        self._key = None            # (device, B, H, W) of the allocated state
        self._state = self._words = self._ws = self._lut = self._table = None

    def _ensure(self, dev, B, H, W):
        key = (dev, B, H, W)
        if self._key == key:
            return
        self._state = _native.workspace("uoc_ident_state_bytes", dev, B, who="Identifier", hint=f"B={B}")
        self._words = self._state.view(torch.int32).view(B, -1)
        self._ws = _native.workspace("uoc_ident_workspace_bytes", dev, B, who="Identifier", hint=f"B={B}")
        self._lut = torch.zeros((B, NUM_IDS), dtype=torch.int32, device=dev)
        self._table = torch.zeros((B, NUM_IDS, _NF), dtype=torch.int32, device=dev)
        self._key = key
        _native.call("uoc_ident_reset", dev, self._state, B, -1)

    def allocate(self, device, H, W):
        """Allocates (and resets) the state for maps of H x W on `device` ahead of the first update; returns state_words,
        which a caller may fill with a saved state."""
        self._ensure(torch.device(device), self.streams, int(H), int(W))
        return self._words

    def reset(self, stream=None):
        """Forgets every identity of `stream` (all streams when None): its next update starts again at entry 1, pid 1."""
        if stream is not None and not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream = {stream} outside [0, {self.streams})")
        if self._key is None:
            return
        _native.call("uoc_ident_reset", self._key[0], self._state, self.streams, -1 if stream is None else int(stream))
        sel = slice(None) if stream is None else int(stream)
        self._lut[sel] = 0
        self._table[sel] = 0

    def step_tables(self, tracks, sig, tracked):
        """The raw uoc_ident_step call: tracks [streams,128,5] int32 (a Tracker's .table after its update), sig
        [streams,128,104] int32 keyed by track slot, tracked [streams,H,W] int32, all on one GPU.  Returns the identity
        map; .lut and .table hold the rest."""
        B = self.streams
        if tuple(tracks.shape) != (B, NUM_IDS, 5) or tuple(sig.shape) != (B, NUM_IDS, WORDS) or tracked.dim() != 3 or tracked.shape[0] != B:
            raise _native.NativeError(f"Identifier: tracks {tuple(tracks.shape)} / sig {tuple(sig.shape)} / tracked {tuple(tracked.shape)} are "
                                      f"not [{B},128,5] / [{B},128,{WORDS}] / [{B},H,W]")
        dev = sig.device
        H, W = (int(v) for v in tracked.shape[1:])
        self._ensure(dev, B, H, W)
        out = torch.empty_like(tracked)
        _native.call("uoc_ident_step", dev, tracked, tracks.contiguous(), sig.contiguous(), B, H, W, self.q, self.r, self.max_lost,
                     self._state, out, self._lut, self._table, self._ws, self._ws.numel())
        return out

    def update(self, tracked, tracker, image_u8, xyz=None):
        """tracked: the map `tracker.update` just returned, [H,W] or [streams,H,W]; tracker: that Tracker (its .table is
        read on the device); image_u8, xyz: as `describe` takes them.  Returns the identity map, int32, same shape: 0 =
        background, else the identity entry in 1..127."""
        if tracker.streams != self.streams:
            raise ValueError(f"tracker has {tracker.streams} streams, the identifier {self.streams}")
        squeeze = tracked.dim() == 2
        d = describe(tracked, image_u8, xyz)
        if d.sig.shape[0] != self.streams:
            raise _native.NativeError(f"Identifier.update: tracked {tuple(tracked.shape)} must be [H,W] or [{self.streams},H,W]")
        lab = _native.as_labels(tracked)
        out = self.step_tables(tracker.table, d.sig, lab[None] if squeeze else lab)
        return out[0] if squeeze else out

    @property
    def lut(self):
        """[streams,128] int32 on the device: track slot -> identity entry of the last update (0 = not visible)."""
        return self._lut

    @property
    def table(self):
        """[streams,128,5] int32 on the device: pid, uid, seen, hits, pixels per entry after the last update."""
        return self._table

    @property
    def state_words(self):
        """[streams, words] int32 view of the whole device state (table, counters, the entries' signatures)."""
        return self._words

    def identities(self, stream=0):
        """The identities of `stream` as host arrays — the one deliberate device-to-host read: dict of entry, pid, uid,
        seen, hits, pixels (ascending entry), plus next_pid, step and evicted."""
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream = {stream} outside [0, {self.streams})")
        head = np.zeros(_HDR, dtype=np.int32) if self._key is None else self._words[int(stream), :_HDR].cpu().numpy()
        tab = head[:NUM_IDS * _NF].reshape(NUM_IDS, _NF)
        entry = np.nonzero(tab[:, 0])[0].astype(np.int32)
        rec = {name: tab[entry, k].copy() for k, name in enumerate(_native.IDENT_FIELDS)}
        rec.update(entry=entry, next_pid=int(head[_META]) + 1, step=int(head[_META + 1]), evicted=int(head[_META + 2]))
        return rec
