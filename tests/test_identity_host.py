"""Re-identification without a GPU: the uint8 image recovered from a float sample, the thresholds rounded once on the host,
the validation of the C ABI before any HIP call with its messages, the input checks of identity.py, the refusal of CPU
tensors, and `--reid` without `--track` on both tools."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import identity_reference as ir
from unseenobjectclustering_amd import _native, identity, tracking
from unseenobjectclustering_amd import io as uio
from unseenobjectclustering_amd.fcn.config import cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_u8_round_trip_returns_every_byte_of_every_channel():
    im = np.zeros((16, 16, 3), dtype=np.uint8)
    for c in range(3):
        im[..., c] = (np.arange(256, dtype=np.int64).reshape(16, 16) * (1, 7, 11)[c] + c) % 256      # all 256 values per channel
        assert len(np.unique(im[..., c])) == 256
    cam = dict(fx=500.0, fy=500.0, x_offset=8.0, y_offset=8.0)
    saved = cfg.INPUT
    cfg.INPUT = "RGBD"
    try:
        sample = uio.make_sample(im, np.full((16, 16), 800, dtype=np.uint16), cam)
    finally:
        cfg.INPUT = saved
    assert sample["image_color"].dtype == torch.float32 and "image_u8" not in sample
    back = identity.image_u8(sample)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (16, 16, 3) and back.is_contiguous()
    assert np.array_equal(back.numpy(), im)
    raw = uio.make_sample_raw(im, np.zeros((16, 16), dtype=np.uint16), cam)
    assert identity.image_u8(raw) is raw["image_u8"]


def test_thresholds_are_rounded_once_on_the_host():
    assert identity.sim_threshold(0.7) == 45875 == ir.sim_threshold(0.7)
    assert identity.sim_threshold(1.0) == 65536 and identity.sim_threshold(1e-9) == 1
    assert identity.size_threshold(0.25) == 64 == ir.size_threshold(0.25)
    assert identity.size_threshold(0.0) == 0 and identity.size_threshold(1.0) == 256
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="min_sim"):
            identity.sim_threshold(bad)
    for bad in (-0.1, 1.01):
        with pytest.raises(ValueError, match="min_size"):
            identity.Identifier(min_size=bad)
    with pytest.raises(ValueError, match="max_lost"):
        identity.Identifier(max_lost=-1)
    with pytest.raises(ValueError, match="streams"):
        identity.Identifier(streams=0)
    ident = identity.Identifier()
    assert (ident.q, ident.r, ident.max_lost, ident.streams) == (45875, 64, 300, 1)
    with pytest.raises(ValueError, match="stream"):
        ident.reset(1)
    ident.reset()
    rec = ident.identities()
    assert rec["entry"].size == 0 and rec["next_pid"] == 1 and rec["step"] == 0 and rec["evicted"] == 0 and ident.lut is None
    with pytest.raises(ValueError, match="streams"):
        ident.update(torch.zeros(4, 4, dtype=torch.int32), tracking.Tracker(streams=2), torch.zeros(4, 4, 3, dtype=torch.uint8))


def last_error():
    return _native.lib().uoc_last_error().decode().lower()


def test_sizes_and_constants():
    lib = _native.lib()
    assert lib.uoc_signature_workspace_bytes(1) == 128 * 104 * 4 and lib.uoc_signature_workspace_bytes(12) == 12 * 128 * 104 * 4
    assert lib.uoc_ident_state_bytes(1) == (1024 + 128 * 104) * 4 and lib.uoc_ident_state_bytes(3) == 3 * lib.uoc_ident_state_bytes(1)
    assert lib.uoc_ident_workspace_bytes(2) == 2 * 128 * 4
    for fn in (lib.uoc_signature_workspace_bytes, lib.uoc_ident_state_bytes, lib.uoc_ident_workspace_bytes):
        assert fn(0) == 0 and fn(-1) == 0 and fn(65536) == 0
    assert (_native.SIG_WORDS, _native.SIG_MAX_N, _native.SIG_DARK) == (104, 1 << 24, 89) == (ir.WORDS, ir.MAX_N, ir.DARK)
    assert (_native.SIG_HIST, _native.SIG_INTENSITY) == (ir.HIST, ir.INTENSITY) and _native.IDENT_FIELDS == ir.FIELDS
    assert _native.IDENT_WORDS == len(ir.FIELDS) and _native.IDENT_WORDS * 128 <= _native.IDENT_META_WORD < _native.IDENT_HEADER_WORDS


def test_calls_validate_without_a_device():
    lib = _native.lib()
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its validation first
    ws = lib.uoc_signature_workspace_bytes(2)

    def sig(labels=p, image=p, xyz=None, B=2, H=48, W=64, out=p, d_ws=p, nws=ws):
        return lib.uoc_signature(labels, image, xyz, B, H, W, out, d_ws, nws, None)

    for kw in (dict(labels=None), dict(image=None), dict(out=None), dict(d_ws=None)):
        assert sig(**kw) == -22 and "null" in last_error(), kw
    for kw in (dict(B=0), dict(H=0), dict(W=-3)):
        assert sig(**kw) == -22 and "shape" in last_error(), kw
    assert sig(B=1, H=4096, W=4097) == -22 and "uoc_sig_max_n" in last_error() and str(4096 * 4097) in last_error()
    assert sig(nws=ws - 1) == -22 and "workspace" in last_error()
    assert sig(d_ws=ctypes.c_void_p((1 << 20) + 4)) == -22 and "aligned" in last_error()

    assert lib.uoc_sig_similarity(None, p, 1, p, None) == -22 and "null" in last_error()
    assert lib.uoc_sig_similarity(p, p, 0, p, None) == -22 and "b=" in last_error()
    assert lib.uoc_sig_similarity(p, ctypes.c_void_p((1 << 20) + 8), 1, p, None) == -22 and "aligned" in last_error()

    iws = lib.uoc_ident_workspace_bytes(2)

    def step(tracked=p, tracks=p, s=p, B=2, H=48, W=64, q=45875, r=64, max_lost=300, state=p, out=p, d_ws=p, nws=iws):
        return lib.uoc_ident_step(tracked, tracks, s, B, H, W, q, r, max_lost, state, out, None, None, d_ws, nws, None)

    for kw in (dict(tracked=None), dict(tracks=None), dict(s=None), dict(state=None), dict(out=None), dict(d_ws=None)):
        assert step(**kw) == -22 and "null" in last_error(), kw
    for kw in (dict(B=0), dict(H=0), dict(W=-3)):
        assert step(**kw) == -22 and "shape" in last_error(), kw
    assert step(H=65536, W=32768) == -22 and "31 bits" in last_error()
    for q in (0, -1, 65537):
        assert step(q=q) == -22 and "q =" in last_error() and "min_sim" in last_error()
    for r in (-1, 257):
        assert step(r=r) == -22 and "r =" in last_error() and "min_size" in last_error()
    assert step(max_lost=-1) == -22 and "max_lost" in last_error()
    assert step(nws=iws - 1) == -22 and "workspace" in last_error()
    assert step(state=ctypes.c_void_p((1 << 20) + 4)) == -22 and "aligned" in last_error()

    assert lib.uoc_ident_reset(None, 1, -1, None) == -22 and "null" in last_error()
    assert lib.uoc_ident_reset(p, 0, -1, None) == -22 and "b=" in last_error()
    for which in (-2, 3):
        assert lib.uoc_ident_reset(p, 3, which, None) == -22 and "stream" in last_error()


def test_image_check_and_its_messages():
    dev = torch.device("cpu")
    with pytest.raises(_native.NativeError, match="not torch.uint8"):
        identity.image_input("describe", torch.zeros(4, 6, 3), 1, 4, 6, dev)
    with pytest.raises(_native.NativeError, match="does not match the labels"):
        identity.image_input("describe", torch.zeros(3, 4, 6, dtype=torch.uint8), 1, 4, 6, dev)
    with pytest.raises(_native.NativeError, match="not contiguous"):
        identity.image_input("describe", torch.zeros(3, 4, 6, dtype=torch.uint8).permute(1, 2, 0), 1, 4, 6, dev)
    with pytest.raises(_native.NativeError, match="on the GPU"):
        identity.image_input("describe", torch.zeros(4, 6, 3, dtype=torch.uint8), 1, 4, 6, dev)
    with pytest.raises(_native.NativeError, match="on the GPU"):
        identity.image_input("describe", np.zeros((4, 6, 3), dtype=np.uint8), 1, 4, 6, dev)


def test_cpu_tensors_are_refused():
    lab, img = torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_native.NativeError, match="labels"):
        identity.describe(lab, img)
    with pytest.raises(_native.NativeError):
        identity.describe(lab, img, torch.zeros(3, 8, 8))
    with pytest.raises(_native.NativeError, match="similarity"):
        identity.similarity(torch.zeros(128, 104, dtype=torch.int32), torch.zeros(128, 104, dtype=torch.int32))
    with pytest.raises(_native.NativeError):
        identity.Identifier().update(lab, tracking.Tracker(), img)


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reid_needs_track_on_both_tools(capsys):
    exporter = load("uoc_export_objects_reid", ("tools", "export_objects.py"))
    with pytest.raises(SystemExit):
        exporter.parse_args(["--imgdir", "x", "--out", "y", "--reid"])
    assert "--reid needs --track" in capsys.readouterr().err
    args = exporter.parse_args(["--imgdir", "x", "--out", "y", "--track", "--reid", "--reid-max-lost", "7"])
    assert args.reid and (args.reid_min_sim, args.reid_min_size, args.reid_max_lost) == (0.7, 0.25, 7)
    assert exporter.parse_args(["--imgdir", "x", "--out", "y", "--track"]).reid is False
    with pytest.raises(SystemExit):
        exporter.parse_args(["--imgdir", "x", "--out", "y", "--track", "--reid", "--reid-min-sim", "0"])
    capsys.readouterr()

    from tests.test_ros_node import load_node_module
    tracked = load("uoc_ros_tracked_reid", ("ros", "segmentation_tracked.py"))
    base = load_node_module()
    with pytest.raises(SystemExit):
        tracked.parse_args(base, ["--reid"])
    assert "--reid needs --track" in capsys.readouterr().err
    args = tracked.parse_args(base, ["--track", "--reid", "--reid_min_sim", "0.8"])
    assert args.track and args.reid == dict(min_sim=0.8, min_size=0.25, max_lost=300)
    assert tracked.parse_args(base, ["--track"]).reid is None and tracked.parse_args(base, []).reid is None
    with pytest.raises(ValueError, match="reid needs track"):
        tracked.make_node(base, "net", "crop", None, reid=dict())
