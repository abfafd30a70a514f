"""_native.grid_inputs on CPU tensors, with _native.on_gpu stubbed the way tests/test_frame_inputs_host.py does it: what it
returns, that a tensor of the right dtype and layout comes back itself, and every NativeError text word for word as grasp,
routes and footprint raised it before they shared the helper.  Then the other shared pieces of a stage wrapper that need no
GPU: host_words, workspace, call on a host-only entry point, and the range checks of the table-grid stages.  (Two grids on
two devices need two devices; the "meta" device stands in for the second one.)"""
import ctypes

import numpy as np
import pytest
import torch

from unseenobjectclustering_amd import _native, placement

WHO = ("grasp", "routes", "footprint")


@pytest.fixture
def any_tensor_is_on_gpu(monkeypatch):
    monkeypatch.setattr(_native, "on_gpu", lambda t: isinstance(t, torch.Tensor))


def grids(B, G, dtype=torch.int32, G2=None):
    state = (torch.arange(B * G * (G2 or G)).reshape(B, G, G2 or G) % 3).to(dtype)
    owner = (torch.arange(B * G * (G2 or G)).reshape(B, G, G2 or G) % 128).to(dtype)
    return state, owner


@pytest.mark.parametrize("who", WHO)
def test_shapes_and_identity(who, any_tensor_is_on_gpu):
    state, owner = grids(1, 8)
    s, o = _native.grid_inputs(who, state[0], owner[0])                     # [G,G] with [G,G]: batched to B = 1
    assert s.shape == o.shape == (1, 8, 8) and s.dtype == o.dtype == torch.int32 and torch.equal(s, state) and torch.equal(o, owner)
    s, o = _native.grid_inputs(who, state[0], owner)                        # [G,G] against [B,G,G] with B = 1
    assert s.shape == o.shape == (1, 8, 8) and o is owner
    state, owner = grids(3, 8)
    s, o = _native.grid_inputs(who, state, owner)
    assert s is state and o is owner                                        # already right: the same objects, no copy
    s, o = _native.grid_inputs(who, state.long(), owner)
    assert o is owner and s.dtype == torch.int32 and torch.equal(s, state)
    for dtype in (torch.int64, torch.int16, torch.uint8, torch.float32):
        s, o = _native.grid_inputs(who, state.to(dtype), owner.to(dtype))
        assert s.dtype == o.dtype == torch.int32 and s.is_contiguous() and o.is_contiguous() and torch.equal(s, state) and torch.equal(o, owner)
    s, o = _native.grid_inputs(who, state.permute(0, 2, 1), owner.permute(0, 2, 1))        # non-contiguous views
    assert s.is_contiguous() and o.is_contiguous() and torch.equal(s, state.permute(0, 2, 1))


@pytest.mark.parametrize("who", WHO)
def test_messages_are_the_stages_own(who, any_tensor_is_on_gpu, monkeypatch):
    state, owner = grids(2, 8)

    def message(s, o):
        with pytest.raises(_native.NativeError) as e:
            _native.grid_inputs(who, s, o)
        assert type(e.value) is _native.NativeError
        return str(e.value)

    no_match = who + ": state %s and owner %s are not two [B,G,G] grids on one device"
    assert message(state[0], owner) == no_match % ("(1, 8, 8)", "(2, 8, 8)")                       # [G,G] against B = 2
    assert message(state, owner[:1]) == no_match % ("(2, 8, 8)", "(1, 8, 8)")
    assert message(*grids(2, 8, G2=16)) == no_match % ("(2, 8, 16)", "(2, 8, 16)")                 # not square
    assert message(grids(1, 8, G2=16)[0][0], grids(1, 8, G2=16)[1][0]) == no_match % ("(1, 8, 16)", "(1, 8, 16)")
    assert message(state, grids(2, 16)[1]) == no_match % ("(2, 8, 8)", "(2, 16, 16)")              # unequal
    assert message(state[0, 0], owner) == no_match % ("(8,)", "(2, 8, 8)")
    assert message(state[None], owner[None]) == no_match % ("(1, 2, 8, 8)", "(1, 2, 8, 8)")
    assert message(state, owner.to("meta")) == no_match % ("(2, 8, 8)", "(2, 8, 8)")               # two devices
    on_gpu = who + ": %s must be a tensor on the GPU (there is no CPU fallback)"
    assert message(state.numpy(), owner) == on_gpu % "state"
    assert message(state, None) == on_gpu % "owner"
    assert message(state.numpy(), owner.numpy()) == on_gpu % "state"                               # state first
    monkeypatch.setattr(_native, "on_gpu", lambda t: isinstance(t, torch.Tensor) and t is not owner)
    assert message(state, owner) == on_gpu % "owner"


def test_without_the_stub_a_host_tensor_is_refused():
    state, owner = grids(1, 8)
    with pytest.raises(_native.NativeError, match="routes: state must be a tensor on the GPU"):
        _native.grid_inputs("routes", state, owner)


def test_host_words():
    w = _native.host_words([(1, 2, 3, 4), (-5, 6, 7, 8)], 4)
    assert isinstance(w, ctypes.Array) and w._type_ is ctypes.c_int32 and list(w) == [1, 2, 3, 4, -5, 6, 7, 8]
    assert list(_native.host_words(np.array([[16384, 0], [0, -16384]], np.int64), 2)) == [16384, 0, 0, -16384]
    assert list(_native.host_words((), 4)) == [0, 0, 0, 0]                  # an empty table still has an address
    assert ctypes.c_void_p.from_param(w) is w                               # a c_void_p argument takes it as it is, no cast


def test_workspace_and_call_on_the_host():
    ws = _native.workspace("uoc_grasp_workspace_bytes", "cpu", 2, 16, 16, 2, who="grasp", hint="B=2 or grid=16")
    assert ws.dtype == torch.uint8 and ws.numel() == _native.lib().uoc_grasp_workspace_bytes(2, 16, 16, 2) > 0
    with pytest.raises(_native.NativeError) as e:
        _native.workspace("uoc_grasp_workspace_bytes", "cpu", 2, 12, 16, 2, who="grasp", hint="B=2 or " + placement.grid_hint(12))
    assert str(e.value) == "grasp: bad shape B=2 or grid=12 (a multiple of 8 in 8..512)"
    h = ctypes.c_void_p()
    with pytest.raises(_native.NativeError, match=r"uoc_net_create_mode failed \(rc=-22\): "):
        _native.call("uoc_net_create_mode", None, ctypes.byref(h), 9)
    _native.call("uoc_net_create_mode", None, ctypes.byref(h), 4)
    assert h.value and _native.lib().uoc_net_embed_dim(h) == 128
    _native.call("uoc_net_destroy", None, h)
    with pytest.raises(AttributeError):
        _native.call("uoc_no_such_function", None)


def test_table_grid_range_checks():
    assert [placement.check_grid(g) for g in (8, 16, 256, 512, "64")] == [8, 16, 256, 512, 64]
    for g in (0, 7, 12, 520, -8):
        with pytest.raises(ValueError) as e:
            placement.check_grid(g)
        assert str(e.value) == f"grid = {g} is not a multiple of 8 in 8..512"
    assert placement.check_min_pts(1) == 1 and placement.check_min_pts(65535) == 65535
    for n in (0, 65536):
        with pytest.raises(ValueError, match=f"min_pts = {n} outside 1..65535"):
            placement.check_min_pts(n)
    assert placement.millimetres(0.010, "cell") == 10 and placement.millimetres(1.0, "tau") == 1000
    assert placement.millimetres(0.0, "h_obs", 0) == 0 and placement.millimetres(0.0004, "h_obs", 0) == 0
    with pytest.raises(ValueError) as e:
        placement.millimetres(0.0, "cell")
    assert str(e.value) == "cell = 0.0 m is 0 mm, outside 1..1000 mm"
    with pytest.raises(ValueError) as e:
        placement.millimetres(1.0006, "step")
    assert str(e.value) == "step = 1.0006 m is 1001 mm, outside 1..1000 mm"
    with pytest.raises(ValueError) as e:
        placement.millimetres(-0.001, "h_obs", 0)
    assert str(e.value) == "h_obs = -0.001 m is -1 mm, outside 0..1000 mm"
