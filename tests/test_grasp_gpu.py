"""uoc_grasp / grasp.candidates on the GPU against the numpy restatement (tests/grasp_reference.py).

The stage has no floating-point output: cand and best are compared with np.array_equal, nothing is sampled.  The grids
are generated in the reference module and tests/test_grasp_host.py asserts on the CPU that they contain what they are
used for here.

Parameter sets (A, M, Wmax, gap, F, Hp, unknown_blocks): the defaults; the lower limits; the upper limits (32 x 25 x 281
bytes of class table: six chunks of directions) with both unknown_blocks; and mixed ones, so that A = 1, 5, 16, 32,
M = 0, 2, 8, Hp = 0, 1, 4, gap = 0, 4, F = 1, 8 and Wmax = 1, 8, 64 each occur.  Grids 8, 64 and 256, B = 1 and 3.

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

from tests import grasp_reference as R
from unseenobjectclustering_amd import _native, grasp

pytestmark = pytest.mark.gpu
EINVAL = -22
DEFAULT = (16, 2, 8, 1, 1, 1, 1)
LIMITS = (32, 8, 64, 4, 8, 4, 1)
CONFIGS = [DEFAULT, (1, 0, 1, 0, 1, 0, 0), LIMITS, (32, 8, 64, 0, 1, 0, 0), (5, 2, 8, 4, 8, 4, 1), (5, 0, 64, 0, 8, 1, 0),
           (16, 8, 1, 4, 1, 0, 1), (16, 2, 8, 1, 1, 1, 0)]


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def random_grid(G, seed):
    return R.random_grid(G, seed, noise_ids=None if G <= 64 else 8)     # G = 256: 3 % redrawn as well, owners from 8 ids


def run(device, st, ow, cfg):
    """uoc_grasp through the raw entry on host grids [G,G] or [B,G,G]; returns host arrays cand, best."""
    A, M, Wmax, gap, F, Hp, ub = cfg
    ds, do = torch.from_numpy(np.ascontiguousarray(st)).to(device), torch.from_numpy(np.ascontiguousarray(ow)).to(device)
    cand, best = grasp.grasp_records(ds, do, R.direction_table(A), M, Wmax, gap, F, Hp, ub)
    B = 1 if st.ndim == 2 else st.shape[0]
    assert cand.shape == (B, 128, A, 2 * M + 1, 2) and best.shape == (B, 128, 8) and cand.dtype == torch.int32 and best.dtype == torch.int32
    assert cand.device.type == "cuda"
    return cand.cpu().numpy(), best.cpu().numpy()


def check(got_cand, got_best, st, ow, cfg, where):
    A, M, Wmax, gap, F, Hp, ub = cfg
    want = R.grasp(st, ow, R.direction_table(A), M, Wmax, gap, F, Hp, ub)
    for k, got in (("cand", got_cand), ("best", got_best)):
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (where, k, got.dtype, got.shape)
        bad = got != want[k]
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6], want[k][bad][:6])
    return want


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_grids_match_reference(device, name):
    st, ow = R.ENGINEERED[name]()
    for cfg in (DEFAULT, CONFIGS[1], CONFIGS[4], CONFIGS[7], (2, 1, 4, 0, 1, 0, 1), (4, 0, 8, 1, 1, 0, 1), (2, 0, 17, 1, 1, 0, 1),
                (2, 0, 33, 1, 1, 0, 1), (16, 2, 24, 1, 1, 1, 1), (2, 0, 1, 4, 8, 0, 1), (4, 1, 2, 4, 8, 1, 0)):
        cand, best = run(device, st, ow, cfg)
        want = check(cand[0], best[0], st, ow, cfg, (name, cfg))
        if name == "empty":
            assert not cand.any() and not best.any()
        if name == "all_ids" and cfg == DEFAULT:
            assert (want["best"][1:, 5] > 0).all()


def test_hand_counted_grids_on_the_device(device):
    S = 16384
    cand, best = run(device, *R.box8(), (2, 1, 4, 0, 1, 0, 1))
    assert cand[0, 1].tolist() == [[[2, -1], [2, -1], [2, -1]], [[-1, 0], [4, -2], [4, -2]]]
    assert best[0, 1].tolist() == [1, 0, 0, -1, 2, 4 * S, 4 * S, 5]
    st, ow = R.box8()
    st[5, 4], ow[5, 4] = 2, 2                                  # +m before -m
    cand, best = run(device, st, ow, (1, 1, 4, 0, 1, 0, 1))
    assert cand[0, 1, 0].tolist() == [[2, -1], [-4, -1], [2, -1]] and best[0, 1].tolist() == [1, 0, 1, -1, 2, 4 * S, 4 * S, 2]
    cand, best = run(device, *R.scene64(), DEFAULT)
    assert [int((cand[0, a, ..., 0] > 0).sum()) for a in range(1, 7)] == [39, 80, 0, 21, 22, 37]
    assert best[0, 1, :5].tolist()[1:3] == [10, 0] and best[0, 1, 4] == 5
    st, ow = R.case_widths(8)                                   # w == Wmax and w == Wmax + 1
    cand, _ = run(device, st, ow, (2, 0, 8, 1, 1, 0, 1))
    assert cand[0, 1, 1, 0].tolist() == [8, -4] and cand[0, 2, 1, 0, 0] == R.WIDE
    st, ow = R.case_beyond_range()                              # finger zones beyond the search range: R = 2, zones to t = 12
    cand, _ = run(device, st, ow, (2, 0, 1, 4, 8, 0, 1))
    assert cand[0, 1].tolist() == [[[R.BLOCKED, 0]], [[R.BLOCKED, 0]]]                  # unknown at t = -11 along i, id 2 at t = 6 along j
    cand, best = run(device, st, ow, (2, 0, 1, 4, 8, 0, 0))
    assert cand[0, 1].tolist() == [[[1, 0]], [[R.BLOCKED, 0]]] and best[0, 1].tolist() == [1, 0, 0, 0, 1, 16 * S + S // 2, 16 * S + S // 2, 1]
    cand, _ = run(device, st, ow, (2, 0, 2, 4, 8, 0, 1))                                # the bar: R = 4, state 3 at t = 11 along j
    assert cand[0, 3].tolist() == [[[R.BLOCKED, 0]], [[R.BLOCKED, -1]]]
    st[16, 22], ow[16, 22], st[26, 25] = 1, 0, 1                                        # the two obstacles removed
    cand, best = run(device, st, ow, (2, 0, 1, 4, 8, 0, 0))
    assert cand[0, 1].tolist() == [[[1, 0]], [[1, 0]]] and best[0, 1, :5].tolist() == [1, 0, 0, 0, 1] and best[0, 1, 7] == 2
    cand, best = run(device, st, ow, (2, 0, 2, 4, 8, 0, 1))
    assert cand[0, 3].tolist() == [[[R.BLOCKED, 0]], [[2, -1]]] and best[0, 3].tolist() == [1, 1, 0, -1, 2, 26 * S + S // 2, 14 * S, 1]


@pytest.mark.parametrize("G", [8, 64, 256])
def test_random_grids_match_reference(device, G):
    frames = [random_grid(G, seed) for seed in (1, 2, 3)]
    st3, ow3 = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    for n, cfg in enumerate(CONFIGS):
        if n % 2 == 0:                                          # B = 3
            cand, best = run(device, st3, ow3, cfg)
            for b in range(3):
                check(cand[b], best[b], *frames[b], cfg, (G, cfg, b))
        else:                                                   # B = 1
            b = n % 3
            cand, best = run(device, *frames[b], cfg)
            check(cand[0], best[0], *frames[b], cfg, (G, cfg, "alone", b))


def test_frames_alone_among_mates_rerun_and_layouts(device):
    frames = [random_grid(64, seed) for seed in (1, 2, 3, 4)]
    st, ow = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    for cfg in (DEFAULT, LIMITS):
        A, M, Wmax, gap, F, Hp, ub = cfg
        d = R.direction_table(A)
        ds, do = torch.from_numpy(st).to(device), torch.from_numpy(ow).to(device)
        whole = grasp.grasp_records(ds[:3], do[:3], d, M, Wmax, gap, F, Hp, ub)
        again = grasp.grasp_records(ds[:3], do[:3], d, M, Wmax, gap, F, Hp, ub)
        assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])            # two runs, the same bits
        order = [3, 2, 0]
        other = grasp.grasp_records(ds[order], do[order], d, M, Wmax, gap, F, Hp, ub)         # frame 0 among other mates
        assert torch.equal(whole[0][0], other[0][2]) and torch.equal(whole[1][0], other[1][2])
        for b in range(3):
            alone = grasp.grasp_records(ds[b], do[b], d, M, Wmax, gap, F, Hp, ub)             # [G,G]
            assert torch.equal(whole[0][b], alone[0][0]) and torch.equal(whole[1][b], alone[1][0])
        # int64 grids, and non-contiguous ones (a transposed view of the transposed grids): the same bits
        wide = grasp.grasp_records(ds[:3].long(), do[:3].long(), d, M, Wmax, gap, F, Hp, ub)
        ts, to = ds[:3].transpose(1, 2).contiguous().transpose(1, 2), do[:3].transpose(1, 2).contiguous().transpose(1, 2)
        assert not ts.is_contiguous() and torch.equal(ts, ds[:3])
        strided = grasp.grasp_records(ts, to, d, M, Wmax, gap, F, Hp, ub)
        for other in (wide, strided):
            assert torch.equal(whole[0], other[0]) and torch.equal(whole[1], other[1])
    check(whole[0][1].cpu().numpy(), whole[1][1].cpu().numpy(), *frames[1], LIMITS, "batch")


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, G, A, M = 2, 16, 4, 1
    wsb = lib.uoc_grasp_workspace_bytes
    nws = wsb(B, G, A, M)
    assert nws > 0 and wsb(0, G, A, M) == 0 and wsb(65536, G, A, M) == 0 and wsb(65535, G, A, M) > 0
    assert wsb(B, 0, A, M) == 0 and wsb(B, 12, A, M) == 0 and wsb(B, 520, A, M) == 0 and wsb(B, 512, A, M) > 0 and wsb(B, 8, A, M) > 0
    assert wsb(B, G, 0, M) == 0 and wsb(B, G, 33, M) == 0 and wsb(B, G, 32, M) > 0 and wsb(B, G, A, -1) == 0 and wsb(B, G, A, 9) == 0
    assert wsb(B, G, A, 8) > 0
    st, ow = R.case_single_cells()
    ds, do = torch.from_numpy(np.stack([st] * B)).to(device), torch.from_numpy(np.stack([ow] * B)).to(device)
    cand = torch.full((B, 128, A, 2 * M + 1, 2), -7, dtype=torch.int32, device=device)
    best = torch.full((B, 128, 8), -7, dtype=torch.int32, device=device)
    ws = torch.full((nws,), 0x55, dtype=torch.uint8, device=device)
    ws_big = torch.full((nws + 16,), 0x55, dtype=torch.uint8, device=device)
    ws_off = ws_big[4:]                                         # large enough, but 4 bytes off a 16-byte boundary
    P, stream = _native.ptr, _native.stream_ptr(device)
    assert ws.data_ptr() % 16 == 0 and ws_off.data_ptr() % 16 == 4
    good = R.direction_table(A).reshape(-1).tolist()

    def call(B_=B, G_=G, dirs=good, A_=A, M_=M, Wmax=8, gap=1, F=1, Hp=1, ub=1, st_=ds, ow_=do, cand_=cand, best_=best, ws_=ws, nws_=nws,
             null_dirs=False):
        hd = (ctypes.c_int32 * max(len(dirs), 1))(*dirs)
        return lib.uoc_grasp(P(st_), P(ow_), B_, G_, None if null_dirs else ctypes.cast(hd, ctypes.c_void_p), A_, M_, Wmax, gap, F, Hp, ub,
                             P(cand_), P(best_), P(ws_), nws_, stream)

    over = [16384] * 2 * A
    for kw in (dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(G_=-8), dict(A_=0), dict(A_=33),
               dict(M_=-1), dict(M_=9), dict(Wmax=0), dict(Wmax=65), dict(gap=-1), dict(gap=5), dict(F=0), dict(F=9), dict(Hp=-1),
               dict(Hp=5), dict(ub=2), dict(ub=-1), dict(null_dirs=True), dict(st_=None), dict(ow_=None), dict(cand_=None),
               dict(best_=None), dict(ws_=None), dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ws_off), dict(dirs=over[:-1] + [16385]),
               dict(dirs=[-16385] + over[1:]), dict(dirs=good[:3] + [1 << 20] + good[4:])):
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert bool((cand == -7).all()) and bool((best == -7).all()) and bool((ws == 0x55).all()) and bool((ws_big == 0x55).all())
    assert call() == 0 and call(dirs=over) == 0 and call() == 0
    torch.cuda.synchronize()
    check(cand[1].cpu().numpy(), best[1].cpu().numpy(), st, ow, (A, M, 8, 1, 1, 1, 1), "after the rejected calls")
    d = R.direction_table(A)
    for bad in (dict(offsets=9), dict(offsets=-1), dict(max_open=0), dict(max_open=65), dict(gap=5), dict(finger=0), dict(finger=9),
                dict(pad=5), dict(dirs=np.zeros((33, 2), np.int64)), dict(dirs=np.zeros((0, 2), np.int64)), dict(dirs=d * 2),
                dict(dirs=d.reshape(-1))):
        kw = {**dict(dirs=d, offsets=1, max_open=8, gap=1, finger=1, pad=1, unknown_blocks=1), **bad}
        with pytest.raises(ValueError):
            grasp.grasp_records(ds, do, **kw)
    kw = dict(dirs=d, offsets=1, max_open=8, gap=1, finger=1, pad=1, unknown_blocks=1)
    with pytest.raises(_native.NativeError):
        grasp.grasp_records(ds.cpu(), do, **kw)
    with pytest.raises(_native.NativeError):
        grasp.grasp_records(ds, do[:1], **kw)
    with pytest.raises(_native.NativeError):
        grasp.grasp_records(ds[:, :12, :12], do[:, :12, :12], **kw)              # G = 12


def placed_of(device, st, ow, unknown_blocks=True, cell_mm=10):
    """What grasp.candidates reads of a placement result, from bare grids and the flat plane z = 1 m."""
    from unseenobjectclustering_amd import placement
    planes = placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0])
    return placement.PlacementResult(state=torch.from_numpy(st[None]).to(device), owner=torch.from_numpy(ow[None]).to(device),
                                     planes=torch.from_numpy(planes).to(device), grid=st.shape[0], cell_mm=cell_mm,
                                     unknown_blocks=unknown_blocks)


def test_candidates_and_helpers(device):
    st, ow = R.scene64()
    st[8:10, 40:46] = 0                                         # an unknown patch under a finger of box 4: unknown_blocks matters
    for ub, over in ((True, None), (False, None), (True, False)):
        res = grasp.candidates(placed_of(device, st, ow, ub), unknown_blocks=over)
        want_ub = ub if over is None else over
        assert (res.angles, res.offsets, res.max_open, res.gap, res.finger, res.pad, res.unknown_blocks) == (16, 2, 8, 1, 1, 1, want_ub)
        want = check(res.cand[0].cpu().numpy(), res.best[0].cpu().numpy(), st, ow, (16, 2, 8, 1, 1, 1, int(want_ub)), ("candidates", ub, over))
    ok = grasp.graspable(res)
    assert ok.shape == (1, 128) and ok.dtype == torch.bool and ok.device.type == "cuda"
    assert np.array_equal(ok[0].cpu().numpy(), want["best"][:, 0] == 1) and ok[0].nonzero().reshape(-1).tolist() == [1, 2, 4, 5, 6]
    assert grasp.pose(res, 0, 3) is None and grasp.pose(res, 0, 9) is None
    p = grasp.pose(res, 0, 1)                                   # the rotated box: across it, 5 cells of 1 cm, through its centre
    assert (p.k, p.m) == (10, 0) and abs(p.width_m - 0.05) < 1e-12 and abs(p.opening_m - 0.07) < 1e-12
    assert np.allclose(p.center, [0.0, 0.0, 1.0], rtol=0, atol=0.005) and abs(p.axis[2]) < 1e-6
    assert np.allclose(p.axis, [np.cos(np.pi * 10 / 16), -np.sin(np.pi * 10 / 16), 0], rtol=0, atol=1e-4)
    res5 = grasp.candidates(placed_of(device, st, ow, True, cell_mm=5), angles=5, offsets=0, max_open=0.04, gap=0.0, finger=0.005, pad=0.0)
    check(res5.cand[0].cpu().numpy(), res5.best[0].cpu().numpy(), st, ow, (5, 0, 8, 0, 1, 0, 1), "cell 5 mm")
    for bad in (dict(angles=0), dict(angles=33), dict(offsets=9), dict(max_open=0.7), dict(max_open=0.001), dict(gap=0.05), dict(finger=0.0),
                dict(pad=0.2)):
        with pytest.raises(ValueError):
            grasp.candidates(placed_of(device, st, ow), **bad)


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_grasp_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out = O.segment_objects(sample, net, net_crop, grasp=True)                       # implies placement, which implies the plane
    assert len(out) == 6
    placed, grasped = out[4], out[5]
    assert hasattr(out[3], "normal") and hasattr(placed, "dist2") and grasped.planes.data_ptr() == placed.planes.data_ptr()
    st, ow = placed.state[0].cpu().numpy(), placed.owner[0].cpu().numpy()
    check(grasped.cand[0].cpu().numpy(), grasped.best[0].cpu().numpy(), st, ow, DEFAULT, "demo")
    np.random.seed(3)
    out2 = O.segment_objects(sample, net, net_crop, placement=True, grasp=True, grasp_args=dict(angles=5, offsets=0, unknown_blocks=False))
    assert len(out2) == 6 and torch.equal(out2[4].state, placed.state)
    check(out2[5].cand[0].cpu().numpy(), out2[5].best[0].cpu().numpy(), st, ow, (5, 0, 8, 1, 1, 1, 0), "demo, other arguments")
