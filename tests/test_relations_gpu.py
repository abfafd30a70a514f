"""uoc_relations / relations.relate on the GPU against the numpy restatement (tests/relations_reference.py).

The feature has no floating-point output: every table and every record field is compared with np.array_equal.  The
scenes are generated in the reference module (seeded) and tests/test_relations_host.py asserts on the CPU that they
contain what they are used for here (occluding, touching and edge objects, the cycle, the thresholds).

Sizes: 1x1, 1x2, 2x1, 3x1 (no / one / two pairs), 24x32 and 61x83 (one block, rows that do not line up with a wave),
97x131 (two blocks: the smallest seeded frame whose pairs cross a block's pixel span), 224x224 and 480x640.

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import faulthandler
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import relations_reference as R
from unseenobjectclustering_amd import _native, relations

pytestmark = pytest.mark.gpu
EINVAL = -22

# (seed, connectivity, gap_mm, min_pairs)
GRID = [(s, c, g, m) for s in (1, 2) for c in (4, 8) for g, m in ((15, 8), (5, 1), (40, 3))]
COMBOS = {(1, 1): GRID[::5], (1, 2): GRID[::3], (2, 1): GRID[::3], (3, 1): GRID[::3], (24, 32): GRID, (61, 83): GRID,
          (97, 131): [(1, 8, 15, 4), (2, 4, 5, 2)], (224, 224): [(1, 8, 15, 8)], (480, 640): [(2, 4, 15, 8)]}


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def scene(H, W, seed):
    return R.tabletop(H, W, seed)


def to_dev(device, lab, xyz):
    return torch.from_numpy(np.ascontiguousarray(lab)).to(device), torch.from_numpy(np.ascontiguousarray(xyz)).to(device)


def host(res, b):
    return {k: getattr(res, k)[b].cpu().numpy() for k in R.TABLES + R.FIELDS}


def check_frame(got, want, where):
    for k in R.TABLES + R.FIELDS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (where, k, got[k][got[k] != want[k]][:8],
                                                                            want[k][got[k] != want[k]][:8])


@pytest.mark.parametrize("H,W", list(COMBOS))
def test_tabletop_scenes_match_reference(device, H, W):
    for seed, conn, gap_mm, min_pairs in COMBOS[(H, W)]:
        lab, xyz = scene(H, W, seed)
        res = relations.relate(*to_dev(device, lab, xyz), connectivity=conn, gap=gap_mm / 1000.0, min_pairs=min_pairs)
        assert res.front.shape == (1, 128, 128) and res.layer.shape == (1, 128) and res.front.device.type == "cuda"
        assert res.gap_mm == gap_mm
        check_frame(host(res, 0), R.relations(lab, xyz[2], conn, gap_mm, min_pairs), (H, W, seed, conn, gap_mm, min_pairs))


@pytest.mark.parametrize("pattern", ["checkerboard", "row_stripes"])
def test_two_id_patterns_counters_do_not_wrap(device, pattern):
    """480x640, connectivity 8: every pair of two ids meets in one cell per table, 2 (checkerboard) or 3 (row stripes) per
    pixel, so a block's 16-bit counters carry 16 and 24 thousand."""
    lab, xyz = getattr(R, pattern)(480, 640)
    res = relations.relate(*to_dev(device, lab, xyz), connectivity=8, gap=0.015, min_pairs=8)
    want = R.relations(lab, xyz[2], 8, 15, 8)
    pairs = 480 * 639 + 479 * 640 if pattern == "checkerboard" else 479 * 640 + 2 * 479 * 639
    assert want["front"][1, 2] == want["border"][1, 2] == pairs
    check_frame(host(res, 0), want, pattern)


@pytest.mark.parametrize("name", list(R.ENGINEERED))
def test_engineered_cases_match_reference(device, name):
    c = R.ENGINEERED[name]()
    dl, dx = to_dev(device, c["lab"], c["xyz"])
    for conn, gap_mm, min_pairs in ((c["connectivity"], c["gap_mm"], c["min_pairs"]), (12 - c["connectivity"], c["gap_mm"], 1),
                                    (8, 1, 2), (4, 65535, 1)):
        res = relations.relate(dl, dx, connectivity=conn, gap=gap_mm / 1000.0, min_pairs=min_pairs)
        check_frame(host(res, 0), R.relations(c["lab"], c["xyz"][2], conn, gap_mm, min_pairs), (name, conn, gap_mm, min_pairs))
    res = relations.relate(dl, dx, connectivity=c["connectivity"], gap=c["gap_mm"] / 1000.0, min_pairs=c["min_pairs"])
    layer = res.layer[0].cpu().numpy()
    if name == "chain5":
        assert layer[1:6].tolist() == [1, 2, 3, 4, 5] and relations.pick_order(res) == [1, 2, 3, 4, 5]
        assert relations.occluders(res, 0, 3) == [2] and relations.neighbours(res, 0, 3) == []
    if name == "cycle":
        assert layer[1:5].tolist() == [-1] * 4 and not res.free[0].any()
    if name == "stripes127":
        assert layer[1:].tolist() == list(range(1, 128)) and relations.pick_order(res) == list(range(1, 128))
    if name == "at_gap":
        assert relations.occluders(res, 0, 2) == [1] and relations.neighbours(res, 0, 3) == [4]


def test_label_dtypes_and_unbatched_input(device):
    lab, xyz = scene(61, 83, 1)
    dl, dx = to_dev(device, lab, xyz)
    a = relations.relate(dl[None], dx[None])
    for other in (relations.relate(dl, dx), relations.relate(dl.float(), dx), relations.relate(dl.long()[None], dx.double()[None])):
        for k in R.TABLES + R.FIELDS:
            assert torch.equal(getattr(a, k), getattr(other, k)), k


def test_deterministic_and_batch_independent(device):
    frames = [scene(61, 83, 1), scene(61, 83, 2), (R.checkerboard(61, 83)), scene(61, 83, 3)]
    dl, dx = to_dev(device, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
    kw = dict(connectivity=8, gap=0.015, min_pairs=4)

    def same(a, b, rows_a, rows_b, where):
        for k in R.TABLES + R.FIELDS:
            assert torch.equal(getattr(a, k)[rows_a], getattr(b, k)[rows_b]), (where, k)

    whole = relations.relate(dl[:3], dx[:3], **kw)
    same(whole, relations.relate(dl[:3], dx[:3], **kw), slice(None), slice(None), "rerun")
    other = relations.relate(dl[[3, 2, 0]], dx[[3, 2, 0]], **kw)                 # frame 0 with different mates, B = 3
    same(whole, other, slice(0, 1), slice(2, 3), "mates")
    for b in range(3):
        same(whole, relations.relate(dl[b], dx[b], **kw), slice(b, b + 1), slice(None), ("alone", b))
        check_frame(host(whole, b), R.relations(frames[b][0], frames[b][1][2], 8, 15, 4), ("batch", b))


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, H, W = 2, 24, 32
    lab, xyz = to_dev(device, np.stack([scene(H, W, 1)[0]] * B), np.stack([scene(H, W, 1)[1]] * B))
    nws = lib.uoc_relations_workspace_bytes(B, H, W)
    assert nws > 0 and lib.uoc_relations_workspace_bytes(0, H, W) == 0 and lib.uoc_relations_workspace_bytes(B, 0, W) == 0
    assert lib.uoc_relations_workspace_bytes(B, 1 << 15, 1 << 14) == 0 and lib.uoc_relations_workspace_bytes(1, (1 << 29) - 1, 1) > 0
    assert lib.uoc_relations_workspace_bytes(65536, H, W) == 0
    pairs = torch.full((B, 3, 128, 128), -7, dtype=torch.int32, device=device)
    objs = torch.full((B, 128, 11), -7, dtype=torch.int32, device=device)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    P, st = _native.ptr, _native.stream_ptr(device)

    def call(conn=4, gap_mm=15, min_pairs=8, pairs_=pairs, objs_=objs, ws_=ws, nws_=nws, lab_=lab, xyz_=xyz, B_=B, H_=H, W_=W):
        return lib.uoc_relations(P(lab_), P(xyz_), B_, H_, W_, conn, gap_mm, min_pairs, P(pairs_), P(objs_), P(ws_), nws_, st)

    for kw in (dict(conn=0), dict(conn=6), dict(gap_mm=0), dict(gap_mm=65536), dict(gap_mm=-1), dict(min_pairs=0), dict(nws_=nws - 1),
               dict(pairs_=None), dict(objs_=None), dict(ws_=None), dict(lab_=None), dict(xyz_=None), dict(B_=0), dict(H_=0),
               dict(W_=-1), dict(H_=1 << 15, W_=1 << 14)):
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    assert bool((pairs == -7).all()) and bool((objs == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(pairs.min()) == 0 and int(objs[0, 1, 0]) > 0 and torch.equal(objs[0], objs[1])
    for bad in (dict(connectivity=6), dict(gap=0.0), dict(gap=66.0), dict(min_pairs=0)):
        with pytest.raises(ValueError):
            relations.relate(lab, xyz, **bad)
    with pytest.raises(_native.NativeError):
        relations.relate(lab.cpu(), xyz)
    with pytest.raises(_native.NativeError):
        relations.relate(lab, xyz[:, :2])


def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_relations_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out0, ref0, objs0 = O.segment_objects(sample, net, net_crop)
    np.random.seed(3)
    out1, ref1, objs1, res = O.segment_objects(sample, net, net_crop, relations=True, relations_args=dict(connectivity=8))
    assert torch.equal(out0, out1) and ref0 is not None and torch.equal(ref0, ref1)
    assert torch.equal(objs0.centroid, objs1.centroid) and torch.equal(objs0.points, objs1.points)
    lab, xyz = ref1[0].numpy().astype(np.int32), sample["depth"][0].numpy()
    want = R.relations(lab, xyz[2], 8, 15, 8)
    check_frame(host(res, 0), want, "demo")
    present = np.nonzero(want["pixels"])[0]
    assert len(present) >= 1 and np.array_equal(present, objs1.label.cpu().numpy())
    assert sorted(relations.pick_order(res)) == present.tolist()
    np.random.seed(3)
    both = O.segment_objects(sample, net, net_crop, plane=True, relations=True, relations_args=dict(connectivity=8))
    assert len(both) == 5 and hasattr(both[3], "normal") and torch.equal(both[4].front, res.front)
