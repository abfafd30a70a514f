"""uoc_support_planes / support.fit_planes on the GPU against the numpy restatement (tests/planes_reference.py).

The rounds are exact integers: count, found, candidates, inliers, hyp, round_candidates, removed, the object counts and
the whole index map are compared with np.array_equal.  Refinement and objects are fp64 sums stored in fp32: every plane
slot goes through tests/test_support_gpu.py's check_frame (its tolerances, under its eigen-gap condition, and, without
exemption, the gap-independent checker of tests/stats_cases.py on every found plane and every object with a point, and
the comparison of the step C and D sums with the reference within half an ulp plus derived terms; the sign rule alone is
judged only where the float32 record decides it, see tests/test_support_gpu.py); cos0 and
offset0 within 2e-6 and extent within 1e-5 where the planes involved meet the gap condition.  Round 0 is compared bit for
bit with support.fit_plane.

The scenes live in the reference module and tests/test_planes_host.py asserts on the CPU that they contain what they are
used for here.  Every GPU test runs under a watchdog, as in tests/test_support_gpu.py; nothing is retried."""
import faulthandler
import functools
import sys

import numpy as np
import pytest
import torch

from tests import planes_reference as P
from tests import support_reference as R
from tests.test_support_gpu import check_frame
from unseenobjectclustering_amd import _native, normals, placement, support

pytestmark = pytest.mark.gpu
EINVAL = -22
BANDS = ((3, 6), (10, 20), (10, 10))
KS = (1, 2, 4, 8)
OBJ_FIELDS = tuple(k for k in support.OBJECT_FIELDS if k != "count")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def shelves(H, W, seed, back=False):
    lab, xyz, _ = P.shelves(H, W, seed, 0.7, True) if back else P.shelves(H, W, seed)
    return lab, xyz


@functools.lru_cache(maxsize=None)
def named(name):
    if name == "stairs":
        return P.stairs()
    if name == "pair":
        return P.parallel_pair()
    if name in P.STOPS:
        return P.STOPS[name]()
    return R.ENGINEERED[name]()


@functools.lru_cache(maxsize=None)
def reference(key, K, num_hyp, tau_mm, rem_mm, min_inliers, seed):
    lab, xyz = shelves(*key[1:]) if key[0] == "shelves" else named(key[1])
    return P.fit(lab, xyz, K, num_hyp, tau_mm, rem_mm, min_inliers, seed)


def to_dev(device, lab, xyz):
    return torch.from_numpy(np.ascontiguousarray(lab)).to(device), torch.from_numpy(np.ascontiguousarray(xyz)).to(device)


def plane_host(res, b, r):
    """Slot r of frame b in the layout check_frame reads."""
    f = {k: getattr(res, k)[b, r].cpu().numpy() for k in support.PLANE_FIELDS + OBJ_FIELDS}
    f["count"] = res.obj_count[b, r].cpu().numpy()
    f["height"] = None
    return f


def check_planes(res, b, want, where):
    """Frame b of a PlanesResult against P.fit(...).  Returns (planes found, planes with their gap ok, objects, objects ok)."""
    K = len(want["planes"])
    assert int(res.count[b]) == want["count"], (where, int(res.count[b]), want["count"])
    assert np.array_equal(res.index[b].cpu().numpy(), want["index"]), where
    gap_ok, objects, objects_ok = [], 0, 0
    for r in range(K):
        ok, n, n_ok = check_frame(plane_host(res, b, r), dict(plane=want["planes"][r], objects=want["objects"][r], height=None),
                                  (where, r))
        gap_ok.append(bool(ok))
        objects += n
        objects_ok += n_ok
        wi = want["info"][r]
        assert int(res.round_candidates[b, r]) == wi["round_candidates"] and int(res.removed[b, r]) == wi["removed"], (where, r)
        cos0, off0, ext = float(res.cos0[b, r]), float(res.offset0[b, r]), res.extent[b, r].cpu().numpy()
        if not want["planes"][r]["found"]:
            assert cos0 == 0.0 and off0 == 0.0 and not np.any(ext), (where, r)
            continue
        print(where, r, "cos0 err", abs(cos0 - wi["cos0"]), "offset0 err", abs(off0 - wi["offset0"]), "extent err",
              float(np.abs(ext - wi["extent"]).max()), "gap ok", ok)
        if ok and gap_ok[0]:
            assert abs(cos0 - wi["cos0"]) <= 2e-6 and abs(off0 - wi["offset0"]) <= 2e-6, (where, r, cos0, off0, wi)
        if ok:
            assert np.abs(ext - wi["extent"]).max() <= 1e-5, (where, r, ext, wi["extent"])
    return want["count"], sum(gap_ok), objects, objects_ok


SHELF_COMBOS = {(24, 32): [(K, t, r, s) for K in KS for t, r in BANDS for s in (1, 2)],
                (48, 64): [(K, t, r, s) for K in KS for t, r in BANDS for s in (1, 2)][::2],
                (61, 83): [(K, t, r, s) for K in KS for t, r in BANDS for s in (1, 2)][1::2],
                (120, 160): [(4, 10, 20, 1), (2, 3, 6, 2), (8, 10, 10, 1), (1, 3, 6, 1)]}


@pytest.mark.parametrize("H,W", list(SHELF_COMBOS))
def test_shelves_match_reference(device, H, W):
    mi = P.default_min_inliers(H, W)
    tot = np.zeros(4, np.int64)
    labs, xyzs = zip(*(shelves(H, W, s) for s in (1, 2)))
    dl, dx = to_dev(device, np.stack(labs), np.stack(xyzs))
    for K, tau_mm, rem_mm, seed in SHELF_COMBOS[(H, W)]:
        res = support.fit_planes(dl, dx, max_planes=K, num_hyp=256, tau=tau_mm / 1000.0, remove=rem_mm / 1000.0, seed=seed)
        assert res.count.dtype == res.index.dtype == torch.int32 and res.normal.shape == (2, K, 3)
        assert res.half.shape == (2, K, 128, 3) and res.records.shape == (2, K, 21) and res.extent.shape == (2, K, 4)
        assert res.min_inliers == mi and res.rem_mm == rem_mm
        for b, scene_seed in enumerate((1, 2)):
            want = reference(("shelves", H, W, scene_seed), K, 256, tau_mm, rem_mm, mi, seed)
            assert want["count"] == min(K, 3)
            tot += check_planes(res, b, want, (H, W, scene_seed, K, tau_mm, rem_mm, seed))
    assert 2 * tot[1] >= tot[0] > 0 and 2 * tot[3] >= tot[2] > 0, tot


def test_vga_frame_matches_reference(device):
    lab, xyz = shelves(480, 640, 1)
    dl, dx = to_dev(device, lab, xyz)
    res = support.fit_planes(dl, dx, max_planes=4, num_hyp=64, tau=0.010, seed=1)
    want = reference(("shelves", 480, 640, 1), 4, 64, 10, 20, P.default_min_inliers(480, 640), 1)
    found, ok, objects, objects_ok = check_planes(res, 0, want, "vga")
    assert found == 3 and 2 * ok >= found and 2 * objects_ok >= objects > 0


NAMED = ("stairs", "pair") + tuple(P.STOPS) + tuple(R.ENGINEERED)


@pytest.mark.parametrize("name", NAMED)
def test_named_scenes_match_reference(device, name):
    lab, xyz = named(name)
    dl, dx = to_dev(device, lab, xyz)
    combos = [(K, t, r, s, 3) for K in KS for t, r in BANDS for s in (1, 2)]
    if name in ("stairs", "pair") or name in P.STOPS:
        combos += [(2, 10, 20, 0xFFFFFFFF, 3), (8, 3, 6, 0xFFFFFFFF, 3)]               # round 1 hashes with seed 0
        top = reference(("named", name), 1, 64, 3, 6, 3, 1)["planes"][0]["inliers"]
        combos += [(4, 3, 6, 1, top), (4, 3, 6, 1, top + 1)]                             # the stop rule at the winning score
    else:
        combos = combos[::3]
    counts = set()
    for K, tau_mm, rem_mm, seed, mi in combos:
        res = support.fit_planes(dl, dx, max_planes=K, num_hyp=64, tau=tau_mm / 1000.0, remove=rem_mm / 1000.0, min_inliers=mi,
                                 seed=seed)
        want = reference(("named", name), K, 64, tau_mm, rem_mm, mi, seed)
        check_planes(res, 0, want, (name, K, tau_mm, rem_mm, seed, mi))
        counts.add(want["count"])
    if name == "stairs":
        assert 8 in counts
    if name in P.STOPS:
        assert counts == {0, 1}
    if name in ("m0", "m2", "collinear", "coincident", "all_objects"):
        assert counts == {0}


ANCHORS = [("tabletop", 61, 83), ("tabletop", 24, 32)] + [("engineered", n) for n in R.ENGINEERED]


@pytest.mark.parametrize("key", ANCHORS, ids=lambda k: "-".join(str(x) for x in k))
def test_round_zero_is_fit_plane_bit_for_bit(device, key):
    lab, xyz = R.tabletop(key[1], key[2], 1) if key[0] == "tabletop" else R.ENGINEERED[key[1]]()
    dl, dx = to_dev(device, lab, xyz)
    found = 0
    for num_hyp, tau_mm, seed in ((256, 10, 1), (64, 3, 2), (1, 10, 7)):
        one = support.fit_plane(dl, dx, num_hyp=num_hyp, tau=tau_mm / 1000.0, seed=seed)
        found += int(one.found[0])
        for K, rem_mm in ((1, tau_mm), (4, 2 * tau_mm), (8, 1000)):
            res = support.fit_planes(dl, dx, max_planes=K, num_hyp=num_hyp, tau=tau_mm / 1000.0, remove=rem_mm / 1000.0,
                                     min_inliers=3, seed=seed)
            assert torch.equal(res.records[:, 0], one.records), (key, num_hyp, tau_mm, seed, K)
            first = res.plane(0)
            assert torch.equal(first.records, one.records) and first.height is None and first.records.is_contiguous()
            for k in support.OBJECT_FIELDS:
                assert torch.equal(getattr(first, k).view(torch.int32), getattr(one, k).view(torch.int32)), (key, k, K)
    if key[0] == "tabletop":
        assert found >= 2


def _bits(res):
    out = {k: getattr(res, k) for k in ("count", "records", "info", "index", "_objs")}
    return {k: v.view(torch.int32) for k, v in out.items()}


def test_deterministic_and_batch_independent(device):
    frames = [shelves(24, 32, 1), P.parallel_pair(24, 32), P.stairs(24, 32), P.grid_plane(24, 32), R.case_m0(24, 32),
              shelves(24, 32, 2)]
    labs, xyzs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    dl, dx = to_dev(device, labs, xyzs)
    kw = dict(max_planes=8, num_hyp=128, tau=0.003, min_inliers=15, seed=5)
    whole = support.fit_planes(dl, dx, **kw)
    assert len(set(whole.count.cpu().tolist())) >= 4
    again = support.fit_planes(dl, dx, **kw)
    for k, v in _bits(whole).items():
        assert torch.equal(v, _bits(again)[k]), ("rerun", k)
    order = [4, 2, 0, 5, 3, 1]
    other = support.fit_planes(dl[order], dx[order], **kw)
    for b in range(len(frames)):
        alone = support.fit_planes(dl[b], dx[b], **kw)
        for k, v in _bits(whole).items():
            assert torch.equal(v[b:b + 1], _bits(alone)[k]), ("alone", b, k)
            assert torch.equal(v[b], _bits(other)[k][order.index(b)]), ("mates", b, k)


def test_labels_dtypes_and_unbatched_input(device):
    lab, xyz = shelves(48, 64, 1)
    rng = np.random.default_rng(0)
    mixed = lab.copy()
    mixed[lab == 0] = rng.choice(np.array([0, 128, -1, 1000], np.int32), size=int((lab == 0).sum()))
    dl, dx = to_dev(device, lab, xyz)
    a = support.fit_planes(dl[None], dx[None], num_hyp=64)
    index = a.index[0].cpu().numpy()
    assert (index[lab > 0] == -2).all() and (index[lab == 0] >= -1).sum() > 0 and int(a.count[0]) == 3
    dm = torch.from_numpy(mixed).to(device)
    for other in (support.fit_planes(dl, dx, num_hyp=64), support.fit_planes(dl.float(), dx, num_hyp=64),
                  support.fit_planes(dl.long()[None], dx.double()[None], num_hyp=64), support.fit_planes(dm, dx, num_hyp=64)):
        for k, v in _bits(a).items():
            assert torch.equal(v, _bits(other)[k]), k
    bare = support.fit_planes(dl, dx, num_hyp=64, objects=False)
    assert torch.equal(bare.records, a.records) and torch.equal(bare.index, a.index) and not bool(bare._objs.any())


def test_error_paths_do_no_device_work(device):
    lib = _native.lib()
    B, H, W, K = 1, 24, 32, 4
    lab, xyz = to_dev(device, *shelves(H, W, 1))
    lab, xyz = lab[None].contiguous(), xyz[None].contiguous()
    nws = lib.uoc_planes_workspace_bytes(B, H, W, 64, K)
    assert nws > 0
    for bad in ((B, H, W, 0, K), (B, H, W, 1025, K), (B, H, W, 64, 0), (B, H, W, 64, 9), (0, H, W, 64, K),
                (B, 1 << 16, 1 << 16, 64, K), (8192, H, W, 64, 8)):
        assert lib.uoc_planes_workspace_bytes(*bad) == 0, bad
    outs = dict(count=torch.full((B,), -7, dtype=torch.int32, device=device),
                planes=torch.full((B, K, support._PW), -7, dtype=torch.int32, device=device),
                info=torch.full((B, K, support._IW), -7, dtype=torch.int32, device=device),
                index=torch.full((B, H, W), -7, dtype=torch.int32, device=device),
                objs=torch.full((B, K, 128, support._OW), -7, dtype=torch.int32, device=device))
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    Pt, st = _native.ptr, _native.stream_ptr(device)

    def call(K_=K, num_hyp=64, tau_mm=10, rem_mm=20, mi=15, nws_=nws, lab_=lab, xyz_=xyz, ws_=ws, **none):
        o = {k: (None if k in none else v) for k, v in outs.items()}
        return lib.uoc_support_planes(Pt(lab_), Pt(xyz_), B, H, W, K_, num_hyp, tau_mm, rem_mm, mi, 1, Pt(o["count"]), Pt(o["planes"]),
                                      Pt(o["info"]), Pt(o["index"]), Pt(o["objs"]), Pt(ws_), nws_, st)

    for kw in (dict(K_=0), dict(K_=9), dict(num_hyp=0), dict(num_hyp=1025), dict(tau_mm=0), dict(tau_mm=1001, rem_mm=1001),
               dict(rem_mm=9), dict(rem_mm=1001), dict(mi=2), dict(nws_=nws - 1), dict(lab_=None), dict(xyz_=None), dict(ws_=None),
               dict(count=1), dict(planes=1), dict(info=1), dict(index=1)):
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == -7).all()), k
    assert call() == 0
    torch.cuda.synchronize()
    assert int(outs["count"][0]) == 3 and int(outs["planes"][0, 0, 0]) == 1
    for kw in (dict(max_planes=0), dict(max_planes=9), dict(num_hyp=0), dict(tau=0.0), dict(remove=0.005), dict(remove=1.5),
               dict(min_inliers=2)):
        with pytest.raises(ValueError):
            support.fit_planes(lab, xyz, **kw)
    with pytest.raises(_native.NativeError):
        support.fit_planes(lab.cpu(), xyz)
    with pytest.raises(_native.NativeError):
        support.fit_planes(lab, xyz[:, :2])


def test_helpers_match_reference(device):
    up = tuple(float(x) for x in R.PLANE_N)
    for key, K in ((("shelves", 61, 83, 1), 4), (("shelves", 61, 83, 1, True), 4), (("shelves", 24, 32, 2), 2)):
        lab, xyz = shelves(*key[1:])
        dl, dx = to_dev(device, lab, xyz)
        H, W = lab.shape
        res = support.fit_planes(dl, dx, max_planes=K, num_hyp=256, seed=1)
        want = reference(key, K, 256, 10, 20, P.default_min_inliers(H, W), 1)
        check_planes(res, 0, want, key)
        for like in (0, 1, up):
            assert support.planes_like(res, like)[0].cpu().tolist() == P.planes_like(want, like), (key, like)
            got = support.standing_on(res, like)
            assert got.dtype == torch.int64 and got.shape == (1, 128)
            assert got[0].cpu().tolist() == P.standing_on(want, like), (key, like)
        assert int(support.choose_support(res)[0]) == P.choose_support(want) == 0
        chosen = support.choose_support(res, up=up)
        assert chosen.dtype == torch.int64 and chosen.shape == (1,) and int(chosen[0]) == P.choose_support(want, up=up)
        picked = res.plane(chosen)
        assert torch.equal(picked.records, res.records[:, int(chosen[0])]) and picked.records.is_contiguous()
        assert torch.equal(picked.height_min, res.height_min[:, int(chosen[0])])
    assert int(chosen[0]) == 0 and P.choose_support(reference(("shelves", 61, 83, 1, True), 4, 256, 10, 20, 101, 1), up=up) == 1


def test_downstream_stages_take_a_plane_of_the_result(device):
    lab, xyz = shelves(61, 83, 1)
    dl, dx = to_dev(device, lab, xyz)
    res = support.fit_planes(dl, dx, max_planes=4, num_hyp=256, seed=1)
    want = reference(("shelves", 61, 83, 1), 4, 256, 10, 20, 101, 1)
    k_board = [k for k in range(3) if want["info"][k]["cos0"] > 0.99 and want["info"][k]["offset0"] > 0.2]
    assert len(k_board) == 1
    board = res.plane(k_board[0])
    a = placement.free_space(dl, dx, board)
    b = placement.free_space(dl, dx, tuple(getattr(board, k)[0].cpu().numpy() for k in ("normal", "d", "centroid", "u", "v")))
    for k in ("state", "owner", "dist2", "cells", "frame"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    cells = a.cells[0].cpu().numpy()
    assert (cells[11:14] > 0).all() and not cells[1:4].any(), cells[:16]
    est = normals.estimate(dx, dl, board)
    assert est is not None
    torch.cuda.synchronize()
