"""uoc_objects and steps C and D of uoc_support_plane / uoc_support_planes on the engineered cases of tests/stats_cases.py.

Every case is tier 1 (exact in every summation order: the expected float32 comes from integer arithmetic, rounded once to
float64 and once to float32) or tier 2 (an irrational value at least 2^-40 from a float32 rounding boundary), so every
float field is compared with np.array_equal and no object, no plane and no field is exempt; tests/test_stats_cases_host.py
proves on the CPU that each case is what it is named for and that the comparisons reject the listed mutants.  The exceptions
are stated in stats_cases.plane_scene: on the two tilted planes a brick is held to exact heights and, like every record
here, to the gap-independent checker that check_against_reference and check_frame now run.

Each case is laid into a 72x128 frame (two 4096-pixel blocks and one 1024-pixel wave) and a 5x13 frame (one wave and one
lane) in three placements: contiguous from pixel 0, straddling the block and wave borders, and scattered by a seeded
permutation among the other ids, invalid depths (0, NaN, inf, negative) and background ids (0, 128, -1).  The ids include
1, 63, 64 and 127.  The three placements run as one batch of three frames and each frame again alone: the float fields
must be the same bits across placements, and every field the same bits in the batch and alone.

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import faulthandler
import sys

import numpy as np
import pytest
import torch

from tests import placement_reference
from tests import stats_cases as S
from tests import support_reference as R
from tests.test_objects_gpu import check_against_reference
from tests.test_support_gpu import check_frame, host
from unseenobjectclustering_amd import objects as O
from unseenobjectclustering_amd import support

pytestmark = pytest.mark.gpu
OBJECT_KEYS = ("pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes", "obb_center", "obb_half")
OBJECT_FLOATS = OBJECT_KEYS[3:]
NUM_HYP, TAU_MM = 16, 10


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def to_dev(device, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrs]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def records(objs):
    """(frame, id) -> {field: value} of an ObjectSet; `eig` names the eigenvalues as the expectations do."""
    f = {k: getattr(objs, k).cpu().numpy() for k in OBJECT_KEYS}
    keys = zip(objs.frame.cpu().tolist(), objs.label.cpu().tolist())
    return {key: dict({k: f[k][i] for k in OBJECT_KEYS}, eig=f["eigenvalues"][i]) for i, key in enumerate(keys)}


@pytest.mark.parametrize("group", list(S.object_groups()))
def test_object_cases_are_exact_in_every_placement(device, group):
    lab, xyz, want = S.object_group_frames(group)
    members = S.object_groups()[group][1]
    dl, dx = to_dev(device, lab, xyz)
    objs = O.extract_objects(dl, dx, min_points=0)
    check_against_reference(objs, lab, xyz)                 # the old tolerances and the checker on every record
    rec = records(objs)
    for b, placement in enumerate(S.PLACEMENTS):
        for l, name, translated in members:
            S.assert_object_exact(rec[(b, l)], want[l], (group, placement, name, translated))
            for k in OBJECT_FLOATS + ("count",):
                assert np.array_equal(bits(rec[(b, l)][k]), bits(rec[(0, l)][k])), (group, placement, name, k)
    # a translation by a dyadic offset moves centroid, AABB and box centre by exactly the offset and nothing else
    base = {name: l for l, name, translated in members if not translated}
    off = np.array(S.OFFSET, np.float64) * 2.0 ** -S.LATTICE_EXP
    for l, name, translated in members:
        if translated:
            a, t = rec[(0, base[name])], rec[(0, l)]
            for k in ("cov", "eigenvalues", "axes", "obb_half"):
                assert np.array_equal(bits(a[k]), bits(t[k])), (group, name, k)
            for k in ("centroid", "aabb_min", "aabb_max", "obb_center"):
                assert np.array_equal(t[k].astype(np.float64), a[k].astype(np.float64) + off), (group, name, k)
    # batch independence: every frame alone gives the bits it gave among the others
    for b, placement in enumerate(S.PLACEMENTS):
        alone = records(O.extract_objects(dl[b:b + 1].contiguous(), dx[b:b + 1].contiguous(), min_points=0))
        assert sorted(l for _, l in alone) == sorted(l for f, l in rec if f == b)
        for (_, l), r in alone.items():
            for k in OBJECT_KEYS:
                assert np.array_equal(bits(r[k]), bits(rec[(b, l)][k])), (group, placement, l, k)


@pytest.mark.parametrize("tiny", [False, True], ids=["72x128", "5x13"])
@pytest.mark.parametrize("name", S.PLANE_NAMES)
def test_plane_scenes_are_exact_in_every_placement(device, name, tiny):
    sc = S.plane_scene(name, tiny)
    frames = [S.plane_scene_frame(name, tiny, placement) for placement in S.PLACEMENTS]
    labs, xyzs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    dl, dx = to_dev(device, labs, xyzs)
    fields = support.PLANE_FIELDS + support.OBJECT_FIELDS
    for seed in S.PLANE_SEEDS:
        kw = dict(num_hyp=NUM_HYP, tau=TAU_MM / 1000.0, seed=seed, height_map=True)
        whole = support.fit_plane(dl, dx, **kw)
        first = host(whole, 0)
        for b, placement in enumerate(S.PLACEMENTS):
            where = (name, tiny, seed, placement)
            got = host(whole, b)
            want = R.fit(labs[b], xyzs[b], NUM_HYP, TAU_MM, seed, height_map=True)
            check_frame(got, want, where)                   # integers, the old tolerances and the checker on every record
            nondeg = np.nonzero(want["scores"] >= 0)[0]
            assert int(got["found"]) == 1 and int(got["inliers"]) == int(got["candidates"]) == len(sc["background"]), where
            assert int(got["hyp"]) == int(nondeg[0]) and np.all(want["scores"][nondeg] == len(sc["background"])), where
            S.assert_plane_exact(got, sc, where)
            for k in fields:
                if k != "hyp":                              # which hypothesis comes first depends on the raster order
                    assert np.array_equal(bits(got[k]), bits(first[k])), (where, k)
            alone = support.fit_plane(dl[b], dx[b], **kw)
            for k in fields + ("height",):
                assert torch.equal(getattr(alone, k)[0].view(torch.int32), getattr(whole, k)[b].view(torch.int32)), (where, k)
        if name == "frontal":
            flat = placement_reference.flat_plane()
            for k in ("normal", "d", "centroid", "u", "v"):
                assert np.array_equal(first[k].reshape(np.shape(flat[k])), flat[k]), (name, k)
            # uoc_support_planes runs the same kernels with (frame, plane) as the batch: round 0 bit for bit
            res = support.fit_planes(dl, dx, max_planes=2, num_hyp=NUM_HYP, tau=TAU_MM / 1000.0, min_inliers=3, seed=seed)
            assert torch.equal(res.records[:, 0], whole.records), (name, tiny, seed)
            zero = res.plane(0)
            for k in support.OBJECT_FIELDS:
                assert torch.equal(getattr(zero, k).view(torch.int32), getattr(whole, k).view(torch.int32)), (name, tiny, seed, k)


@pytest.mark.parametrize("H,W,ids", [(24, 32, "all"), (48, 64, "gaps")])
def test_seeded_small_scenes_pass_the_checker(device, H, W, ids):
    """The seeded scenes on which tests/test_stats_cases_host.py holds the reference to the checker: small objects whose
    covariance is rank-deficient or nearly so, where a Jacobi rotation can leave an eigenvalue of -1e-20."""
    from tests.test_objects_gpu import synthetic
    lab, xyz, _ = synthetic(2, H, W, seed=H * 7 + W, ids=ids)
    dl, dx = to_dev(device, lab, xyz)
    objs = O.extract_objects(dl, dx, min_points=0)
    K, _ = check_against_reference(objs, lab, xyz)
    assert K > 100 and float(objs.eigenvalues.min()) >= 0.0
