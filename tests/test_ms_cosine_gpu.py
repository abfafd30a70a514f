"""The cosine clustering kernels (csrc/meanshift.hip) through the C ABI, stage by stage, against the float64 restatement
tests/ms_cosine_reference.py.

Decisions (farthest-point sampling, seed components, assignment, the swap, the whole call without iterations) run on inputs
whose fp32 arithmetic is exact in every summation order (tests/ms_cosine_cases.py; proved on the CPU in
test_ms_cosine_host.py): every integer is compared exactly, no pixel is exempt.  Hill climbing is compared with float64
under a tolerance measured per case: K_CLIMB x the larger deviation from float64 of two other fp32 evaluations (the torch
oracle and a 16-pixel-tile summation).  profiles/ms_cosine_error.md holds the measured deviations; one lost or repeated pixel
moves every case by at least 10 x its tolerance (test_ms_cosine_host.py)."""
import numpy as np
import pytest
import torch

from tests import ms_cosine_cases as CS
from tests import ms_cosine_reference as R
from tests.golden.cases import EPSILON, KAPPA
from tests.ms_stage_calls import assign_raw, both_sampling_kernels, components_raw, hill_climb_raw, select_raw, to_dev
from unseenobjectclustering_amd import _native
from unseenobjectclustering_amd.utils import mean_shift as MS

pytestmark = pytest.mark.gpu
assert KAPPA == CS.KAPPA


# ---- the stage entry points (tests/ms_stage_calls.py; the metric defaults to cosine) ---------------------------------------
# ---- 3a. hill climbing against float64 ---------------------------------------------------------------------------------
def climb_rows(what, got, fields, seeds, iters, check=None):
    """Per checked field: (name, kernel deviation from float64, the oracle's, the tile order's, the tolerance)."""
    rows = []
    for b in (range(len(fields)) if check is None else check):
        ref, dev_o, dev_t = CS.climb_yardstick(fields[b], seeds[b], KAPPA, iters)
        err = float(np.abs(got[b].astype(np.float64) - ref).max())
        rows.append((what if len(fields) == 1 else "%s field %d" % (what, b), err, dev_o, dev_t, CS.climb_tolerance(dev_o, dev_t)))
    return rows


def run_climb(device, what, fields, seeds, iters, check=None):
    got = hill_climb_raw(to_dev(np.stack(fields), device), to_dev(np.stack(seeds), device), iters).cpu().numpy()
    assert np.isfinite(got).all()
    return climb_rows(what, got, fields, seeds, iters, check)


def tile_case(device, m, iters):
    X = CS.hc_field(1961)
    return run_climb(device, "n 1961 m %d iters %d" % (m, iters), [X], [CS.hc_seeds(X, m)[0]], iters)


def edge_case(device, n, m):
    fields = [CS.hc_field(n, seed=1 + k) for k in range(3 if n == 4097 else 1)]
    return run_climb(device, "n %d m %d" % (n, m), fields, [CS.hc_seeds(X, m, k)[0] for k, X in enumerate(fields)], 10)


def strided_case(device):
    batch, n, m = CS.HC_STRIDED
    fields = [CS.hc_field(n, seed=100 + b) for b in range(batch)]
    return run_climb(device, "batch %d n %d" % (batch, n), fields, [CS.hc_seeds(X, m, b)[0] for b, X in enumerate(fields)], 10)


def affine_case(device):
    batch, n, m, check = CS.HC_AFFINE
    fields = [CS.hc_affine_field(b) for b in range(batch)]
    return run_climb(device, "batch %d n %d" % (batch, n), fields, [CS.hc_seeds(X, m, b)[0] for b, X in enumerate(fields)], 10, check)


def wide_case(device, n, m):
    X = CS.hc_field(n, seed=7, channels=128)
    Xd = MS.to_planes(to_dev(X, device)[None])
    _, idx, Z, _ = MS.cluster_batch(Xd, [CS.WIDE_FIRST], KAPPA, m, 10, EPSILON, return_parts=True, metric="cosine")
    torch.cuda.synchronize(device)
    idx = idx[0].cpu().numpy()
    assert idx[0] == CS.WIDE_FIRST and idx.min() >= 0 and idx.max() < n
    got = Z[0].permute(1, 0, 2).reshape(m, 128).cpu().numpy()
    return climb_rows("128-d n %d m %d" % (n, m), [got], [X], [X[idx]], 10)


def climb_cases():
    """Every 3a case: name -> function(device) -> rows.  scripts/ms_cosine_error.py prints them all."""
    out = {}
    for iters in CS.HC_TILE_ITERS:
        for m in CS.HC_TILE_M:
            out["tile m%d iters%d" % (m, iters)] = lambda device, m=m, iters=iters: tile_case(device, m, iters)
    for m in CS.HC_EDGE_M:
        for n in CS.HC_EDGE_N + [4097]:
            out["edge n%d m%d" % (n, m)] = lambda device, n=n, m=m: edge_case(device, n, m)
    out["strided"] = strided_case
    out["affine"] = affine_case
    for n, m in CS.HC_WIDE:
        out["wide n%d m%d" % (n, m)] = lambda device, n=n, m=m: wide_case(device, n, m)
    return out


def assert_rows(rows):
    for name, err, dev_o, dev_t, tol in rows:
        print("%-32s kernel %.3e  oracle %.3e  tiles %.3e  ratio %.2f  (K = %g)" % (name, err, dev_o, dev_t, err / max(dev_o, dev_t), CS.K_CLIMB))
    for name, err, dev_o, dev_t, tol in rows:
        assert err <= tol, "%s: %.3e from float64, allowed %.3e = %g x max(oracle %.3e, tiles %.3e)" % (name, err, tol, CS.K_CLIMB, dev_o, dev_t)


@pytest.mark.parametrize("iters", CS.HC_TILE_ITERS)
@pytest.mark.parametrize("m", CS.HC_TILE_M)
def test_climb_every_seed_tile_count(device, m, iters):
    """hc_iter_flat_kernel<ST, QUAD> for ST = 1..8, QUAD where the last seed tile holds 1..4 seeds (m = 16k + 2), not QUAD at
    16k + 9, and the full-tile boundaries 16k: n = 37 x 53, one and ten iterations."""
    assert_rows(tile_case(device, m, iters))


@pytest.mark.parametrize("m", CS.HC_EDGE_M)
@pytest.mark.parametrize("n", CS.HC_EDGE_N + [4097])
def test_climb_pixel_count_edges(device, n, m):
    """One partial tile, waves without a tile, the step from one virtual block to two at 1024 | 1025; n = 4097 as three fields."""
    assert_rows(edge_case(device, n, m))


def test_climb_more_items_than_blocks(device):
    """300 fields of 144 pixels: the strided item walk; every field against its own float64 run."""
    rows = strided_case(device)
    assert len(rows) == CS.HC_STRIDED[0]
    assert_rows(rows)


def test_climb_two_virtual_blocks_per_field(device):
    """256 fields of 2048 pixels (two virtual blocks each, 512 items): neighbours point opposite ways, so a seed fragment or a
    pixel tile of the wrong field is an O(1) error."""
    rows = affine_case(device)
    assert len(rows) == 5
    assert_rows(rows)


@pytest.mark.parametrize("n,m", CS.HC_WIDE)
def test_climb_128d(device, n, m):
    """hc_iter_kernel (two planes) through the whole call: the returned Z against the float64 climb from the returned indices."""
    assert_rows(wide_case(device, n, m))


@pytest.mark.parametrize("n", CS.HC_OVERREAD_N)
def test_climb_reads_no_row_beyond_n(device, n):
    """The field inside a larger buffer whose rows from n on are (a) the opposite of the field's dominant direction, (b) seed 0
    itself, which a kernel that read them would weigh e^20: bit for bit the result of the tight buffer."""
    m = 100
    X = CS.hc_field(n, seed=7)
    Z0 = to_dev(CS.hc_seeds(X, m)[0][None], device)
    tight = hill_climb_raw(to_dev(X[None], device), Z0, 10)
    mean = X.astype(np.float64).sum(axis=0)
    for fill in (-(mean / np.linalg.norm(mean)), CS.hc_seeds(X, m)[0][0]):
        buf = np.empty((1, n + 2048, 64), np.float32)
        buf[0, :n] = X
        buf[0, n:] = fill.astype(np.float32)
        got = hill_climb_raw(to_dev(buf, device), Z0, 10, n=n)
        assert torch.equal(got, tight)
    assert torch.isfinite(tight).all() and not torch.equal(tight, Z0)


# ---- 3b. farthest-point sampling, exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CS.fps_cases()))
def test_sampling_exact_ties(device, name):
    """Exact ties between pixels of one 16-lane row group, of two waves, of two blocks of either kernel: the lower index."""
    c = CS.fps_cases()[name]
    want, _ = R.select_seeds(c["X"], c["m"], c["first"])

    def check(kernel):
        idx, seeds = select_raw(device, c["X"][None], c["m"], [c["first"]])
        assert np.array_equal(idx[0], want), kernel
        assert np.array_equal(seeds[0], R.seed_rows(c["X"], want)), kernel
    both_sampling_kernels(check)


@pytest.mark.parametrize("name", list(CS.fps_continuation_cases()))
def test_sampling_continuation_exact(device, name):
    c = CS.fps_continuation_cases()[name]
    want, _ = R.select_seeds(c["X"], c["m"], None, c["init"], c["num_init"])

    def check(kernel):
        idx, seeds = select_raw(device, c["X"][None], c["m"], None, c["init"][None], c["num_init"])
        assert np.array_equal(idx[0], want), kernel
        assert np.array_equal(seeds[0], R.seed_rows(c["X"], want, c["init"])), kernel
    both_sampling_kernels(check)


def test_sampling_batch_exact(device):
    c = CS.fps_batch_case()
    want = [R.select_seeds(c["X"][b], c["m"], c["first"][b])[0] for b in range(3)]

    def check(kernel):
        idx, seeds = select_raw(device, c["X"], c["m"], c["first"])
        for b in range(3):
            assert np.array_equal(idx[b], want[b]), (kernel, b)
            assert np.array_equal(seeds[b], R.seed_rows(c["X"][b], want[b])), (kernel, b)
    both_sampling_kernels(check)


# ---- 3c. seed components, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [CS.EPS_EXACT, CS.EPS_PRODUCT])
@pytest.mark.parametrize("name", list(CS.cc_cases()))
def test_components_exact(device, name, eps):
    """Pairs exactly at eps are members (<=); the mode of the labels present, ties to the smallest; members are overwritten."""
    Z, _ = CS.cc_cases()[name]
    want, _ = R.seed_components(Z, eps)
    got, nu = components_raw(device, Z[None], eps)
    assert np.array_equal(got[0], want) and nu[0] == len(np.unique(want))


@pytest.mark.parametrize("m", [m for m in CS.CC_M if m > 5])
def test_components_batch_exact(device, m):
    Zb = np.stack([CS.cc_chain(m, "low", "tied"), CS.cc_chain(m, "high", "majority"), CS.cc_chain(m, "high", "tied")])
    got, nu = components_raw(device, Zb, CS.EPS_EXACT)
    for b in range(3):
        want, _ = R.seed_components(Zb[b], CS.EPS_EXACT)
        assert np.array_equal(got[b], want) and nu[b] == len(np.unique(want)), b


# ---- 3d. assignment and the swap, exact ------------------------------------------------------------------------------------
def check_assignment(device, X, Z, sl, nu):
    """Batched inputs through both calls: closest and labels exact against the reference, the confidence call's equal."""
    (la, ca), (lc, cc) = assign_raw(device, X, Z, sl, nu)
    for b in range(X.shape[0]):
        labels, closest, _ = R.assign(X[b], Z[b], sl[b], nu[b])
        assert np.array_equal(ca[b], closest), "closest, field %d" % b
        assert np.array_equal(la[b], labels), "labels, field %d" % b
    assert np.array_equal(lc, la) and np.array_equal(cc, ca), "uoc_ms_confidence differs from uoc_ms_assign"


@pytest.mark.parametrize("n", CS.ASSIGN_N)
@pytest.mark.parametrize("m", CS.ASSIGN_M)
def test_assignment_exact_ties(device, m, n):
    """A pixel equidistant from two seeds of one 16-seed tile, of two tiles on one lane, of two tiles and lanes, in every pixel
    slot of a lane: the lower seed.  Three fields: the pixels rotated, the seed labels shifted."""
    Z = CS.assign_seeds(m)
    sl, nu = CS.assign_labels(m)
    X = CS.assign_pixels(n)
    Xb = np.stack([np.roll(X, b, axis=0) for b in range(3)])
    slb = np.stack([(sl + b) % nu for b in range(3)]).astype(np.int32)
    check_assignment(device, Xb, np.stack([Z] * 3), slb, [nu] * 3)


@pytest.mark.parametrize("m", CS.PAD_M)
def test_assignment_padding_rows_never_win(device, m):
    """Every real seed is farther than 1/2 from every pixel: a zero padding row of the last seed tile, unmasked, would win."""
    X, Z = CS.padding_case(m)
    sl = (np.arange(m) % 3).astype(np.int32)
    (la, ca), _ = assign_raw(device, X[None], Z[None], sl[None], [len(np.unique(sl))])
    assert ca.min() >= 0 and ca.max() < m
    check_assignment(device, X[None], Z[None], sl[None], [len(np.unique(sl))])


@pytest.mark.parametrize("name", list(CS.swap_cases()))
def test_swap_exact(device, name):
    """The largest cluster becomes 0: equal counts (the first wins), a largest label that is not 0, labels with a gap."""
    X, Z, sl, nu = CS.swap_cases()[name]
    check_assignment(device, X[None], Z[None], sl[None], [nu])


# ---- 3e. the whole call on exact inputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,wide,batch", CS.WHOLE)
def test_whole_call_exact(device, n, m, wide, batch):
    """No iteration: the seeds stay rows of the field, so sampling, components, assignment and swap are all exact."""
    fields = [CS.whole_field(n, k, wide) for k in range(batch)]
    firsts = [(37 * k + 11) % n for k in range(batch)]
    Xd = to_dev(np.stack(fields), device)
    labels, idx, Z, sl = MS.cluster_batch(MS.to_planes(Xd) if wide else Xd, firsts, KAPPA, m, 0, EPSILON, return_parts=True,
                                          metric="cosine")
    torch.cuda.synchronize(device)
    for k in range(batch):
        wl, wi, _, ws = R.cluster(fields[k], KAPPA, m, 0, EPSILON, firsts[k])
        assert np.array_equal(idx[k].cpu().numpy(), wi), "indices, field %d" % k
        rows = fields[k][wi]
        assert np.array_equal(Z[k].cpu().numpy(), R.planes(rows) if wide else rows), "Z, field %d" % k
        assert np.array_equal(sl[k].cpu().numpy(), ws), "seed labels, field %d" % k
        assert np.array_equal(labels[k].cpu().numpy(), wl), "labels, field %d" % k


# ---- 3f. the pixel no seed wins ------------------------------------------------------------------------------------------------
def confidence_all(device, X, Z, sl, nu, halves):
    """uoc_ms_confidence with all five outputs on one field, X [n, 64] or planes [2, n, 64] -> numpy arrays."""
    L = _native.lib()
    Xd, Zd = to_dev(X[None], device), to_dev(Z[None], device)
    sld, nud = to_dev(np.asarray(sl, np.int32)[None], device), to_dev(np.asarray([nu], np.int32), device)
    n, m = X.shape[-2], Z.shape[-2]
    labels, second, closest, rival = (torch.full((1, n), -7, dtype=torch.int32, device=device) for _ in range(4))
    margin = torch.full((1, n), -7.0, device=device)
    nws = L.uoc_ms_confidence_workspace_bytes(1, n, m, halves)
    cws = torch.empty(nws, dtype=torch.uint8, device=device)
    _native.call("uoc_ms_confidence", device, Xd, halves, 1, n, Zd, sld, nud, m, 0, labels, margin, second, closest, rival, cws, nws)
    return [t[0].cpu().numpy() for t in (labels, margin, second, closest, rival)]


@pytest.mark.parametrize("n,m,wide", CS.NOSEED)
def test_pixel_no_seed_wins(device, n, m, wide):
    """A non-finite row compares below no distance: label 0, counted under label 0, closest = INT_MAX; margin 1, second and
    rival -1.  Every other pixel as the float64 restatement has it on the finite rows, and both calls agree on every pixel.
    uoc_ms_assign has no 128-d form: the 128-d field goes through uoc_ms_confidence (two planes) and must reproduce what
    uoc_ms_assign gives on the 64-d field it was widened from (widening keeps every dot product)."""
    X, Z, sl, nu = CS.noseed_case(n, m, wide)
    X64, Z64, _, _ = CS.noseed_case(n, m, False)
    bad = list(CS.noseed_rows(n))
    fin = np.setdiff1d(np.arange(n), bad)
    (la, ca), _ = assign_raw(device, X64[None], Z64[None], sl[None], [nu])
    lc, margin, second, cc, rival = confidence_all(device, R.planes(X) if wide else X, R.planes(Z) if wide else Z, sl, nu,
                                                   2 if wide else 1)
    for labels, closest in ((la[0], ca[0]), (lc, cc)):
        assert (labels[bad] == 0).all() and (closest[bad] == 2147483647).all()
    assert (margin[bad] == 1.0).all() and (second[bad] == -1).all() and (rival[bad] == -1).all()
    want_labels, want_closest, _ = R.assign(X64[fin], Z64, sl, nu)
    for labels, closest in ((la[0], ca[0]), (lc, cc)):
        assert np.array_equal(closest[fin], want_closest) and np.array_equal(labels[fin], want_labels)
    assert np.array_equal(lc, la[0]) and np.array_equal(cc, ca[0]), "uoc_ms_confidence differs from uoc_ms_assign"
    assert (margin[fin] > 0).all() and (second[fin] == 1 - want_labels).all()
