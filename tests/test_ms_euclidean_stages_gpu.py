"""The euclidean clustering kernels (csrc/meanshift.hip, MET = MS_EUCLIDEAN) through the C ABI's metric entry points, stage
by stage, against the float64 restatement tests/ms_euclidean_reference.py.

Decisions (farthest-point sampling in both kernels, seed components, assignment, the swap, the whole call without
iterations) run on inputs whose fp32 arithmetic is exact in every summation order, by the norm expansion and by direct
differences alike (tests/ms_euclidean_cases.py; proved on the CPU in test_ms_euclidean_cases_host.py): every integer is
compared exactly, no pixel, seed or pick is exempt.  In every family rows of different norms take part, so a norm taken from
the wrong pixel slot, seed row, seed tile or 128-d half is a wrong answer.

Hill climbing is compared with float64 under a tolerance measured per case: K_CLIMB x the largest deviation from float64 of
the CPU yardsticks (the reference's code in torch float32 with direct differences; the norm expansion summed in 16-pixel
tiles, in six channel orders; float64 with every squared distance one fp32 ulp off: ms_euclidean_cases.climb_yardstick).
profiles/ms_euclidean_error.md holds the measured deviations; one lost or repeated pixel moves every case by at least 10 x
its tolerance (test_ms_euclidean_cases_host.py).

Which m reaches which instantiation: ST = ceil(m / 16) seed tiles; hc_iter_flat_kernel<ST, QUAD, EUC> is QUAD where ST >= 2 and
the last tile holds 1..4 seeds (m = 16k + 2; 100), not QUAD otherwise (m = 1; 16k + 9; 16k; 89; 96); assign_kernel<ST, 1, EUC>
likewise by ST; 128-d fields run hc_iter_kernel<ST, 2, EUC> and assign_kernel<ST, 2, EUC>."""
import numpy as np
import pytest
import torch

from tests import ms_cosine_reference as G
from tests import ms_euclidean_cases as EC
from tests import ms_euclidean_reference as R
from tests.golden.cases import KAPPA
from tests.ms_stage_calls import EUCLIDEAN, assign_raw, both_sampling_kernels, components_raw, hill_climb_raw, select_raw, to_dev
from unseenobjectclustering_amd.utils import mean_shift as MS

pytestmark = pytest.mark.gpu
assert KAPPA == EC.KAPPA


# ---- 2. hill climbing against float64 ---------------------------------------------------------------------------------
def climb_rows(what, got, fields, seeds, iters, check=None):
    """Per checked field: (name, kernel deviation from float64, the three yardsticks (direct, tiles, ulp), the tolerance)."""
    rows = []
    for b in (range(len(fields)) if check is None else check):
        ref, devs = EC.climb_yardstick(fields[b], seeds[b], KAPPA, iters)
        err = float(np.abs(got[b].astype(np.float64) - ref).max())
        rows.append((what if len(fields) == 1 else "%s field %d" % (what, b), err, devs, EC.climb_tolerance(devs)))
    return rows


def ratio(err, devs):
    """The kernel's deviation in units of the farthest yardstick (0 / 0, one pixel: both exact, = 0)."""
    return err / max(devs) if err > 0 else 0.0


def run_climb(device, what, fields, seeds, iters, check=None):
    got = hill_climb_raw(to_dev(np.stack(fields), device), to_dev(np.stack(seeds), device), iters, metric=EUCLIDEAN).cpu().numpy()
    assert np.isfinite(got).all()
    return climb_rows(what, got, fields, seeds, iters, check)


def tile_case(device, m, iters):
    X = EC.hc_field(1961)
    return run_climb(device, "n 1961 m %d iters %d" % (m, iters), [X], [EC.hc_seeds(X, m)[0]], iters)


def edge_case(device, n, m):
    fields = [EC.hc_field(n, seed=1 + k) for k in range(3 if n == 4097 else 1)]
    return run_climb(device, "n %d m %d" % (n, m), fields, [EC.hc_seeds(X, m, k)[0] for k, X in enumerate(fields)], 10)


def strided_case(device):
    """Every field against its own float64 run, under the batch's yardstick (ms_euclidean_cases.strided_yardstick)."""
    batch, n, m = EC.HC_STRIDED
    fields, seeds = zip(*(EC.strided_field(b) for b in range(batch)))
    got = hill_climb_raw(to_dev(np.stack(fields), device), to_dev(np.stack(seeds), device), 10, metric=EUCLIDEAN).cpu().numpy()
    assert np.isfinite(got).all()
    devs = EC.strided_yardstick()
    return [("batch %d n %d field %d" % (batch, n, b), float(np.abs(got[b] - R.hill_climb(fields[b], seeds[b], KAPPA, 10)).max()),
             devs, EC.climb_tolerance(devs)) for b in range(batch)]


def affine_case(device):
    batch, n, m, check = EC.HC_AFFINE
    fields = [EC.hc_affine_field(b) for b in range(batch)]
    return run_climb(device, "batch %d n %d" % (batch, n), fields, [EC.hc_affine_seeds(b) for b in range(batch)], 10, check)


def wide_case(device, n, m, X=None):
    X = EC.hc_field(n, seed=7, channels=128) if X is None else X
    Xd = MS.to_planes(to_dev(X, device)[None])
    _, idx, Z, _ = MS.cluster_batch(Xd, [EC.WIDE_FIRST], KAPPA, m, 10, EC.WIDE_EPS, return_parts=True, metric="euclidean")
    torch.cuda.synchronize(device)
    idx = idx[0].cpu().numpy()
    assert idx[0] == EC.WIDE_FIRST and idx.min() >= 0 and idx.max() < n
    got = Z[0].permute(1, 0, 2).reshape(m, 128).cpu().numpy()
    return climb_rows("128-d n %d m %d" % (n, m), [got], [X], [X[idx]], 10)


def scaled_case(device, m):
    X, Z0 = EC.hc_scaled_case(m)
    return run_climb(device, "scaled rows m %d" % m, [X], [Z0], 10)


def clamp_case(device):
    X, Z0 = EC.hc_clamp_case()
    return run_climb(device, "clamp n %d m %d" % EC.HC_CLAMP[:2], [X], [Z0], 10) + run_climb(device, "clamp, one iteration", [X], [Z0], 1)


def climb_cases():
    """Every climb case: name -> function(device) -> rows.  scripts/ms_euclidean_error.py prints them all."""
    out = {}
    for iters in EC.HC_TILE_ITERS:
        for m in EC.HC_TILE_M:
            out["tile m%d iters%d" % (m, iters)] = lambda device, m=m, iters=iters: tile_case(device, m, iters)
    for m in EC.HC_EDGE_M:
        for n in EC.HC_EDGE_N + [4097]:
            out["edge n%d m%d" % (n, m)] = lambda device, n=n, m=m: edge_case(device, n, m)
    out["strided"] = strided_case
    out["affine"] = affine_case
    for n, m in EC.HC_WIDE:
        out["wide n%d m%d" % (n, m)] = lambda device, n=n, m=m: wide_case(device, n, m)
    for m in EC.HC_SCALED_M:
        out["scaled m%d" % m] = lambda device, m=m: scaled_case(device, m)
    out["wide scaled"] = lambda device: wide_case(device, *EC.HC_WIDE_SCALED, X=EC.hc_wide_scaled_field())
    out["clamp"] = clamp_case
    return out


def assert_rows(rows):
    for name, err, devs, tol in rows:
        print("%-32s kernel %.3e  direct %.3e  tiles %.3e  ulp %.3e  ratio %.2f  (K = %g)" % ((name, err) + devs + (ratio(err, devs), EC.K_CLIMB)))
    for name, err, devs, tol in rows:
        assert err <= tol, "%s: %.3e from float64, allowed %.3e = %g x max(direct %.3e, tiles %.3e, ulp %.3e)" % ((name, err, tol, EC.K_CLIMB) + devs)


def tile_id(m):
    return "m%d-ST%d-%s" % (m, EC.instantiation(m)[0], "QUAD" if EC.instantiation(m)[1] else "full")


@pytest.mark.parametrize("iters", EC.HC_TILE_ITERS)
@pytest.mark.parametrize("m", EC.HC_TILE_M, ids=tile_id)
def test_climb_every_seed_tile_count(device, m, iters):
    """hc_iter_flat_kernel<ST, QUAD, EUC> for ST = 1..8, QUAD where the last seed tile holds 1..4 seeds (m = 16k + 2), not QUAD at
    16k + 9, and the full-tile boundaries 16k: n = 37 x 53, one and ten iterations."""
    assert_rows(tile_case(device, m, iters))


@pytest.mark.parametrize("m", EC.HC_EDGE_M, ids=tile_id)
@pytest.mark.parametrize("n", EC.HC_EDGE_N + [4097])
def test_climb_pixel_count_edges(device, n, m):
    """One partial tile (every row beyond n must weigh exactly 0 in numerator AND denominator), waves without a tile, the step
    from one virtual block to two at 1024 | 1025; n = 4097 as three fields."""
    assert_rows(edge_case(device, n, m))


def test_climb_more_items_than_blocks(device):
    """300 fields of 144 pixels: the strided item walk; every field against its own float64 run, the tolerance from the
    batch's yardstick (the largest deviations over every 13th field)."""
    rows = strided_case(device)
    assert len(rows) == EC.HC_STRIDED[0]
    assert_rows(rows)


def test_climb_two_virtual_blocks_per_field(device):
    """256 fields of 2048 pixels (two virtual blocks each: the weight sums of both halves meet in hc_finalize_kernel):
    neighbours point opposite ways, so a seed fragment, a norm or a pixel tile of the wrong field is an O(1) error."""
    rows = affine_case(device)
    assert len(rows) == 5
    assert_rows(rows)


@pytest.mark.parametrize("n,m", EC.HC_WIDE)
def test_climb_128d(device, n, m):
    """hc_iter_kernel<ST, 2, EUC> (two planes) through the whole call: the returned Z against the float64 climb from the
    returned indices."""
    assert_rows(wide_case(device, n, m))


@pytest.mark.parametrize("m", EC.HC_SCALED_M, ids=tile_id)
def test_climb_rows_of_different_norms(device, m):
    """Every row of X scaled by 1, 1/2, 3/4 or 5/4, Z0 rows of all four scales: ||x||^2 ranges over 0.25 .. 1.56 pixel to pixel
    and ||z||^2 seed to seed, so a norm from the wrong slot, row, tile or QUAD lane moves a weight by a factor e^(20 x 0.3)."""
    assert_rows(scaled_case(device, m))


def test_climb_128d_rows_of_different_norms(device):
    """The 128-d field with rows of four norms: each plane holds its own part of every norm, and a padding row of the last
    pixel tile that kept a weight would weigh e^-5 against a seed at 1/2 (against unit seeds e^-20: the unit 128-d cases
    cannot see it)."""
    assert_rows(wide_case(device, *EC.HC_WIDE_SCALED, X=EC.hc_wide_scaled_field()))


def test_climb_clamp_active(device):
    """Two seeds whose weight sums are below 1 (8e-13: the antipode of the field's mean; 0.7: half a field row): the update
    divides by 1, the first lands on the origin, the second on 0.7 x a mean of rows.  After one and after ten iterations."""
    rows = clamp_case(device)
    assert len(rows) == 2
    assert_rows(rows)


@pytest.mark.parametrize("n", EC.HC_OVERREAD_N)
def test_climb_reads_no_row_beyond_n(device, n):
    """The field inside a larger buffer whose rows from n on are seed 0 itself, which a kernel that read them would weigh 1
    each, in numerator and denominator (and the opposite of the field's dominant direction): bit for bit the result of the
    tight buffer."""
    m = 100
    X = EC.hc_field(n, seed=7)
    Z0 = to_dev(EC.hc_seeds(X, m)[0][None], device)
    tight = hill_climb_raw(to_dev(X[None], device), Z0, 10, metric=EUCLIDEAN)
    mean = X.astype(np.float64).sum(axis=0)
    for fill in (EC.hc_seeds(X, m)[0][0], -(mean / np.linalg.norm(mean))):
        buf = np.empty((1, n + 2048, 64), np.float32)
        buf[0, :n] = X
        buf[0, n:] = fill.astype(np.float32)
        got = hill_climb_raw(to_dev(buf, device), Z0, 10, n=n, metric=EUCLIDEAN)
        assert torch.equal(got, tight)
    assert torch.isfinite(tight).all() and not torch.equal(tight, Z0)


# ---- 3a. farthest-point sampling, exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.fps_cases()))
def test_sampling_exact_ties(device, name):
    """Exact ties between pixels of one 16-lane row group, of two waves, of two blocks of either kernel, of two slots of one
    lane: the lower index.  fps_persistent_kernel (norm expansion, xx[] per slot) and fps_step_kernel (direct differences)
    give the same indices and the same seed rows, bit for bit."""
    c = EC.fps_cases()[name]
    want, _ = R.select_seeds(c["X"], c["m"], c["first"])

    def check(kernel):
        idx, seeds = select_raw(device, c["X"][None], c["m"], [c["first"]], metric=EUCLIDEAN)
        assert np.array_equal(idx[0], want), kernel
        assert np.array_equal(seeds[0], R.seed_rows(c["X"], want)), kernel
    both_sampling_kernels(check)


@pytest.mark.parametrize("name", list(EC.fps_continuation_cases()))
def test_sampling_continuation_exact(device, name):
    c = EC.fps_continuation_cases()[name]
    want, _ = R.select_seeds(c["X"], c["m"], None, c["init"], c["num_init"])

    def check(kernel):
        idx, seeds = select_raw(device, c["X"][None], c["m"], None, c["init"][None], c["num_init"], metric=EUCLIDEAN)
        assert np.array_equal(idx[0], want), kernel
        assert np.array_equal(seeds[0], R.seed_rows(c["X"], want, c["init"])), kernel
    both_sampling_kernels(check)


def test_sampling_batch_exact(device):
    c = EC.fps_batch_case()
    want = [R.select_seeds(c["X"][b], c["m"], c["first"][b])[0] for b in range(3)]

    def check(kernel):
        idx, seeds = select_raw(device, c["X"], c["m"], c["first"], metric=EUCLIDEAN)
        for b in range(3):
            assert np.array_equal(idx[b], want[b]), (kernel, b)
            assert np.array_equal(seeds[b], R.seed_rows(c["X"][b], want[b])), (kernel, b)
    both_sampling_kernels(check)


# ---- 3b. seed components, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [EC.EPS_EXACT, EC.EPS_BETWEEN])
@pytest.mark.parametrize("name", list(EC.cc_cases()))
def test_components_exact(device, name, eps):
    """Pairs exactly at eps = 1/2 are members (sqrtf(d^2) <= eps), between seeds of equal and of different norms; the mode of
    the labels present, ties to the smallest; members are overwritten."""
    Z, _ = EC.cc_cases()[name]
    want = R.seed_components(Z, eps)
    got, nu = components_raw(device, Z[None], eps, metric=EUCLIDEAN)
    assert np.array_equal(got[0], want) and nu[0] == len(np.unique(want))


@pytest.mark.parametrize("m", [m for m in EC.CC_M if m > 5])
def test_components_batch_exact(device, m):
    Zb = np.stack([EC.cc_chain(m, "low", "tied"), EC.cc_chain_scaled(m, "high", "majority"), EC.cc_chain_scaled(m, "high", "tied")])
    got, nu = components_raw(device, Zb, EC.EPS_EXACT, metric=EUCLIDEAN)
    for b in range(3):
        want = R.seed_components(Zb[b], EC.EPS_EXACT)
        assert np.array_equal(got[b], want) and nu[b] == len(np.unique(want)), b


# ---- 3c. assignment and the swap, exact ------------------------------------------------------------------------------------
def check_assignment(device, X, Z, sl, nu):
    """Batched inputs through uoc_ms_assign_ex: closest and labels exact against the reference."""
    (la, ca), _ = assign_raw(device, X, Z, sl, nu, metric=EUCLIDEAN)
    for b in range(X.shape[0]):
        labels, closest, _ = R.assign_exact(X[b], Z[b], sl[b], nu[b])
        assert np.array_equal(ca[b], closest), "closest, field %d" % b
        assert np.array_equal(la[b], labels), "labels, field %d" % b
    return la, ca


@pytest.mark.parametrize("scale", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("n", EC.ASSIGN_N)
@pytest.mark.parametrize("m", EC.ASSIGN_M)
def test_assignment_exact_ties(device, m, n, scale):
    """A pixel equidistant from two seeds of one 16-seed tile, of two tiles on one lane, of two tiles and lanes, in every pixel
    slot of a lane: the lower seed.  Scaled: the two seeds have different norms (p(k +- 1) and 0.75 p(k), both 1/4 from p(k)), so
    zzs[] of the wrong seed breaks the tie.  Three fields: the pixels rotated, the seed labels shifted."""
    Z = EC.assign_seeds(m, scale)
    sl, nu = EC.assign_labels(m)
    X = EC.assign_pixels(n)
    Xb = np.stack([np.roll(X, b, axis=0) for b in range(3)])
    slb = np.stack([(sl + b) % nu for b in range(3)]).astype(np.int32)
    check_assignment(device, Xb, np.stack([Z] * 3), slb, [nu] * 3)


@pytest.mark.parametrize("m", EC.PAD_M)
def test_assignment_padding_rows_never_win(device, m):
    """Every real seed is farther from every pixel than ||x||, the distance of a zero padding row of the last seed tile, which,
    unmasked, would win.  The pixels have four different norms."""
    X, Z = EC.padding_case(m)
    sl = (np.arange(m) % 3).astype(np.int32)
    la, ca = check_assignment(device, X[None], Z[None], sl[None], [len(np.unique(sl))])
    assert ca.min() >= 0 and ca.max() < m


@pytest.mark.parametrize("name", list(EC.swap_cases()))
def test_swap_exact(device, name):
    """The largest cluster becomes 0: equal counts (the first wins), a largest label that is not 0, labels with a gap."""
    X, Z, sl, nu = EC.swap_cases()[name]
    check_assignment(device, X[None], Z[None], sl[None], [nu])


# ---- 3d. the whole call on exact inputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,wide,batch", EC.WHOLE)
def test_whole_call_exact(device, n, m, wide, batch):
    """No iteration: the seeds stay rows of the field, so sampling, components (eps = 1/2, exactly a distance), assignment and
    swap are all exact.  Rows of four norms; 128-d: each plane holds a different part of every norm."""
    fields = [EC.whole_field(n, k, wide) for k in range(batch)]
    firsts = [(37 * k + 11) % n for k in range(batch)]
    Xd = to_dev(np.stack(fields), device)
    labels, idx, Z, sl = MS.cluster_batch(MS.to_planes(Xd) if wide else Xd, firsts, KAPPA, m, 0, EC.WHOLE_EPS, return_parts=True,
                                          metric="euclidean")
    torch.cuda.synchronize(device)
    for k in range(batch):
        wl, wi, _, ws = R.cluster_exact(fields[k], m, EC.WHOLE_EPS, firsts[k])
        assert np.array_equal(idx[k].cpu().numpy(), wi), "indices, field %d" % k
        rows = fields[k][wi]
        assert np.array_equal(Z[k].cpu().numpy(), G.planes(rows) if wide else rows), "Z, field %d" % k
        assert np.array_equal(sl[k].cpu().numpy(), ws), "seed labels, field %d" % k
        assert np.array_equal(labels[k].cpu().numpy(), wl), "labels, field %d" % k


# ---- 3e. the pixel no seed wins ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.NOSEED_N)
def test_pixel_no_seed_wins(device, n):
    """A NaN row (one in a full pixel tile, one in the partial tile) has no nearest seed: label 0, counted under label 0 (label 0
    is the largest only WITH the two rows: counted elsewhere or not at all, the swap would exchange 0 and 1 on every pixel).
    closest is seed 0, numpy's and torch's argmin of a row of NaN (max(NaN, 0) = 0 is the kernel's route to it), or INT_MAX, the
    cosine kernels' 'none'; every other pixel as the float64 restatement has it.  (uoc_ms_assign_ex takes 64-d fields only and
    uoc_ms_confidence is cosine only, so there is no 128-d form of this case.)"""
    X, Z, sl, nu = EC.noseed_case(n)
    bad = list(EC.noseed_rows(n))
    fin = np.setdiff1d(np.arange(n), bad)
    (la, ca), _ = assign_raw(device, X[None], Z[None], sl[None], [nu], metric=EUCLIDEAN)
    labels, closest, _ = R.assign_exact(X, Z, sl, nu)
    print("closest of the NaN rows:", ca[0][bad])
    assert (la[0][bad] == 0).all() and np.isin(ca[0][bad], (0, 2147483647)).all()
    assert np.array_equal(ca[0][fin], closest[fin]) and np.array_equal(la[0], labels)
    assert np.array_equal(la[0][fin], sl[closest[fin]])             # no swap
