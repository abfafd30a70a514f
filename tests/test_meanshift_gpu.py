"""GPU parity of the HIP mean-shift path (through the C ABI) against
  (a) golden vectors captured from the reference, and
  (b) the CPU oracle on the same seeded inputs,
plus size-independent properties at the full 480x640 size.

Bars: integer outputs (seed indices, seed labels, label maps) bit-exact — label maps up to
label permutation as north_star states; converged seeds within 1e-4 (fp32).
"""
import os

import numpy as np
import pytest
import torch

from oracle import mean_shift_oracle as O
from tests.golden.cases import MEANSHIFT_CASES, KAPPA, EPSILON, SEED_CONTINUATION_CASES, continuation_inputs
from unseenobjectclustering_amd import synth
from unseenobjectclustering_amd.utils import mean_shift as MS

pytestmark = pytest.mark.gpu
Z_TOL = 1e-4


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "meanshift.npz"))


def _field(c, device):
    X, lab = synth.embedding_field(c["seed"], c["H"], c["W"], 64, c["num_objects"], c["noise"])
    return torch.from_numpy(X).to(device), X, lab


@pytest.mark.parametrize("name", list(MEANSHIFT_CASES))
def test_cluster_matches_reference_golden(golden, device, name):
    c = MEANSHIFT_CASES[name]
    Xd, X, _ = _field(c, device)
    first = int(golden[name + "/indices"][0])
    labels, idx, Z, sl = MS.cluster_batch(Xd[None], [first], KAPPA, c["m"], c["iters"], EPSILON, return_parts=True)
    torch.cuda.synchronize()
    assert np.array_equal(idx[0].cpu().numpy(), golden[name + "/indices"]), "farthest-point indices differ"
    assert np.abs(Z[0].cpu().numpy() - golden[name + "/Z"]).max() < Z_TOL
    assert np.array_equal(sl[0].cpu().numpy(), golden[name + "/seed_labels"])
    got = labels[0].cpu().numpy()
    assert O.labels_equal_up_to_permutation(got, golden[name + "/labels"])
    assert np.array_equal(got.astype(np.uint8), golden[name + "/labels"])  # ids too: CC order + swap are deterministic


@pytest.mark.parametrize("name", ["tiny_60x80", "ragged_37x53", "crop_224_a"])
def test_stagewise_vs_oracle(golden, device, name):
    """Each C-ABI stage on its own, fed the oracle's inputs for that stage."""
    c = MEANSHIFT_CASES[name]
    Xd, X, _ = _field(c, device)
    Xt = torch.from_numpy(X)
    first = int(golden[name + "/indices"][0])
    seeds_o, idx_o = O.select_seeds(Xt, c["m"], first)
    np.random.seed(0)
    state = np.random.get_state()
    # select_smart_seeds draws its own first index: emulate by seeding so that randint gives `first`
    import unittest.mock as mock
    with mock.patch("numpy.random.randint", return_value=first):
        seeds, idx = MS.select_smart_seeds(Xd, c["m"], return_selected_indices=True)
    assert np.array_equal(idx.numpy(), idx_o.numpy())
    assert torch.equal(seeds.cpu(), seeds_o)
    Z_o = O.hill_climb(Xt, seeds_o, KAPPA, c["iters"])
    Z = MS.seed_hill_climbing_ball(Xd, seeds, KAPPA, c["iters"])
    assert (Z.cpu() - Z_o).abs().max().item() < Z_TOL
    sl_o = O.seed_connected_components(Z_o, EPSILON)
    sl = MS.connected_components(Z_o.to(device), EPSILON)
    assert torch.equal(sl, sl_o)


@pytest.mark.parametrize("name", list(SEED_CONTINUATION_CASES))
def test_seed_continuation_matches_reference_golden(golden_dir, device, name):
    """select_smart_seeds(init_seeds=..., num_init_seeds=k) (mean_shift.py:142-170) through uoc_ms_select_seeds_from:
    indices (-1 for the given rows) and the seed matrix bit-exact against the reference's run; the selection lands in
    the caller's init_seeds tensor; the global RNG is consumed only when k == 0."""
    g = np.load(os.path.join(golden_dir, "seedcont.npz"))
    c = SEED_CONTINUATION_CASES[name]
    X, init = continuation_inputs(c)
    Xd, it = torch.from_numpy(X).to(device), torch.from_numpy(init).to(device)
    if c["init"] == "rows":
        np.random.seed(3)
        plain, pidx = MS.select_smart_seeds(Xd, c["m"], return_selected_indices=True)
        assert np.array_equal(pidx.numpy().astype(np.int32), g[name + "/plain_indices"])
        it[:c["k"]] = plain[:c["k"]]
    np.random.seed(3)
    seeds, idx = MS.select_smart_seeds(Xd, c["m"], return_selected_indices=True, init_seeds=it, num_init_seeds=c["k"])
    assert seeds.data_ptr() == it.data_ptr()
    assert idx.dtype == torch.int64 and np.array_equal(idx.numpy().astype(np.int32), g[name + "/indices"])
    assert np.array_equal(seeds.cpu().numpy(), g[name + "/seeds"])
    assert int(np.random.randint(0, 1 << 30)) == int(g[name + "/next_rng"])
    (only_seeds,) = MS.select_smart_seeds(Xd, c["m"], init_seeds=it.clone(), num_init_seeds=c["m"])   # nothing left to pick
    assert torch.equal(only_seeds, it)


def test_seed_continuation_argument_errors(device):
    Xd = torch.from_numpy(synth.embedding_field(1, 16, 16, 64, 2, 0.05)[0]).to(device)
    good = torch.zeros((10, 64), device=device)
    with pytest.raises(TypeError):
        MS.select_smart_seeds(Xd, 10, init_seeds=good)                              # num_init_seeds missing
    with pytest.raises(ValueError):
        MS.select_smart_seeds(Xd, 10, init_seeds=good[:5], num_init_seeds=2)        # wrong shape
    with pytest.raises(ValueError):
        MS.select_smart_seeds(Xd, 10, init_seeds=good, num_init_seeds=11)
    with pytest.raises(ValueError):
        MS.select_smart_seeds(Xd, 10, init_seeds=good.cpu(), num_init_seeds=2)      # other device


def test_public_api_types_and_rng(device):
    """mean_shift_smart_init keeps the reference's signature, return types and RNG coupling."""
    c = MEANSHIFT_CASES["tiny_60x80"]
    Xd, X, _ = _field(c, device)
    np.random.seed(3)
    labels, idx = MS.mean_shift_smart_init(Xd, kappa=20, num_seeds=100, max_iters=10, metric="cosine")
    assert labels.dtype == torch.int64 and labels.shape == (X.shape[0],)
    assert idx.dtype == torch.int64 and idx.shape == (100,)
    np.random.seed(3)
    assert int(idx[0]) == np.random.randint(0, X.shape[0])
    with pytest.raises(NotImplementedError):
        MS.mean_shift_smart_init(Xd, 20, metric="euclidean")


def test_batched_equals_individual(device):
    """K fields in one launch set == K separate calls (stage-2 batching must not change results)."""
    c = MEANSHIFT_CASES["crop_224_a"]
    fields = []
    for s in (2, 3, 4):
        X, _ = synth.embedding_field(s, 224, 224, 64, 3 + s % 3, 0.05)
        fields.append(torch.from_numpy(X))
    Xb = torch.stack(fields).to(device)
    firsts = [5994, 17, 50000]
    lb, ib = MS.cluster_batch(Xb, firsts, KAPPA, 100, 10, EPSILON)
    for k in range(3):
        l1, i1 = MS.cluster_batch(Xb[k:k + 1], firsts[k:k + 1], KAPPA, 100, 10, EPSILON)
        assert torch.equal(l1[0], lb[k]) and torch.equal(i1[0], ib[k])


@pytest.mark.parametrize("shape", [(224, 224), (480, 640), (37, 53)])
def test_converged_seeds_do_not_depend_on_the_batch(device, shape):
    """The fp32 summation order of a hill-climbing iteration must depend on the field only (virtual blocks,
    csrc/meanshift.hip): the converged seed positions Z of a field are BIT-identical whether it is clustered alone, with
    three other fields or among 29 — for every batch the physical grid differs (blocks per field, virtual blocks per
    block, rounds of CUs).  (Round 2 derived the block count from the batch; the label maps agreed only because no
    pixel of the test fields sat on a near-tie.)"""
    H, W = shape
    X, _ = synth.embedding_field(31, H, W, 64, 6, 0.05)
    x0 = torch.from_numpy(X).to(device)
    first = 4321 % (H * W)
    _, _, z1, s1 = MS.cluster_batch(x0[None], [first], KAPPA, 100, 10, EPSILON, return_parts=True)
    for batch in ((4, 30) if H * W <= 224 * 224 else (2, 4)):
        others = [torch.from_numpy(synth.embedding_field(40 + k, H, W, 64, 3 + k % 4, 0.05)[0]) for k in range(min(batch - 1, 3))]
        fields = [x0] + [others[k % len(others)].to(device) for k in range(batch - 1)]
        pos = batch // 2                                   # the field under test somewhere in the middle
        fields[0], fields[pos] = fields[pos], fields[0]
        firsts = [(first + 17 * k) % (H * W) for k in range(batch)]
        firsts[pos] = first
        _, _, zb, sb = MS.cluster_batch(torch.stack(fields), firsts, KAPPA, 100, 10, EPSILON, return_parts=True)
        assert torch.equal(zb[pos], z1[0]), f"batch {batch}: converged seeds differ from the single-field run"
        assert torch.equal(sb[pos], s1[0])


def _hill_climb_raw(X, Z0, iters=10):
    from unseenobjectclustering_amd import _native
    L = _native.lib()
    batch, n, _ = X.shape
    ws = MS._workspace(X.device, L.uoc_ms_workspace_bytes(batch, n, Z0.shape[1]))
    Z = Z0.clone()
    _native.call("uoc_ms_hill_climb", X.device, X, batch, n, Z, Z0.shape[1], KAPPA, iters, ws, ws.numel())
    torch.cuda.synchronize()
    return Z


@pytest.mark.parametrize("batch,n,m", [(1, 224 * 224, 100), (6, 224 * 224, 100), (7, 224 * 224, 100), (8, 224 * 224, 100),
                                       (11, 224 * 224, 98), (29, 224 * 224, 100), (2, 480 * 640, 100), (3, 37 * 53, 97),
                                       (300, 16 * 9, 100)])
def test_seed_tile_parts_are_bit_identical(device, batch, n, m):
    """The flat item schedule of the hill-climbing kernel (csrc/meanshift.hip, HcPlan) may run left-over virtual blocks as
    2 / 3 / 6 seed-tile parts on otherwise idle CUs.  A part accumulates its seed tiles over the same pixel tiles in
    the same order, so the converged seeds must be BIT-identical for every split, forced (UOC_HC_PARTS, speed-only) or
    chosen by the makespan model (0), whatever the batch (tail only / tail + last round / two passes over the grid)."""
    from unseenobjectclustering_amd import _native
    g = torch.Generator(device="cpu").manual_seed(batch * 1000 + m)
    X = torch.nn.functional.normalize(torch.randn(batch, n, 64, generator=g), dim=-1).to(device)
    Z0 = torch.nn.functional.normalize(torch.randn(batch, m, 64, generator=g), dim=-1).to(device)
    old = os.environ.get("UOC_HC_PARTS")
    try:
        out = {}
        for parts in (1, 0, 2, 3, 6):
            os.environ["UOC_HC_PARTS"] = str(parts)
            _native.lib().uoc_reload_env()
            out[parts] = _hill_climb_raw(X, Z0, iters=3)
        for parts in (0, 2, 3, 6):
            assert torch.equal(out[parts], out[1]), f"{parts} seed-tile parts differ from whole items"
        assert torch.isfinite(out[1]).all() and not torch.equal(out[1], Z0)
    finally:
        os.environ.pop("UOC_HC_PARTS", None)
        if old is not None:
            os.environ["UOC_HC_PARTS"] = old
        _native.lib().uoc_reload_env()


def test_full_size_properties(device):
    """480x640 (BASELINE config 3): determinism, purity against the generating partition,
    label 0 is the largest cluster, seed indices distinct and in range."""
    X, lab = synth.embedding_field(21, 480, 640, 64, 8, 0.05)
    Xd = torch.from_numpy(X).to(device)
    l1, i1 = MS.cluster_batch(Xd[None], [12345], KAPPA, 100, 10, EPSILON)
    l2, i2 = MS.cluster_batch(Xd[None], [12345], KAPPA, 100, 10, EPSILON)
    assert torch.equal(l1, l2) and torch.equal(i1, i2)
    got = l1[0].cpu().numpy()
    idx = i1[0].cpu().numpy()
    assert len(set(idx.tolist())) == 100 and idx.min() >= 0 and idx.max() < X.shape[0]
    assert O.labels_equal_up_to_permutation(got, lab.reshape(-1))
    counts = np.bincount(got)
    assert counts.argmax() == 0


def test_degenerate_inputs(device):
    """All-identical points (every distance ties -> lowest index wins) and n < num_seeds tiles."""
    v = np.zeros((1000, 64), np.float32)
    v[:, 3] = 1.0
    Xd = torch.from_numpy(v).to(device)
    labels, idx = MS.cluster_batch(Xd[None], [7], KAPPA, 100, 10, EPSILON)
    lo, io = O.mean_shift_smart_init(torch.from_numpy(v), KAPPA, 100, 10, first_index=7, epsilon=EPSILON)
    assert np.array_equal(idx[0].cpu().numpy(), io.numpy())
    assert np.array_equal(labels[0].cpu().numpy(), lo.numpy())


@pytest.mark.parametrize("shape,batch", [((480, 640), 1), ((224, 224), 7), ((224, 224), 12), ((37, 53), 3)])
def test_persistent_and_streaming_seed_selection_agree(device, shape, batch):
    """The on-chip persistent farthest-point kernel and the one-launch-per-step kernel must pick the
    same 100 indices (batch 12 x 224^2 does not fit on chip and exercises the automatic fallback)."""
    from unseenobjectclustering_amd import _native
    L = _native.lib()
    H, W = shape
    fields = [torch.from_numpy(synth.embedding_field(60 + k, H, W, 64, 3 + k % 4, 0.05)[0]) for k in range(batch)]
    Xb = torch.stack(fields).to(device)
    firsts = [(977 * k + 13) % (H * W) for k in range(batch)]
    try:
        L.uoc_ms_set_persistent_fps(1)
        l1, i1 = MS.cluster_batch(Xb, firsts, KAPPA, 100, 10, EPSILON)
        L.uoc_ms_set_persistent_fps(0)
        l0, i0 = MS.cluster_batch(Xb, firsts, KAPPA, 100, 10, EPSILON)
    finally:
        L.uoc_ms_set_persistent_fps(1)
    assert torch.equal(i1, i0) and torch.equal(l1, l0)


@pytest.mark.parametrize("n,m", [(50, 100), (1, 100), (200, 1), (130, 128), (4097, 17), (300, 34), (515, 51), (77, 68)])
def test_ragged_and_tiny_inputs_vs_oracle(device, n, m):
    """Fewer points than seeds (duplicate seeds, every distance ties), a single point, a single seed,
    the maximum seed count, sizes that are not multiples of any tile, and seed counts whose last tile holds 1 - 4 seeds
    (17, 34, 51, 68: that tile runs on the 4x4x1 matrix instruction, csrc/meanshift.hip QUAD)."""
    rng = np.random.default_rng(n * 1000 + m)
    c = rng.standard_normal((3, 64)).astype(np.float32)
    x = c[rng.integers(0, 3, n)] + 0.05 * rng.standard_normal((n, 64)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    first = int(rng.integers(0, n))
    lo, io, parts = O.mean_shift_smart_init(torch.from_numpy(x), KAPPA, m, 10, first_index=first, epsilon=EPSILON,
                                            return_parts=True)
    labels, idx, Z, sl = MS.cluster_batch(torch.from_numpy(x).to(device)[None], [first], KAPPA, m, 10, EPSILON,
                                          return_parts=True)
    got_idx = idx[0].cpu().numpy()
    if n < m:
        # Once every point is a seed, all running minima are rounding noise around 0 (|x.x - 1| ~ 1e-7) and
        # the reference's later picks depend on MKL's summation order: only the first n picks are defined.
        assert np.array_equal(got_idx[:n], io.numpy()[:n])
        assert got_idx.min() >= 0 and got_idx.max() < n
        assert O.labels_equal_up_to_permutation(labels[0].cpu().numpy(), lo.numpy())
        return
    assert np.array_equal(got_idx, io.numpy())
    assert np.abs(Z[0].cpu().numpy() - parts["Z"].numpy()).max() < Z_TOL
    assert np.array_equal(sl[0].cpu().numpy(), parts["seed_labels"].numpy())
    assert np.array_equal(labels[0].cpu().numpy(), lo.numpy())


def test_argument_errors_are_reported(device):
    from unseenobjectclustering_amd import _native
    X = torch.nn.functional.normalize(torch.randn(1, 256, 64, device=device), dim=2)
    with pytest.raises(_native.NativeError):
        MS.cluster_batch(X, [0], KAPPA, 129, 10, EPSILON)            # num_seeds > UOC_MAX_SEEDS
    with pytest.raises(NotImplementedError):
        MS.cluster_batch(torch.zeros(1, 256, 32, device=device), [0])   # d != 64
