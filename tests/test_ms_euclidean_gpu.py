"""GPU parity of the euclidean-metric mean shift (metric='euclidean', the reference's code default) against the reference's
goldens (tests/golden/meanshift_euclidean.npz) and its float64 restatement (tests/ms_euclidean_reference.py), plus the
properties the cosine path keeps: batch independence, bit-identical reruns, 128-d fields, degenerate inputs, the
two-stage frame, and a cosine path that is unchanged.

Bars: seed indices exact up to the first pick whose top-two gap in the restatement is below GAP_TOL (fp32 near-tie);
converged seeds within Z_TOL; seed labels exact (the goldens' pairwise seed distances are checked to be CC_TOL away from
epsilon); pixel labels equal up to permutation except pixels whose two nearest seeds are within ASSIGN_TOL."""
import os

import numpy as np
import pytest
import torch

from tests import ms_euclidean_reference as R
from tests.golden.cases import MEANSHIFT_CASES, WIDE_MEANSHIFT_CASES, KAPPA, EPSILON
from unseenobjectclustering_amd import _native, networks, synth
from unseenobjectclustering_amd.fcn import graph_replay as GR, test_dataset as TD
from unseenobjectclustering_amd.fcn.config import cfg
from unseenobjectclustering_amd.utils import mean_shift as MS

pytestmark = pytest.mark.gpu
CASES = {**MEANSHIFT_CASES, **WIDE_MEANSHIFT_CASES}
GAP_TOL = 1e-5
Z_TOL = 1e-4
CC_TOL = 1e-4
ASSIGN_TOL = 1e-4


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "meanshift_euclidean.npz"))


GOLDEN_NAMES = ["tiny_60x80", "ragged_37x53", "fewseeds_m20", "oneiter", "wide_60x80"]


def _field(name):
    c = CASES[name]
    d = 128 if name.startswith("wide") else 64
    X, _ = synth.embedding_field(c["seed"], c["H"], c["W"], d, c["num_objects"], c["noise"])
    return X, c


def _kernel_layout(X, device):
    """[n, d] numpy -> the [1, n, 64] or [1, 2, n, 64] device layout of cluster_batch."""
    Xd = torch.from_numpy(X).to(device)[None]
    return MS.to_planes(Xd) if X.shape[1] == 128 else Xd


def _rows(Z):
    """[1, m, 64] or [1, 2, m, 64] seeds -> [m, d] numpy."""
    Z = Z[0]
    if Z.dim() == 3:
        Z = Z.permute(1, 0, 2).reshape(Z.shape[1], -1)
    return Z.cpu().numpy()


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_cluster_matches_reference_golden(golden, device, name):
    X, c = _field(name)
    g_idx, g_Z, g_sl, g_lab = (golden[name + k] for k in ("/indices", "/Z", "/seed_labels", "/labels"))
    labels, idx, Z, sl = MS.cluster_batch(_kernel_layout(X, device), [int(g_idx[0])], KAPPA, c["m"], c["iters"], EPSILON,
                                          return_parts=True, metric="euclidean")
    idx = idx[0].cpu().numpy()
    _, gaps = R.select_seeds(X, c["m"], int(g_idx[0]))
    tie = np.flatnonzero(gaps < GAP_TOL)
    k = int(tie[0]) if tie.size else c["m"]
    assert np.array_equal(idx[:k], g_idx[:k]), "farthest-point indices differ before any near-tie"
    if np.array_equal(idx, g_idx):
        ref_Z, ref_sl = g_Z, g_sl                  # the reference's own converged seeds and labels
    else:                                          # a near-tied pick went the other way: the restatement from these seeds
        ref_Z = R.hill_climb(X, X[idx], KAPPA, c["iters"])
        ref_sl = R.seed_components(ref_Z, EPSILON)
    Zg = _rows(Z).astype(np.float64)
    assert np.abs(Zg - ref_Z).max() < Z_TOL
    sl = sl[0].cpu().numpy()
    if R.cc_margin(Zg, EPSILON) > 1e-6:            # the component kernel on its own seeds
        assert np.array_equal(sl, R.seed_components(Zg, EPSILON))
    if R.cc_margin(ref_Z, EPSILON) > CC_TOL:
        assert np.array_equal(sl, ref_sl)
        want, gap = R.assign(X, ref_Z, ref_sl)
        if ref_Z is g_Z:
            assert R.labels_equal_up_to_permutation(want, g_lab)
        clear = gap > ASSIGN_TOL
        assert clear.mean() > 0.95
        got = labels[0].cpu().numpy()
        assert R.labels_equal_up_to_permutation(got[clear], want[clear])


@pytest.fixture
def euclidean_cfg():
    """The program's opt-in to the euclidean metric (fcn/config.py), undone afterwards."""
    saved = cfg.TRAIN.EMBEDDING_METRIC
    cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
    yield
    cfg.TRAIN.EMBEDDING_METRIC = saved


def test_reference_surface_stage_by_stage(golden, device, euclidean_cfg):
    name = "tiny_60x80"
    X, c = _field(name)
    Xd = torch.from_numpy(X).to(device)
    first = int(golden[name + "/indices"][0])
    np.random.seed(0)
    draw = np.random.randint(0, X.shape[0])
    np.random.seed(0)
    seeds, idx = MS.select_smart_seeds(Xd, c["m"], return_selected_indices=True, metric="euclidean")
    assert int(idx[0]) == draw and idx.dtype == torch.int64
    want, _ = R.select_seeds(X, c["m"], draw)
    assert np.array_equal(idx.numpy(), want)
    assert torch.equal(seeds, Xd[idx.to(device)])
    # hill climbing from the golden seeds, components of the golden converged seeds
    Z0 = Xd[torch.from_numpy(golden[name + "/indices"]).long().to(device)]
    Z = MS.seed_hill_climbing_ball(Xd, Z0, KAPPA, max_iters=c["iters"], metric="euclidean")
    assert np.abs(Z.cpu().numpy() - golden[name + "/Z"]).max() < Z_TOL
    assert np.abs(Z.cpu().numpy() - R.hill_climb(X, X[golden[name + "/indices"]], KAPPA, c["iters"])).max() < Z_TOL
    sl = MS.connected_components(torch.from_numpy(golden[name + "/Z"]).to(device), EPSILON, metric="euclidean")
    assert sl.dtype == torch.int64 and np.array_equal(sl.numpy(), golden[name + "/seed_labels"])
    np.random.seed(5)
    labels, idx2 = MS.mean_shift_smart_init(Xd, KAPPA, num_seeds=c["m"], max_iters=c["iters"], metric="euclidean")
    np.random.seed(5)
    assert int(idx2[0]) == np.random.randint(0, X.shape[0])
    assert labels.dtype == torch.int64 and labels.shape == (X.shape[0],) and int(labels.min()) == 0
    sl2, Z2 = MS.mean_shift_with_seeds(Xd, Z0, KAPPA, max_iters=c["iters"], metric="euclidean")
    assert torch.equal(Z2, Z) and torch.equal(sl2, MS.connected_components(Z, EPSILON, metric="euclidean"))


def test_public_api_types_and_rng_with_the_opt_in(device, euclidean_cfg):
    """mean_shift_smart_init with metric='euclidean' keeps the reference's signature, return types and RNG coupling."""
    X, c = _field("tiny_60x80")
    Xd = torch.from_numpy(X).to(device)
    np.random.seed(3)
    labels, idx = MS.mean_shift_smart_init(Xd, kappa=20, num_seeds=100, max_iters=10, metric="euclidean")
    assert labels.dtype == torch.int64 and labels.shape == (X.shape[0],)
    assert idx.dtype == torch.int64 and idx.shape == (100,)
    np.random.seed(3)
    assert int(idx[0]) == np.random.randint(0, X.shape[0])
    with pytest.raises(NotImplementedError):
        MS.mean_shift_smart_init(Xd, 20, metric="manhattan")
    cfg.TRAIN.EMBEDDING_METRIC = "cosine"
    with pytest.raises(NotImplementedError):          # without the opt-in: refused
        MS.mean_shift_smart_init(Xd, 20, metric="euclidean")


def _crop_fields(B, H, W, d=64, seed0=40):
    return np.stack([synth.embedding_field(seed0 + i, H, W, d, 3 + i % 4, 0.05)[0] for i in range(B)])


@pytest.mark.parametrize("d,B,H,W", [(64, 7, 224, 224), (64, 2, 480, 640), (128, 3, 224, 224)])
def test_batched_equals_individual_and_reruns_are_identical(device, d, B, H, W):
    Xs = _crop_fields(B, H, W, d)
    Xd = torch.from_numpy(Xs).to(device)
    if d == 128:
        Xd = MS.to_planes(Xd)
    firsts = [(977 * (i + 1)) % (H * W) for i in range(B)]
    out = MS.cluster_batch(Xd, firsts, KAPPA, 100, 10, EPSILON, return_parts=True, metric="euclidean")
    again = MS.cluster_batch(Xd, firsts, KAPPA, 100, 10, EPSILON, return_parts=True, metric="euclidean")
    for a, b in zip(out, again):
        assert torch.equal(a, b), "two runs differ"
    for i in range(B):
        one = MS.cluster_batch(Xd[i:i + 1].contiguous(), [firsts[i]], KAPPA, 100, 10, EPSILON, return_parts=True,
                               metric="euclidean")
        for a, b in zip(out, one):
            assert torch.equal(a[i:i + 1], b), f"field {i}: batched result differs from the field alone"
    assert torch.isfinite(out[2]).all()
    labels = out[0]
    assert int(labels.min()) >= 0 and int(labels.max()) < 100
    # the euclidean update is not renormalised: converged seeds sit inside the unit sphere
    norms = out[2].pow(2).sum(dim=-1)
    norms = norms.sum(dim=1) if d == 128 else norms
    assert float(norms.max()) < 1.0 + 1e-5


def test_restatement_agrees_on_a_full_size_field(device):
    X = synth.embedding_field(77, 480, 640, 64, 6, 0.05)[0]
    first = 123457
    labels, idx, Z, sl = MS.cluster_batch(torch.from_numpy(X).to(device)[None], [first], KAPPA, 100, 10, EPSILON,
                                          return_parts=True, metric="euclidean")
    want_idx, gaps = R.select_seeds(X, 100, first)
    tie = np.flatnonzero(gaps < GAP_TOL)
    k = int(tie[0]) if tie.size else 100
    assert np.array_equal(idx[0].cpu().numpy()[:k], want_idx[:k])
    if k == 100:
        Zr = R.hill_climb(X, X[want_idx], KAPPA, 10)
        assert np.abs(Z[0].cpu().numpy() - Zr).max() < Z_TOL


def test_degenerate_inputs(device):
    v = np.zeros((64,), np.float32)
    v[3] = 1.0
    same = torch.from_numpy(np.tile(v, (500, 1))).to(device)[None]
    labels, idx, Z, sl = MS.cluster_batch(same, [17], KAPPA, 100, 10, EPSILON, return_parts=True, metric="euclidean")
    assert int(labels.abs().max()) == 0 and torch.isfinite(Z).all()
    assert int(idx[0, 0]) == 17 and int(idx[0, 1]) == 0         # every distance is 0: the first index wins the tie
    assert torch.allclose(Z[0], same[0, :1].expand(100, 64), atol=1e-6)
    few = torch.from_numpy(synth.embedding_field(9, 5, 10, 64, 2, 0.05)[0]).to(device)[None]   # 50 points, 100 seeds
    labels, idx, Z, sl = MS.cluster_batch(few, [3], KAPPA, 100, 10, EPSILON, return_parts=True, metric="euclidean")
    assert torch.isfinite(Z).all() and int(labels.min()) >= 0 and int(labels.max()) < 100
    assert int(idx.min()) >= 0 and int(idx.max()) < 50
    for stage in (few, same[:, :50]):
        a = MS.cluster_batch(stage, [1], KAPPA, 100, 10, EPSILON, metric="euclidean")
        b = MS.cluster_batch(stage, [1], KAPPA, 100, 10, EPSILON, metric="euclidean")
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_cosine_metric_equals_the_unchanged_entry_points(device):
    X = torch.from_numpy(synth.embedding_field(31, 224, 224, 64, 5, 0.05)[0]).to(device)[None]
    B, n = 1, X.shape[1]
    got = MS.cluster_batch(X, [4321], KAPPA, 100, 10, EPSILON, return_parts=True, metric="cosine")
    L = _native.lib()
    first = torch.tensor([4321], dtype=torch.int32, device=device)
    labels = torch.empty((B, n), dtype=torch.int32, device=device)
    indices = torch.empty((B, 100), dtype=torch.int32, device=device)
    Z = torch.empty((B, 100, 64), dtype=torch.float32, device=device)
    sl = torch.empty((B, 100), dtype=torch.int32, device=device)
    ws = torch.empty(L.uoc_ms_workspace_bytes(B, n, 100), dtype=torch.uint8, device=device)
    _native.call("uoc_ms_cluster", device, X, B, n, 100, KAPPA, 10, EPSILON, first, labels, indices, Z, sl, ws, ws.numel())
    for a, b in zip(got, (labels, indices, Z, sl)):
        assert torch.equal(a, b)
    assert cfg.TRAIN.EMBEDDING_METRIC == "cosine"
    dflt = MS.cluster_batch(X, [4321], KAPPA, 100, 10, EPSILON, return_parts=True)      # the configured metric
    for a, b in zip(dflt, (labels, indices, Z, sl)):
        assert torch.equal(a, b)
    euc = MS.cluster_batch(X, [4321], KAPPA, 100, 10, EPSILON, return_parts=True, metric="euclidean")
    assert not torch.equal(euc[2], Z)          # the metric argument reaches the kernels


@pytest.fixture(scope="module")
def nets(device):
    cfg.device = device
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return (networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval())


def test_two_stage_frame_with_the_euclidean_metric(device, nets):
    saved = (cfg.TRAIN.EMBEDDING_METRIC, cfg.TEST.GRAPH_REPLAY)
    frames = []
    for seed, objects in ((20011, 5), (20012, 3)):
        fr = synth.palette_frame(seed, 480, 640, objects)
        frames.append(dict(image_color=torch.from_numpy(fr["image_color"]).to(device),
                           depth=torch.from_numpy(fr["depth"]).to(device)))
    try:
        cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        cfg.TEST.GRAPH_REPLAY = False
        runs = []
        for rep in range(2):
            out = []
            for i, f in enumerate(frames):
                np.random.seed(300 + i)
                lab, ref = TD.test_sample(f, nets[0], nets[1])
                out.append((lab, ref, TD.LAST_FRAME_STATS["rois"]))
            runs.append(out)
        rois = [k for _, _, k in runs[0]]
        assert max(rois) > 0, f"no frame reached stage 2: K = {rois}"
        for (l0, r0, k0), (l1, r1, k1) in zip(*runs):
            assert k0 == k1 and torch.equal(l0, l1)
            assert (r0 is None) == (r1 is None) and (r0 is None or torch.equal(r0, r1))
            assert l0.shape[-2:] == (480, 640) and float(l0.min()) >= 0 and len(torch.unique(l0)) >= 2
            if r0 is not None:
                assert r0.shape[-2:] == (480, 640) and float(r0.min()) >= 0
        # the stage-1 map is not the cosine one: the metric reaches the pipeline
        cfg.TRAIN.EMBEDDING_METRIC = "cosine"
        np.random.seed(300)
        lab_cos, _ = TD.test_sample(frames[0], nets[0], nets[1])
        assert not torch.equal(lab_cos, runs[0][0][0])
        # graph replay honours the metric: capture + replay equal the eager euclidean frames
        cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        cfg.TEST.GRAPH_REPLAY = True
        GR.reset()
        for rnd in range(3):
            for i, f in enumerate(frames):
                np.random.seed(300 + i)
                out, refined = TD._run_frame(f, nets[0], nets[1], TD.DEPTH_FILTER, return_device=True, checked=True)
                assert torch.equal(out.float().cpu().reshape(-1), runs[0][i][0].reshape(-1)), (rnd, i)
    finally:
        cfg.TRAIN.EMBEDDING_METRIC, cfg.TEST.GRAPH_REPLAY = saved
        GR.reset()
