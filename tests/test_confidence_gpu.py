"""Label confidence on the GPU (uoc_ms_confidence, uoc_conf_paste, uoc_conf_objects, confidence.py) against the fp64 numpy
restatement tests/confidence_reference.py.

The margin is held to TOL = 2 (C + 4) 2^-24 (derived in the reference's docstring: 8.1e-6 for 64 channels, 1.57e-5 for
128); labels / second are compared wherever the fp64 decision is further than 2 TOL from flipping; labels and closest are
bit-identical to uoc_ms_assign's; the integer entries are compared exactly."""
import json
import os

import numpy as np
import pytest
import torch

from tests import confidence_reference as R
from tests.golden.cases import EPSILON, GLUE_CASES, KAPPA, MEANSHIFT_CASES, crop_cluster_labels, glue_inputs
from unseenobjectclustering_amd import _native, confidence as CF, io as uio, networks, synth
from unseenobjectclustering_amd import objects as O
from unseenobjectclustering_amd.fcn import test_dataset as TD
from unseenobjectclustering_amd.fcn.config import cfg
from unseenobjectclustering_amd.utils import mean_shift as MS

pytestmark = pytest.mark.gpu
FIELDS = ("labels", "margin", "second", "closest", "rival")


def unit(rng, *shape):
    v = rng.standard_normal(shape)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def seeded_labels(rng, m):
    """Random seed labels over k = min(5, m) ids, every id present, about half the seeds on id 1: the largest cluster is
    then id 1 by a wide margin of pixels, so the swap is exercised and does not hinge on a near-tie pixel."""
    k = min(5, m)
    sl = rng.integers(0, k, size=m)
    if k > 1:
        sl[rng.random(m) < 0.5] = 1
    sl[:k] = np.arange(k)
    return sl.astype(np.int32)


def run(device, X, Z, sl, nu=None):
    """One field (X [n,64] or planes [2,n,64]) through assign_confidence -> numpy outputs."""
    res = CF.assign_confidence(torch.from_numpy(X)[None].to(device), torch.from_numpy(Z)[None].to(device),
                               torch.from_numpy(sl)[None].to(device), None if nu is None else [nu])
    return {k: getattr(res, k)[0].cpu().numpy() for k in FIELDS}


def raw_assign(device, X, Z, sl, nu):
    """uoc_ms_assign on one 64-d field -> (labels, closest) device tensors."""
    L = _native.lib()
    Xd, Zd = torch.from_numpy(X)[None].to(device), torch.from_numpy(Z)[None].to(device)
    sld = torch.from_numpy(sl)[None].to(device)
    nud = torch.tensor([nu], dtype=torch.int32, device=device)
    n, m = X.shape[0], Z.shape[0]
    labels, closest = (torch.empty((1, n), dtype=torch.int32, device=device) for _ in range(2))
    ws = MS._workspace(device, L.uoc_ms_workspace_bytes(1, n, m))
    _native.call("uoc_ms_assign", device, Xd, 1, n, Zd, sld, nud, m, labels, closest, ws, ws.numel())
    return labels[0].cpu().numpy(), closest[0].cpu().numpy()


def check_against_reference(got, X, Z, sl, nu=None, exclude_labels=True):
    """The comparisons every field gets.  Returns (pixels excluded from the labels check, from the second check)."""
    channels = 64 * (1 if X.ndim == 2 else X.shape[0])
    TOL = R.tol(channels)
    want = R.assign(X, Z, sl, nu)
    err = np.abs(got["margin"].astype(np.float64) - want["margin"])
    print("margin error max %.3e (TOL %.3e), smallest fp64 margin %.3e" % (err.max(), TOL, want["margin"].min()))
    assert err.max() <= TOL
    assert (got["margin"] >= 0).all()
    sure = want["margin"] > 2 * TOL
    if not exclude_labels:
        assert sure.all()
    assert np.array_equal(got["labels"][sure], want["labels"][sure])
    sure2 = sure & (want["gap23"] >= 2 * TOL)
    assert np.array_equal(got["second"][sure2], want["second"][sure2])
    # what the outputs say about each other, everywhere: rival -1 <=> second -1 <=> margin 1.0f; the rival's seed label differs
    none = got["rival"] < 0
    assert np.array_equal(none, got["second"] < 0) and (got["margin"][none] == 1.0).all()
    assert np.array_equal(none, want["rival"] < 0)
    sl64 = np.asarray(sl)
    assert (sl64[got["rival"][~none]] != sl64[got["closest"][~none]]).all()
    # ... and the margin is the fp64 distance gap of the very pair of seeds the kernel names
    d = 0.5 * (1.0 - R.flat(X) @ R.flat(Z).T)
    rows = np.arange(d.shape[0])[~none]
    pair = d[rows, got["rival"][~none]] - d[rows, got["closest"][~none]]
    assert np.abs(got["margin"][~none] - pair).max(initial=0.0) <= TOL
    return int((~sure).sum()), int((~sure2).sum())


# ---- 1. engineered: pixels walking from one seed to a seed of the other component --------------------------------------
@pytest.mark.parametrize("variant", ["axes", "rotated"])
def test_engineered_walk_between_two_components(device, variant):
    """n = 257, m = 4, two components; pixel k = normalize((1 - a) z0 + a z2), a = k / 256: the margin falls to ~0 at a = 1/2.
    'axes': the seeds are basis vectors, every dot product is exact and the tie at a = 1/2 is an exact tie that both sides
    resolve to the lowest seed: 129 : 128 pixels, no swap.  'rotated': random unit seeds (inexact products, the tie pixel
    falls either way), seed labels (2, 2, 1, 1) with num_unique = 2: only ids 0 and 1 are counted, so id 1 is the largest
    cluster whatever the tie pixel does and changes places with the (absent) id 0."""
    rng = np.random.default_rng(7)
    if variant == "axes":
        Z = np.eye(64, dtype=np.float32)[[0, 2, 1, 3]]          # z0 = e0, z1 = e2 | z2 = e1, z3 = e3
        sl, nu = np.array([0, 0, 1, 1], np.int32), 2
    else:
        Z = unit(rng, 4, 64)
        sl, nu = np.array([2, 2, 1, 1], np.int32), 2
    a = (np.arange(257) / 256.0)[:, None]
    X = (1 - a) * Z[0].astype(np.float64) + a * Z[2].astype(np.float64)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    got = run(device, X, Z, sl, nu)
    unsure, _ = check_against_reference(got, X, Z, sl, nu)
    assert unsure <= 3                                           # a = 1/2 and at most its two neighbours
    assert got["margin"][128] <= 2 * R.tol(64) and got["margin"][0] > 0.2 and got["margin"][256] > 0.2
    if variant == "axes":
        assert got["margin"][128] == 0.0 and got["closest"][128] == 0 and got["rival"][128] == 2
        assert got["labels"][:129].tolist() == [0] * 129 and got["labels"][129:].tolist() == [1] * 128
        assert got["second"][:129].tolist() == [1] * 129 and got["second"][129:].tolist() == [0] * 128
    else:
        assert set(got["labels"][:120].tolist()) == {2} and set(got["labels"][137:].tolist()) == {0}
        assert set(got["second"][:120].tolist()) == {0} and set(got["second"][137:].tolist()) == {2}


# ---- 2. one component ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 37])
def test_one_component_has_no_rival(device, m):
    rng = np.random.default_rng(m)
    X, Z = unit(rng, 300, 64), unit(rng, m, 64)
    got = run(device, X, Z, np.zeros(m, np.int32))
    assert (got["margin"] == 1.0).all() and (got["second"] == -1).all() and (got["rival"] == -1).all()
    assert (got["labels"] == 0).all()
    if m == 1:
        assert (got["closest"] == 0).all()
    lab_a, clo_a = raw_assign(device, X, Z, np.zeros(m, np.int32), 1)
    assert np.array_equal(got["labels"], lab_a) and np.array_equal(got["closest"], clo_a)


# ---- 3. shapes + 4. bit-identity with uoc_ms_assign -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 1961])
@pytest.mark.parametrize("m", [1, 16, 17, 100, 128])
def test_shapes_against_reference_and_assign(device, n, m):
    """Tile tails in n (16 pixels per MFMA tile, 4 waves per block) and in m (16 seeds per seed tile)."""
    rng = np.random.default_rng(1000 * m + n)
    X, Z, sl = unit(rng, n, 64), unit(rng, m, 64), seeded_labels(rng, m)
    nu = len(np.unique(sl))
    got = run(device, X, Z, sl)
    check_against_reference(got, X, Z, sl, nu)
    lab_a, clo_a = raw_assign(device, X, Z, sl, nu)
    assert np.array_equal(got["labels"], lab_a) and np.array_equal(got["closest"], clo_a)


def test_two_halves(device):
    """128-d fields as two planes, n = 600, m = 20.  uoc_ms_assign has no 128-d form; the clustering's own assignment
    (uoc_ms_cluster_wide) is the bit-identity partner there."""
    rng = np.random.default_rng(128)
    X, Z, sl = unit(rng, 600, 128), unit(rng, 20, 128), seeded_labels(rng, 20)
    Xp = np.ascontiguousarray(X.reshape(600, 2, 64).transpose(1, 0, 2))
    Zp = np.ascontiguousarray(Z.reshape(20, 2, 64).transpose(1, 0, 2))
    got = run(device, Xp, Zp, sl)
    check_against_reference(got, Xp, Zp, sl)
    Xw, _ = synth.embedding_field(21, 30, 40, 128, 4, 0.05)
    Xd = MS.to_planes(torch.from_numpy(Xw)[None].to(device))
    labels, _, Zd, sld = MS.cluster_batch(Xd, [77], KAPPA, 100, 10, EPSILON, return_parts=True, metric="cosine")
    res = CF.assign_confidence(Xd, Zd, sld)
    assert torch.equal(res.labels, labels)
    got = {k: getattr(res, k)[0].cpu().numpy() for k in FIELDS}
    check_against_reference(got, Xd[0].cpu().numpy(), Zd[0].cpu().numpy(), sld[0].cpu().numpy())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "meanshift.npz"))


@pytest.mark.parametrize("name", ["tiny_60x80", "ragged_37x53", "fewseeds_m20"])
def test_golden_fields(golden, device, name):
    """The converged seeds of the clustering itself: labels and closest bit-identical to cluster_batch's and uoc_ms_assign's,
    the margin within TOL of fp64, labels equal with NO exclusion (the smallest fp64 margin of these fields is 0.27), second
    skipping only pixels whose fp64 gap between the second and third component is below 2 TOL: at most 1 % of them."""
    c = MEANSHIFT_CASES[name]
    X, _ = synth.embedding_field(c["seed"], c["H"], c["W"], 64, c["num_objects"], c["noise"])
    Xd = torch.from_numpy(X)[None].to(device)
    first = int(golden[name + "/indices"][0])
    labels_cb, _, Zd, sld = MS.cluster_batch(Xd, [first], KAPPA, c["m"], c["iters"], EPSILON, return_parts=True, metric="cosine")
    lab_c, margin, second, Z2, sl2 = CF.cluster_with_confidence(Xd, [first], KAPPA, c["m"], c["iters"], EPSILON)
    assert torch.equal(lab_c, labels_cb) and torch.equal(Z2, Zd) and torch.equal(sl2, sld)
    res = CF.assign_confidence(Xd, Zd, sld)
    assert torch.equal(res.labels, labels_cb) and torch.equal(res.margin, margin) and torch.equal(res.second, second)
    Z, sl = Zd[0].cpu().numpy(), sld[0].cpu().numpy()
    nu = len(np.unique(sl))
    lab_a, clo_a = raw_assign(device, X, Z, sl, nu)
    got = {k: getattr(res, k)[0].cpu().numpy() for k in FIELDS}
    assert np.array_equal(got["labels"], lab_a) and np.array_equal(got["closest"], clo_a)
    _, skipped = check_against_reference(got, X, Z, sl, nu, exclude_labels=False)
    print("second: skipped %d of %d pixels" % (skipped, X.shape[0]))
    assert skipped <= 0.01 * X.shape[0]


def test_null_optional_outputs(device):
    """second, closest and rival are nullable: with all three NULL (one relabel launch instead of two) labels and margin
    are those of the full call, and each one alone may be left out."""
    rng = np.random.default_rng(77)
    n, m = 1961, 100
    X, Z, sl = unit(rng, n, 64), unit(rng, m, 64), seeded_labels(rng, m)
    full = CF.assign_confidence(torch.from_numpy(X)[None].to(device), torch.from_numpy(Z)[None].to(device),
                                torch.from_numpy(sl)[None].to(device))
    L = _native.lib()
    Xd, Zd, sld = (torch.from_numpy(a)[None].to(device) for a in (X, Z, sl))
    nud = torch.tensor([len(np.unique(sl))], dtype=torch.int32, device=device)
    nws = L.uoc_ms_confidence_workspace_bytes(1, n, m, 1)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    for keep in ((), ("second",), ("closest",), ("rival",)):
        labels = torch.full((1, n), -77, dtype=torch.int32, device=device)
        margin = torch.full((1, n), -77.0, device=device)
        opt = {k: torch.full((1, n), -77, dtype=torch.int32, device=device) if k in keep else None for k in ("second", "closest", "rival")}
        _native.call("uoc_ms_confidence", device, Xd, 1, 1, n, Zd, sld, nud, m, 0, labels, margin, opt["second"], opt["closest"],
                     opt["rival"], ws, nws)
        assert torch.equal(labels, full.labels) and torch.equal(margin, full.margin), keep
        for k in keep:
            assert torch.equal(opt[k], getattr(full, k)), k
    assert int(full.labels.max()) >= 1 and int((full.second >= 0).sum()) == n


def test_segment_confidence_refuses_the_euclidean_opt_in_on_the_device(device, golden_dir):
    """Under the euclidean opt-in test_sample clusters with the euclidean metric; the confidence entries refuse, draw nothing
    from the RNG and leave the plain path alone."""
    cfg.device = device
    sample = _demo_sample(golden_dir)
    net, net_crop = _nets()
    old = cfg.TRAIN.EMBEDDING_METRIC
    try:
        cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        np.random.seed(3)
        before = np.random.get_state()[1].copy()
        with pytest.raises(NotImplementedError, match="cosine"):
            CF.segment_confidence(sample, net, net_crop)
        with pytest.raises(NotImplementedError, match="cosine"):
            O.segment_objects(sample, net, net_crop, confidence=True)
        assert np.array_equal(np.random.get_state()[1], before)
    finally:
        cfg.TRAIN.EMBEDDING_METRIC = old


# ---- 5. batch independence -------------------------------------------------------------------------------------------
def test_batch_of_three_equals_single_calls(device):
    rng = np.random.default_rng(55)
    X, Z = unit(rng, 3, 600, 64), unit(rng, 3, 20, 64)
    sl = np.stack([seeded_labels(rng, 20) for _ in range(3)])
    Xd, Zd, sld = (torch.from_numpy(a).to(device) for a in (X, Z, sl))
    both = CF.assign_confidence(Xd, Zd, sld)
    for b in range(3):
        one = CF.assign_confidence(Xd[b:b + 1], Zd[b:b + 1], sld[b:b + 1])
        for k in FIELDS:
            assert torch.equal(getattr(both, k)[b], getattr(one, k)[0]), (b, k)


# ---- 6. uoc_conf_paste -----------------------------------------------------------------------------------------------
def roi_table(boxes, device):
    t = _native.RoiTable()
    t.K = len(boxes)
    for k, box in enumerate(boxes):
        for i in range(4):
            t.box[k][i] = int(box[i])
        t.label[k] = k + 1
    return torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(device)


def match_with_plan(labels_crop, mask, depth, table, K, S, H, W, device):
    """One uoc_roi_match call that asks for the plan -> (refined [H*W] int32, plan [K + K*128] int32), device tensors."""
    refined = torch.empty((H * W,), dtype=torch.int32, device=device)
    plan = torch.empty((K + K * 128,), dtype=torch.int32, device=device)
    ws, status = TD._ws(device), TD._status_word(device)
    _native.call("uoc_roi_match", device, labels_crop, mask, depth, table, K, S, H, W, refined, None, plan, status, ws, ws.numel())
    assert not TD._take_order_flag(status)
    return refined, plan


@pytest.mark.parametrize("name", ["normal_5", "border_8", "small_ragged"])
def test_paste_follows_the_label_paste(device, name):
    """Pasting values = float(map[k][labels_crop]) into a zero map gives `refined` itself; into a NaN map, NaN exactly where
    refined == 0; and the numpy restatement of the walk agrees."""
    cfg.device = device
    c = GLUE_CASES[name]
    img, lab, depth, gt = glue_inputs(c)
    imgd, depthd = img.to(device), depth.to(device)
    filt = TD.filter_labels_depth(lab, depthd, 0.8)
    _, mask_c, rois, depth_c = TD.crop_rois(imgd, filt.clone(), depthd)
    K, S = int(mask_c.shape[0]), int(mask_c.shape[1])
    H, W = c["H"], c["W"]
    assert K >= 1
    labels_crop = crop_cluster_labels(c, gt, rois.cpu()).to(device).round().to(torch.int32).reshape(K, S * S).contiguous()
    boxes = rois.cpu().numpy().astype(np.int64)
    table = roi_table(boxes, device)
    refined, plan = match_with_plan(labels_crop, mask_c, depth_c, table, K, S, H, W, device)
    idmap = plan[K:].view(K, 128)
    values = torch.gather(idmap, 1, labels_crop.long().clamp(0, 127)).float().contiguous()
    out0 = CF.paste_values(values, labels_crop, table, plan, K, H, W, torch.zeros(H * W, device=device))
    assert torch.equal(out0, refined.float()) and int(refined.max()) >= 1
    outn = CF.paste_values(values, labels_crop, table, plan, K, H, W, torch.full((H * W,), float("nan"), device=device))
    assert torch.equal(torch.isnan(outn), refined == 0)
    assert torch.equal(torch.nan_to_num(outn, nan=0.0), refined.float())
    want = R.paste(values.cpu().numpy(), labels_crop.cpu().numpy(), boxes, plan.cpu().numpy(), K, S, H, W, np.zeros((H, W), np.float32))
    assert np.array_equal(out0.view(H, W).cpu().numpy(), want)


def test_paste_overlapping_rois_later_wins(device):
    """Two overlapping ROIs with distinct values: the nearer ROI (painted last) owns the overlap where it keeps a cluster,
    the farther one shows through where it does not; untouched pixels keep the pre-fill."""
    S, H, W = 8, 40, 48
    boxes = np.array([[4, 5, 30, 28], [18, 12, 45, 37]])
    labels_crop = torch.ones((2, S * S), dtype=torch.int32, device=device)
    labels_crop[1, S * S // 2:] = 2                               # the lower half of crop 1 is another cluster ...
    mask = torch.ones((2, S, S), device=device)
    mask[1, S // 2:] = 0.0                                       # ... that does not overlap the stage-1 mask: dropped
    depth = torch.zeros((2, 3, S, S), device=device)
    depth[0, 2], depth[1, 2] = 1.5, 0.9                           # ROI 0 is farther: painted first
    table = roi_table(boxes, device)
    refined, plan = match_with_plan(labels_crop, mask, depth, table, 2, S, H, W, device)
    assert plan[:2].tolist() == [0, 1]
    values = torch.stack([torch.full((S * S,), 0.25, device=device), 0.5 + torch.arange(S * S, device=device) / 256.0]).contiguous()
    out = CF.paste_values(values, labels_crop, table, plan, 2, H, W, torch.full((H * W,), -7.0, device=device)).view(H, W).cpu().numpy()
    want = R.paste(values.cpu().numpy(), labels_crop.cpu().numpy(), boxes, plan.cpu().numpy(), 2, S, H, W, np.full((H, W), -7.0, np.float32))
    assert np.array_equal(out, want)
    ref = refined.view(H, W).cpu().numpy()
    assert np.array_equal(out == -7.0, ref == 0)
    assert out[13, 20] >= 0.5 and ref[13, 20] == 2               # the overlap, upper part of ROI 1: ROI 1's value
    assert out[27, 20] == 0.25 and ref[27, 20] == 1              # the overlap, dropped part of ROI 1: ROI 0 shows through
    assert out[6, 6] == 0.25 and out[36, 44] == -7.0 and out[0, 0] == -7.0


# ---- 7. uoc_conf_objects ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weak_q", [0, 1311, 65535])
def test_objects_table_is_exact(device, weak_q):
    rng = np.random.default_rng(3)
    B, H, W = 2, 37, 53
    lab = rng.choice(np.array([-3, 0, 0, 1, 2, 5, 64, 127, 128, 255], np.int32), size=(B, H, W))
    lab[1][lab[1] == 5] = 6                                      # id 5 only in frame 0, id 6 only in frame 1
    conf = rng.random((B, H, W)).astype(np.float32)
    special = np.array([np.nan, -1.0, 0.0, 1 - 2.0 ** -17, 1.0, 7.5, 0.02, 2.0 ** -16, np.inf, -0.0], np.float32)
    sel = rng.random((B, H, W)) < 0.3
    conf[sel] = rng.choice(special, size=int(sel.sum()))
    conf[0][lab[0] == 64] = np.float32(0.75)                     # a constant object: min == mean
    stats = CF.object_stats(torch.from_numpy(lab).to(device), torch.from_numpy(conf).to(device), weak_q)
    want = R.objects(lab, conf, weak_q)
    assert np.array_equal(stats.cpu().numpy(), want)
    assert want[0, 64, 2] == 49152 and want[0, 64, 1] == 49152 * want[0, 64, 0] and want[0, 6].tolist() == [0, 0, 0, 0]
    if weak_q == 1311:
        s = CF.summarize(torch.from_numpy(lab).to(device).float(), torch.from_numpy(conf).to(device), weak=0.02)
        assert s.weak_q == 1311 and np.array_equal(s.stats.cpu().numpy(), want) and np.array_equal(s.pixels, want[..., 0])
        assert s.mean[0, 64] == 0.75 and s.min[0, 64] == 0.75 and np.isnan(s.mean[0, 6]) and np.isnan(s.weak_share[0, 6])
        assert np.array_equal(s.weak_share[0, :3], want[0, :3, 3] / want[0, :3, 0])


# ---- 8. end to end on the demo frame --------------------------------------------------------------------------------
def _demo_sample(golden_dir):
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    return uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)


def _nets():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_confidence_end_to_end(device, golden_dir):
    cfg.device = device
    sample = _demo_sample(golden_dir)
    net, net_crop = _nets()
    np.random.seed(3)
    want_out, want_ref = TD.test_sample(sample, net, net_crop)
    np.random.seed(3)
    out, ref, conf = CF.segment_confidence(sample, net, net_crop)
    assert torch.equal(out, want_out) and ref is not None and torch.equal(ref, want_ref)
    _, H, W = out.shape
    assert tuple(conf.margin1.shape) == (1, H, W) and tuple(conf.second1.shape) == (1, H, W) and tuple(conf.margin.shape) == (H, W)
    assert conf.margin1.dtype == torch.float32 and conf.second1.dtype == torch.int32 and conf.margin.dtype == torch.float32
    # the three-case rule, pixel by pixel, restated from the stage-1 margins, the crop margins, the plan and the ROI table
    s2, K = conf.stage2, conf.rois
    assert K >= 1 and s2 is not None
    S = cfg.TRAIN.SYN_CROP_SIZE
    t = _native.RoiTable.from_buffer_copy(s2["table"].cpu().numpy().tobytes())
    boxes = np.array([[t.box[k][i] for i in range(4)] for k in range(K)])
    plan, labels_crop = s2["plan"].cpu().numpy(), s2["labels_crop"].cpu().numpy()
    refined = ref[0].numpy().astype(np.int32)
    _, _, ident = R.paste_source(labels_crop, boxes, plan, K, S, H, W)
    assert np.array_equal(ident, refined)
    pasted = R.paste(s2["margin_crop"].cpu().numpy(), labels_crop, boxes, plan, K, S, H, W, np.zeros((H, W), np.float32))
    labels1 = out[0].numpy().astype(np.int32)
    assert np.array_equal(labels1, s2["labels1"].view(H, W).cpu().numpy())
    want_margin = R.final_margin(refined, labels1, conf.margin1[0].cpu().numpy(), pasted)
    got_margin = conf.margin.cpu().numpy()
    assert np.array_equal(got_margin, want_margin)
    disagree = (refined == 0) & (labels1 != 0)
    assert (got_margin[disagree] == 0).all() and (got_margin >= 0).all() and (got_margin <= 1).all()
    assert (refined != 0).sum() > 1000 and ((refined == 0) & (labels1 == 0)).sum() > 1000
    # per_object is the summary of the final map
    again = CF.summarize(ref[:1].to(device), conf.margin[None])
    assert np.array_equal(conf.per_object.stats.cpu().numpy(), again.stats.cpu().numpy())
    assert np.array_equal(conf.per_object.stats.cpu().numpy(), R.objects(refined[None], got_margin[None], CF.weak_to_q(0.02)))
    ids = [int(i) for i in np.unique(refined) if i > 0]
    assert all(conf.per_object.pixels[0, i] == (refined == i).sum() for i in ids)
    assert all(0 <= conf.per_object.min[0, i] <= conf.per_object.mean[0, i] <= 1 for i in ids)
    # segment_objects(confidence=True): every other item unchanged, the confidence item last
    np.random.seed(3)
    plain = O.segment_objects(sample, net, net_crop)
    np.random.seed(3)
    both = O.segment_objects(sample, net, net_crop, confidence=True)
    assert len(plain) == 3 and len(both) == 4
    assert torch.equal(plain[0], both[0]) and torch.equal(plain[1], both[1]) and torch.equal(both[0], want_out)
    for k in ("frame", "label", "pixels", "count", "box", "centroid", "cov", "points", "pixel_index", "offsets"):
        assert torch.equal(getattr(plain[2], k).cpu(), getattr(both[2], k).cpu()), k
    assert torch.equal(both[3].margin, conf.margin) and torch.equal(both[3].margin1, conf.margin1)
    # no crop network: the stage-1 margins are the answer
    np.random.seed(3)
    out1, none, conf1 = CF.segment_confidence(sample, net, None)
    assert none is None and torch.equal(out1, want_out) and conf1.stage2 is None
    assert torch.equal(conf1.margin, conf1.margin1[0]) and torch.equal(conf1.margin1, conf.margin1)
    assert np.array_equal(conf1.per_object.stats.cpu().numpy(),
                          R.objects(labels1[None], conf1.margin1.cpu().numpy(), CF.weak_to_q(0.02)))


# ---- 9. error paths on the device: a rejected call writes nothing ---------------------------------------------------
def test_rejected_calls_leave_the_outputs_untouched(device):
    rng = np.random.default_rng(9)
    L = _native.lib()
    n, m = 100, 10
    Xd, Zd = torch.from_numpy(unit(rng, 1, n, 64)).to(device), torch.from_numpy(unit(rng, 1, m, 64)).to(device)
    sld = torch.zeros((1, m), dtype=torch.int32, device=device)
    nud = torch.ones((1,), dtype=torch.int32, device=device)
    outs = [torch.full((1, n), -77, dtype=torch.int32, device=device) for _ in range(4)]
    margin = torch.full((1, n), -77.0, device=device)
    nws = L.uoc_ms_confidence_workspace_bytes(1, n, m, 1)
    ws = torch.full((nws + 16,), 0x5A, dtype=torch.uint8, device=device)

    def call(**kw):
        a = dict(halves=1, m=m, metric=0, labels=outs[0], ws=ws, ws_bytes=nws)
        a.update(kw)
        with torch.cuda.device(device):
            return L.uoc_ms_confidence(_native.ptr(Xd), a["halves"], 1, n, _native.ptr(Zd), _native.ptr(sld), _native.ptr(nud), a["m"],
                                       a["metric"], _native.ptr(a["labels"]), _native.ptr(margin), _native.ptr(outs[1]),
                                       _native.ptr(outs[2]), _native.ptr(outs[3]), _native.ptr(a["ws"]), a["ws_bytes"],
                                       _native.stream_ptr(device))
    for kw in (dict(metric=_native.METRIC_EUCLIDEAN), dict(m=129), dict(halves=3), dict(ws_bytes=nws - 1), dict(ws=ws[8:]),
               dict(labels=sld)):
        assert call(**kw) == -22, kw
    stats = torch.full((1, 128, 4), -77, dtype=torch.int64, device=device)
    lab2 = torch.zeros((1, 4, 4), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        assert L.uoc_conf_objects(_native.ptr(lab2), _native.ptr(margin), 1, 4, 4, 70000, _native.ptr(stats), _native.stream_ptr(device)) == -22
        assert L.uoc_conf_paste(_native.ptr(margin), _native.ptr(lab2), _native.ptr(ws), _native.ptr(lab2), 0, 8, 4, 4, _native.ptr(margin),
                                _native.stream_ptr(device)) == -22
    torch.cuda.synchronize(device)
    assert all((o == -77).all() for o in outs) and (margin == -77.0).all() and (ws == 0x5A).all() and (stats == -77).all()
    assert (sld == 0).all()
    assert call() == 0                                           # the same buffers are accepted once the arguments are right
    torch.cuda.synchronize(device)
    assert (outs[0] == 0).all() and (margin == 1.0).all() and (outs[1] == -1).all() and (outs[3] == -1).all()
