"""The two-stage glue kernels (csrc/roi.hip) on the engineered cases of tests/glue_cases.py, against oracle/glue_oracle.py:
depth-coverage filter, ROI boxes, crop + resize, crop-cluster matching, paint order and paste-back, uoc_labels_to_u8 and
the argument checks of the ROI entry points.  Integer outputs are bit-exact; the bilinear crops are held to the bound of
glue_cases.bilinear_bound.  tests/test_glue_cases_host.py proves on the CPU that every case sits on its edge."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import glue_oracle as G
from tests import glue_cases as C
from unseenobjectclustering_amd import _native
from unseenobjectclustering_amd.fcn import test_dataset as TD
from unseenobjectclustering_amd.fcn.config import cfg

pytestmark = pytest.mark.gpu

NAN = float("nan")


@contextlib.contextmanager
def crop_size(S, device):
    """cfg.TRAIN.SYN_CROP_SIZE = S for the body, restored whatever happens."""
    cfg.device = device
    old = cfg.TRAIN.SYN_CROP_SIZE
    cfg.TRAIN.SYN_CROP_SIZE = S
    try:
        yield
    finally:
        cfg.TRAIN.SYN_CROP_SIZE = old


def _table_dev(t, device):
    return torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(device)


def _last_error():
    return _native.lib().uoc_last_error().decode("utf-8", "replace")


def _z_plane(depth_d, H, W):
    return ctypes.c_void_p(depth_d.data_ptr() + 2 * H * W * 4)


# ---- 2. depth-coverage filter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", C.THRESHOLDS)
def test_filter_fraction_at_the_threshold(device, thr):
    """Fractions equal to the threshold are kept (`<` in float32), the nearest ones below are removed; z <= 0, -0,
    negative and NaN z do not count; ids with gaps up to 127; an object of two blobs; label 0 without any depth."""
    cfg.device = device
    labels, depth, _ = C.filter_frame()
    want = G.filter_labels_depth(labels, depth, thr)
    got = TD.filter_labels_depth(labels, depth.to(device), thr)
    assert got.dtype == labels.dtype and got.device == labels.device
    assert torch.equal(got, want)


@pytest.mark.parametrize("thr", C.THRESHOLDS)
def test_filter_batch_of_three(device, thr):
    """Per-item reset of the statistics and the batch stride of the z plane: a label that fails in one item only, labels
    that exist in one item only."""
    cfg.device = device
    labels, depth, _ = C.filter_batch()
    want = G.filter_labels_depth(labels, depth, thr)
    got = TD.filter_labels_depth(labels, depth.to(device), thr)
    assert torch.equal(got, want)


@pytest.mark.parametrize("thr", C.THRESHOLDS)
def test_filter_raw_abi_leaves_foreign_ids_alone(device, thr):
    """uoc_filter_labels_depth and uoc_roi_build through the C ABI: pixels with ids outside [0, 128) stay as they are and
    change the result for no valid label (the Python wrapper refuses such maps)."""
    cfg.device = device
    raw, depth, clean, invalid = C.filter_raw_abi()
    with pytest.raises(ValueError):
        TD.filter_labels_depth(raw.float(), depth.to(device), thr)
    filtered = G.filter_labels_depth(clean.float(), depth, thr)
    want = filtered.to(torch.int32)
    want[invalid] = raw[invalid]
    ws = TD._ws(device)
    B, H, W = raw.shape
    depth_d = depth.to(device).contiguous()
    lab = raw.to(device).contiguous()
    _native.call("uoc_filter_labels_depth", device, lab, _z_plane(depth_d, H, W), 3 * H * W, B, H, W, float(thr), ws, ws.numel())
    assert torch.equal(lab.cpu(), want)
    # the fused form: filter + ROI table in one call
    lab = raw[0].to(device).contiguous()
    t = TD._read_table(TD._build_rois(lab, _z_plane(depth_d, H, W), H, W, device, thr))
    ids, boxes = G.roi_boxes(filtered[0])
    assert torch.equal(lab.cpu(), want[0])
    assert t.K == len(ids) and list(t.label[:t.K]) == ids
    assert [list(t.box[k]) for k in range(t.K)] == boxes.tolist()


# ---- 3. boxes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.box_cases()))
def test_boxes(device, name):
    """Padding products of x.5 (round half to even), one clamped border at a time, a whole-frame object, single pixels,
    rows and columns, frames of one row / one column, 127 objects, an object of two blobs."""
    lab = C.box_cases()[name]
    H, W = lab.shape
    ids, want = G.roi_boxes(lab)
    with crop_size(3, device):
        rgb_c, mask_c, rois, depth_c = TD.crop_rois(torch.zeros(1, 3, H, W, device=device), lab[None], None)
        assert rois.dtype == torch.float32 and tuple(rois.shape) == (len(ids), 4) and depth_c is None
        assert torch.equal(rois.cpu(), want.float())
        assert tuple(rgb_c.shape) == (len(ids), 3, 3, 3) and tuple(mask_c.shape) == (len(ids), 3, 3)
        # K and the ascending label order, from the table uoc_roi_build writes; without depth the map is not touched
        lab0 = lab.to(torch.int32).to(device)
        t = TD._read_table(TD._build_rois(lab0, ctypes.c_void_p(0), H, W, device))
        assert t.K == len(ids) and list(t.label[:t.K]) == ids
        assert [list(t.box[k]) for k in range(t.K)] == want.tolist()
        assert torch.equal(lab0.cpu(), lab.to(torch.int32))


# ---- 4. crops --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    H, W = C.SWEEP_H, C.SWEEP_W
    boxes = C.sweep_boxes(41)
    rgb, depth = C.ramp_noise(3, H, W, 42), C.ramp_noise(3, H, W, 43)
    return dict(boxes=boxes, rgb=rgb, depth=depth, lab=C.id_pattern(H, W), ids=[1 + k % 5 for k in range(len(boxes))],
                bound_rgb=C.bilinear_bound(rgb, boxes), bound_depth=C.bilinear_bound(depth, boxes))


def _guarded(img, device):
    """[3,H,W] on the device as the first three planes of a four-plane buffer whose last plane is NaN: a tap behind the
    last pixel of the image stays inside the allocation and shows."""
    buf = torch.full((4,) + tuple(img.shape[1:]), NAN, device=device)
    buf[:3] = img.to(device)
    return buf[:3]


def _device_crops(rgb, depth, lab, boxes, ids, device):
    """TD._crop over hand-made tables of up to 127 boxes -> rgb crops, mask crops, depth crops (CPU)."""
    H, W = lab.shape
    rgb_d, lab_d = _guarded(rgb, device), lab.to(torch.int32).to(device)
    depth_d = _guarded(depth, device) if depth is not None else None
    parts = []
    for a in range(0, len(boxes), 127):
        K = len(boxes[a:a + 127])
        table = _table_dev(C.roi_table(boxes[a:a + 127], ids[a:a + 127]), device)
        parts.append([None if t is None else t.cpu() for t in TD._crop(rgb_d, depth_d, lab_d, table, K, H, W, device)])
    return [None if p[0] is None else torch.cat(p) for p in zip(*parts)]


def _check_bilinear(got, img, boxes, bound, S):
    """Every position of every channel against F.interpolate on the float64 copy -> largest error / bound."""
    assert bool(torch.isfinite(got).all())
    want = C.ref_bilinear(img.double(), boxes, S)
    err = (got.double() - want).abs().amax(dim=(1, 2, 3)).numpy()
    ratio = err / bound
    worst = int(ratio.argmax())
    print("S=%d: largest bilinear error/bound %.3f (error %.3e, window %s)" % (S, ratio[worst], err[worst], boxes[worst].tolist()))
    assert (err <= bound).all(), (S, boxes[worst].tolist(), float(err[worst]), float(bound[worst]))
    return float(ratio[worst])


@pytest.mark.parametrize("S", C.SWEEP_S)
def test_crop_sweep(device, sweep, S):
    """Every window extent ch, cw in 1..40 (cw == 1, ch == 1 and S == 1 included) against this S, 127 boxes per launch.
    Mask crops (nearest) bit-exact at every position against the oracle's float32 F.interpolate, on a label map where a
    wrong index lands on another id; rgb and depth crops at every position against F.interpolate on the float64 input,
    within 2^-23 ((cw-1) max|dx| + (ch-1) max|dy|) + 8 2^-24 max|v| of their own window.
    Largest error / bound measured on the MI355X over the sweep: 0.41 (S = 16, depth crops; 0.38 for the rgb crops),
    where the oracle's own float32 F.interpolate reaches 0.51 on the CPU."""
    boxes, ids = sweep["boxes"], sweep["ids"]
    with crop_size(S, device):
        rgb_c, mask_c, depth_c = _device_crops(sweep["rgb"], sweep["depth"], sweep["lab"], boxes, ids, device)
        assert tuple(rgb_c.shape) == (len(boxes), 3, S, S) == tuple(depth_c.shape)
        want_mask = C.ref_mask(sweep["lab"], ids, boxes, S)
        assert 0 < float(want_mask.mean()) < 1
        assert torch.equal(mask_c, want_mask)
        _check_bilinear(rgb_c, sweep["rgb"], boxes, sweep["bound_rgb"], S)
        _check_bilinear(depth_c, sweep["depth"], boxes, sweep["bound_depth"], S)


@pytest.mark.parametrize("S", C.SWEEP_S)
def test_crop_reads_only_its_window(device, S):
    """Windows in a frame that is NaN everywhere else: the taps of the last row and column (weight 0) must stay inside."""
    rgb, depth, lab, boxes = C.poisoned_windows()
    ids = [1 + k % 5 for k in range(len(boxes))]
    with crop_size(S, device):
        rgb_c, mask_c, depth_c = _device_crops(rgb, depth, lab, boxes, ids, device)
        assert torch.equal(mask_c, C.ref_mask(lab, ids, boxes, S))
        clean = lambda t: torch.nan_to_num(t, nan=0.0)        # the bound looks at the windows only
        _check_bilinear(rgb_c, clean(rgb), boxes, C.bilinear_bound(clean(rgb), boxes), S)
        _check_bilinear(depth_c, clean(depth), boxes, C.bilinear_bound(clean(depth), boxes), S)


@pytest.mark.parametrize("name,S", [("padding", 7), ("thin", 2), ("frame_1xN", 3), ("frame_Nx1", 1), ("blobs", 16)])
def test_crop_rois_with_and_without_depth(device, name, S):
    """TD.crop_rois against the oracle's crop_rois: boxes and mask crops bit-exact, rgb and depth crops within the bound
    of the float64 resize; COLOR input (depth=None) gives no depth crops and the same rgb and mask crops, bit for bit."""
    lab = C.box_cases()[name]
    H, W = lab.shape
    rgb, depth = C.ramp_noise(3, H, W, 51)[None], C.ramp_noise(3, H, W, 52)[None]
    with crop_size(S, device):
        _, want_mask, want_rois, _ = G.crop_rois(rgb, lab[None], depth, crop_size=S)
        rgb_c, mask_c, rois, depth_c = TD.crop_rois(rgb.to(device), lab[None], depth.to(device))
        assert torch.equal(rois.cpu(), want_rois) and torch.equal(mask_c.cpu(), want_mask)
        boxes = want_rois.long().numpy()
        _check_bilinear(rgb_c.cpu(), rgb[0], boxes, C.bilinear_bound(rgb[0], boxes), S)
        _check_bilinear(depth_c.cpu(), depth[0], boxes, C.bilinear_bound(depth[0], boxes), S)
        rgb_n, mask_n, rois_n, depth_n = TD.crop_rois(rgb.to(device), lab[None], None)
        assert depth_n is None
        assert torch.equal(rgb_n, rgb_c) and torch.equal(mask_n, mask_c) and torch.equal(rois_n, rois)


# ---- 5. matching and paste -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paste_frames():
    return C.paste_sweep_frames()


@pytest.mark.parametrize("S", C.SWEEP_S)
def test_paste_sweep(device, paste_frames, S):
    """Nearest resize of an SxS crop back to every box size h, w in 1..40, a few disjoint boxes per call, crop labels
    that differ between neighbouring crop pixels; every cluster kept, no depth.  Refined map and labels_crop bit-exact
    against the oracle's match_label_crop (its vectorised restatement, pinned to it on the CPU)."""
    H, W = 64, 72
    init = torch.zeros(1, H, W)
    with crop_size(S, device):
        for boxes in paste_frames:
            K = len(boxes)
            labels, rois = C.paste_labels(K, S), torch.from_numpy(boxes).float()
            want = C.match_all_kept_no_depth(labels, rois, H, W)
            refined, labels_out = TD.match_label_crop(init, labels.to(device), torch.ones(K, S, S, device=device), rois, None)
            assert refined.dtype == torch.float32 and tuple(refined.shape) == (1, H, W)
            assert torch.equal(refined[0].cpu(), want), boxes.tolist()
            assert torch.equal(labels_out.cpu(), labels)


def _match_both(c, device, with_depth=True):
    depth = c["depth"] if with_depth else None
    S = c["labels_crop"].shape[-1]
    want = G.match_label_crop(c["initial_masks"], c["labels_crop"], c["mask"], c["rois"], depth)
    with crop_size(S, device):
        got = TD.match_label_crop(c["initial_masks"], c["labels_crop"].to(device), c["mask"].to(device), c["rois"],
                                  depth.to(device) if with_depth else None)
    assert got[0].dtype == torch.float32 and got[0].shape == c["initial_masks"].shape
    assert torch.equal(got[0].cpu(), want[0]), "refined map"
    assert torch.equal(got[1].cpu(), want[1]), "labels_crop with -1 for rejected clusters"
    return want


@pytest.mark.parametrize("with_depth", [True, False])
def test_match_overlap_of_exactly_one_half(device, with_depth):
    """Overlap 0.5 kept, the nearest fraction below dropped; cluster id 127, ids with gaps, id 0 kept and renumbered; a ROI
    whose clusters are all dropped paints nothing."""
    refined, labels_out = _match_both(C.overlap_case(), device, with_depth)
    assert bool((labels_out[1] == -1).all()) and int(refined.max()) == 3


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("perm", C.ORDER_PERMS)
def test_match_paint_order(device, perm, with_depth):
    """Overlapping boxes: the nearer ROI overwrites the farther one, a dropped cluster does not overwrite, bit-equal mean
    depths fall back to the index order, a NaN key (K < 64) is ordered as CPython's sort does; without depth the box
    areas (two of them equal) decide."""
    _match_both(C.order_case(perm), device, with_depth)


def test_match_raw_abi_ignores_foreign_crop_ids(device):
    """uoc_roi_match through the C ABI with crop labels outside [0, 128) (the Python wrapper refuses them): they count
    for no cluster, do not enter a mean depth unless nothing is kept, and paint nothing — the oracle on the crops with
    those pixels at -1."""
    c, raw, clean = C.match_raw_abi()
    K, S = raw.shape[0], raw.shape[-1]
    _, H, W = c["initial_masks"].shape
    want, _ = G.match_label_crop(c["initial_masks"], clean, c["mask"], c["rois"], c["depth"])
    want_keep, _, _ = C.oracle_keep_meanz(clean, c["mask"], c["depth"])
    with crop_size(S, device):
        with pytest.raises(ValueError):
            TD.match_label_crop(c["initial_masks"], raw.float().to(device), c["mask"].to(device), c["rois"], c["depth"].to(device))
        table = _table_dev(C.roi_table(c["rois"].long().tolist(), [0] * K), device)
        refined, keep = TD._match(raw.reshape(K, -1).to(device), c["mask"].to(device), c["depth"].to(device), table, K, H, W, device)
        assert torch.equal(keep.cpu(), want_keep)
        assert torch.equal(refined.view(H, W).cpu(), want[0].to(torch.int32))


def _stats_inputs():
    c = C.overlap_case()
    cases = {"overlap": (c["labels_crop"], c["mask"], c["depth"]),
             "all_dropped": (c["labels_crop"][1:], c["mask"][1:], c["depth"][1:])}
    for K in (1, 2, 127):
        cases["random%d" % K] = C.stats_case(K)
    return cases


@pytest.mark.parametrize("name", ["overlap", "all_dropped", "random1", "random2", "random127"])
def test_roi_match_stats_alone(device, name):
    """uoc_roi_match_stats: the keep table and the mean depth of every ROI against the oracle's own quantities, for K in
    {1, 2, 127}; a ROI with nothing kept takes its mean over all its pixels, one without any z > 0 gives NaN."""
    labels, mask, depth = _stats_inputs()[name]
    K, S = labels.shape[0], labels.shape[-1]
    want_keep, want_meanz, _ = C.oracle_keep_meanz(labels, mask, depth)
    ws = TD._ws(device)
    lab_d = labels.to(torch.int32).reshape(K, -1).to(device)
    mask_d, depth_d = mask.to(device).contiguous(), depth.to(device).contiguous()
    for with_depth in (True, False):
        keep = torch.full((K, 128), -7, dtype=torch.int32, device=device)
        meanz = torch.full((K,), 123.0, device=device)
        _native.call("uoc_roi_match_stats", device, lab_d, mask_d, depth_d if with_depth else None, K, S, keep,
                     meanz if with_depth else None, ws, ws.numel())
        assert torch.equal(keep.cpu(), want_keep)
        got = meanz.cpu()
        if not with_depth:
            assert bool((got == 123.0).all())
            continue
        nan = torch.isnan(want_meanz)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got[~nan].view(torch.int32), want_meanz[~nan].view(torch.int32)), "bit-equal means"
    if name == "all_dropped":
        assert int(want_keep.sum()) == 0 and not bool(torch.isnan(want_meanz).any())


# ---- 6. uoc_labels_to_u8 ---------------------------------------------------------------------------------------------
def _to_u8(lab_d, n, preset, device):
    out = torch.full((n + 8,), 0xAA, dtype=torch.uint8, device=device)
    top = torch.tensor([preset], dtype=torch.int32, device=device)
    _native.call("uoc_labels_to_u8", device, lab_d, n, out, top)
    return out.cpu().numpy(), int(top.item())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 4 * 256 * 1024 + 3])
def test_labels_to_u8(device, n):
    """Against numpy (astype(uint8), max): vector body, scalar tail (the largest id sits in it) and, at the last size,
    the grid-stride loop; the running maximum preset to 0, above and below the map's maximum; an all-zero map leaves it
    untouched; nothing is written behind n."""
    rng = np.random.RandomState(n % 9973)
    lab = rng.randint(0, 127, size=n).astype(np.int32)
    lab[n - 1] = 127
    lab_d = torch.from_numpy(lab).to(device)
    assert lab_d.data_ptr() % 16 == 0
    for preset in (0, 200, 5, -7):
        out, top = _to_u8(lab_d, n, preset, device)
        assert np.array_equal(out[:n], lab.astype(np.uint8)) and (out[n:] == 0xAA).all()
        assert top == max(preset, int(lab.max())), preset
    zeros = torch.zeros(n, dtype=torch.int32, device=device)
    for preset in (0, 9, -7):
        out, top = _to_u8(zeros, n, preset, device)
        assert not out[:n].any() and (out[n:] == 0xAA).all()
        assert top == preset, "an all-zero map leaves the running maximum untouched"


def test_labels_to_u8_refuses_misaligned_pointers(device):
    L = _native.lib()
    buf = torch.full((65,), 3, dtype=torch.int32, device=device)
    out = torch.full((72,), 0xAA, dtype=torch.uint8, device=device)
    top = torch.tensor([-7], dtype=torch.int32, device=device)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    for lab_p, out_p in ((view, out), (buf, out[1:])):
        with torch.cuda.device(device):
            rc = L.uoc_labels_to_u8(_native.ptr(lab_p), 64, _native.ptr(out_p), _native.ptr(top), _native.stream_ptr(device))
        assert rc != 0 and "misaligned" in _last_error()
        torch.cuda.synchronize(device)
        assert bool((out == 0xAA).all()) and int(top.item()) == -7, "nothing was launched"


# ---- 7. argument errors of the ROI entry points ----------------------------------------------------------------------
POISON_I, POISON_F = -77, 77.5


class _Args:
    """Valid arguments of the four ROI entry points for K = 2, S = 4 in an 8x8 frame (buffers sized for K = 128), the
    outputs pre-filled; call(name, **changed) runs one entry point with some arguments replaced."""

    def __init__(self, device):
        K, S, H, W = 2, 4, 8, 8
        self.device = device
        dev = dict(device=device)
        self.v = dict(K=K, S=S, H=H, W=W,
                      rgb=torch.zeros(3, H, W, **dev), xyz=torch.ones(3, H, W, **dev),
                      labels=torch.ones(H, W, dtype=torch.int32, **dev),
                      table=_table_dev(C.roi_table([(0, 0, 3, 3), (2, 2, 7, 7)], [1, 1]), device),
                      labels_crop=torch.zeros(128, S * S, dtype=torch.int32, **dev), mask=torch.ones(128, S, S, **dev),
                      xyz_crops_in=torch.ones(128, 3, S, S, **dev),
                      map=torch.ones(128, 128, dtype=torch.int32, **dev), order=torch.zeros(128, dtype=torch.int32, **dev),
                      status=torch.full((1,), POISON_I, dtype=torch.int32, **dev),
                      ws=TD._ws(device), ws_bytes=TD._ws(device).numel())
        self.out = dict(rgb_crops=torch.full((128, 3, S, S), POISON_F, **dev), xyz_crops=torch.full((128, 3, S, S), POISON_F, **dev),
                        mask_crops=torch.full((128, S, S), POISON_F, **dev),
                        keep=torch.full((128, 128), POISON_I, dtype=torch.int32, **dev), meanz=torch.full((128,), POISON_F, **dev),
                        refined=torch.full((H * W,), POISON_I, dtype=torch.int32, **dev),
                        plan=torch.full((128 + 128 * 128,), POISON_I, dtype=torch.int32, **dev))

    def call(self, name, **changed):
        a = dict(self.v, **self.out)
        a.update(changed)
        p = lambda key: _native.ptr(a[key])
        L, st = _native.lib(), _native.stream_ptr(self.device)
        with torch.cuda.device(self.device):
            if name == "uoc_roi_crop":
                return L.uoc_roi_crop(p("rgb"), p("xyz"), p("labels"), a["H"], a["W"], p("table"), a["K"], a["S"], p("rgb_crops"),
                                      p("xyz_crops"), p("mask_crops"), st)
            if name == "uoc_roi_match_stats":
                return L.uoc_roi_match_stats(p("labels_crop"), p("mask"), p("xyz_crops_in"), a["K"], a["S"], p("keep"), p("meanz"),
                                             p("ws"), a["ws_bytes"], st)
            if name == "uoc_roi_paste":
                return L.uoc_roi_paste(p("labels_crop"), p("table"), p("map"), p("order"), a["K"], a["S"], a["H"], a["W"],
                                       p("refined"), st)
            assert name == "uoc_roi_match"
            return L.uoc_roi_match(p("labels_crop"), p("mask"), p("xyz_crops_in"), p("table"), a["K"], a["S"], a["H"], a["W"],
                                   p("refined"), p("keep"), p("plan"), p("status"), p("ws"), a["ws_bytes"], st)

    def untouched(self):
        torch.cuda.synchronize(self.device)
        ok = all(bool((t == (POISON_F if t.dtype == torch.float32 else POISON_I)).all()) for t in self.out.values())
        return ok and int(self.v["status"].item()) == POISON_I


ENTRY_POINTS = ("uoc_roi_crop", "uoc_roi_match_stats", "uoc_roi_paste", "uoc_roi_match")


def test_roi_entry_points_refuse_bad_arguments(device):
    """K = 0, K = 128, S = 0, a workspace one byte short, d_xyz without d_xyz_crops: a non-zero code, a message, and the
    output buffers as they were.  All of these are refused on the host, before any launch."""
    a = _Args(device)
    short = _native.lib().uoc_roi_workspace_bytes() - 1
    refused = [(name, dict(K=K), "out of range") for name in ENTRY_POINTS for K in (0, 128)]
    refused += [(name, dict(S=0), "out of range") for name in ENTRY_POINTS]
    refused += [(name, dict(ws_bytes=short), "workspace too small") for name in ("uoc_roi_match_stats", "uoc_roi_match")]
    refused += [("uoc_roi_crop", dict(xyz_crops=None), "given together"), ("uoc_roi_crop", dict(xyz=None), "given together")]
    for name, changed, message in refused:
        rc = a.call(name, **changed)
        assert rc != 0, (name, changed)
        assert message in _last_error(), (name, changed, _last_error())
        assert a.untouched(), (name, changed)
    # the filter and the table build check their workspace the same way
    L, ws = _native.lib(), TD._ws(device)
    lab = torch.ones(8, 8, dtype=torch.int32, device=device)
    z = torch.zeros(8, 8, device=device)
    table = torch.full((_native.ROI_TABLE_BYTES,), 0xAA, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        rc1 = L.uoc_filter_labels_depth(_native.ptr(lab), _native.ptr(z), 64, 1, 8, 8, 0.8, _native.ptr(ws), short,
                                        _native.stream_ptr(device))
        e1 = _last_error()
        rc2 = L.uoc_roi_build(_native.ptr(lab), _native.ptr(z), 8, 8, 0.8, 0.25, _native.ptr(table), _native.ptr(ws), short,
                              _native.stream_ptr(device))
        e2 = _last_error()
    torch.cuda.synchronize(device)
    assert rc1 != 0 and rc2 != 0 and "workspace too small" in e1 and "workspace too small" in e2
    assert bool((lab == 1).all()) and bool((table == 0xAA).all())
    # ... and with everything in order the same arguments are accepted
    for name in ENTRY_POINTS:
        _native.check(a.call(name), name)
    torch.cuda.synchronize(device)
    assert not a.untouched()
