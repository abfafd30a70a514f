"""CPU proof that every engineered case of tests/glue_cases.py sits on the edge it is named for, using only
oracle/glue_oracle.py: a case that misses its edge would test nothing on the GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import glue_oracle as G
from tests import glue_cases as C


# ---- depth-coverage filter -------------------------------------------------------------------------------------------
def _fractions(labels, depth):
    """{(item, id): (pixels, pixels with z > 0)} counted from the tensors, not taken from the spec."""
    out = {}
    for b in range(labels.shape[0]):
        for mid in torch.unique(labels[b]).tolist():
            sel = labels[b] == mid
            out[(b, int(mid))] = (int(sel.sum()), int((depth[b, 2][sel] > 0).sum()))
    return out


def test_filter_frame_fractions_sit_on_the_thresholds():
    labels, depth, spec = C.filter_frame()
    counted = _fractions(labels, depth)
    assert sorted(m for _, m in counted) == sorted([0] + [s["id"] for s in spec]), "ids with gaps, 127 the largest"
    assert counted[(0, 0)][1] == 0, "label 0 has no depth at all"
    hit = {0.5: {"at": 0, "below": 0}, 0.8: {"at": 0, "below": 0}}
    for s in spec:
        cnt, zpos = counted[(0, s["id"])]
        assert (cnt, zpos) == (s["cnt"], s["zpos"])
        frac = np.float32(zpos) / np.float32(cnt)
        kind, thr = s["edge"]
        if kind == "at":
            assert frac == np.float32(thr), "the float32 fraction IS the float32 threshold"
        elif kind == "below":
            assert frac < np.float32(thr) <= np.float32(zpos + 1) / np.float32(cnt), "the nearest fraction below"
        else:
            assert zpos == 0
        hit[thr][kind] = hit[thr].get(kind, 0) + 1
    assert all(hit[thr][kind] >= 2 for thr in hit for kind in ("at", "below")), hit
    # the oracle keeps the labels at a threshold and removes the ones just below, at both thresholds
    for thr in C.THRESHOLDS:
        out = G.filter_labels_depth(labels, depth, thr)
        for s in spec:
            frac = s["zpos"] / s["cnt"]         # exact comparison in rationals: 4/5 vs 0.8 means "equal"
            at = s["edge"] == ("at", thr)
            want_kept = at or frac > thr
            assert bool((out == s["id"]).any()) == want_kept, (thr, s)
            assert int((out == s["id"]).sum()) in (0, s["cnt"])


def test_filter_frame_depth_values_and_blobs():
    labels, depth, spec = C.filter_frame()
    z = depth[0, 2][labels[0] > 0]
    assert torch.isnan(z).any() and (z < 0).any() and (z == 0).any() and (z > 0).any()
    assert bool((depth[0, :2] > 0).all()), "x and y planes are positive: reading the wrong plane covers everything"
    ys, xs = torch.nonzero(labels[0] == 33, as_tuple=True)
    assert int(ys.max() - ys.min()) > 15, "label 33 is two distant blobs"


def test_filter_batch_differs_per_item():
    labels, depth, spec = C.filter_batch()
    out = G.filter_labels_depth(labels, depth, 0.8)
    present = lambda t, b, mid: bool((t[b] == mid).any())
    assert [present(labels, b, 9) for b in range(3)] == [False, True, False]
    assert [present(labels, b, 11) for b in range(3)] == [False, True, False]
    assert [present(out, b, 5) for b in range(3)] == [True, False, True], "label 5 fails in item 1 only"
    assert [present(out, b, 6) for b in range(3)] == [True, True, False], "label 6 fails in item 2 only"
    assert not present(out, 1, 9) and present(out, 1, 11)
    # with statistics carried over from item to item both would pass: that is what the case is for
    counted = _fractions(labels, depth)
    for mid, upto in ((5, 1), (6, 2)):
        cnt = sum(counted[(b, mid)][0] for b in range(upto + 1))
        pos = sum(counted[(b, mid)][1] for b in range(upto + 1))
        assert not np.float32(pos) / np.float32(cnt) < np.float32(0.8)


def test_filter_raw_abi_ids_would_alias_labels_at_the_threshold():
    raw, depth, clean, invalid = C.filter_raw_abi()
    assert int(invalid.sum()) == 3 * len(C.INVALID_IDS)
    assert set(raw[invalid].tolist()) == set(C.INVALID_IDS)
    assert bool((clean[invalid] == 0).all()) and torch.equal(raw[~invalid], clean[~invalid])
    assert not bool((depth[0, 2][invalid[0]] > 0).any())
    at = {s["id"] for s in C.FILTER_SPEC if s["edge"] == ("at", 0.8)}
    assert {10000 % 128, -1 % 128} <= at, "taken modulo 128 they would push labels 16 and 127 below 0.8"
    out = G.filter_labels_depth(clean.float(), depth, 0.8)
    assert bool((out == 16).any()) and bool((out == 127).any())


# ---- boxes -----------------------------------------------------------------------------------------------------------
def _tight(lab, mid):
    ys, xs = torch.nonzero(lab == mid, as_tuple=True)
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def test_box_padding_products_are_halves_and_round_to_even():
    lab, meta = C.box_padding()
    H, W = lab.shape
    ids, boxes = G.roi_boxes(lab)
    assert ids == sorted(m[0] for m in meta)
    assert {m[1] for m in meta} == set(C.PAD_EXTENTS) == {m[2] for m in meta}
    halves = [e for e in C.PAD_EXTENTS if (e * G.PAD_FRACTION) % 1 == 0.5]
    assert [e * G.PAD_FRACTION for e in halves] == [0.5, 1.5, 2.5, 3.5]
    assert [C.PAD_EXPECT[e] for e in halves] == [0, 2, 2, 4] != [math.floor(e * G.PAD_FRACTION + 0.5) for e in halves]
    for (mid, ex, ey), box in zip(sorted(meta), boxes.tolist()):
        x0, y0, x1, y1 = _tight(lab, mid)
        assert (x1 - x0, y1 - y0) == (ex, ey)
        px, py = C.PAD_EXPECT[ex], C.PAD_EXPECT[ey]
        assert box == [x0 - px, y0 - py, x1 + px, y1 + py], "padded as rounded half to even"
        assert box[0] > 0 and box[1] > 0 and box[2] < W - 1 and box[3] < H - 1, "and not clamped"


def test_box_clamp_hits_one_border_each():
    lab, sides = C.box_clamp()
    H, W = lab.shape
    ids, boxes = G.roi_boxes(lab)
    limit = (0, 0, W - 1, H - 1)
    for mid, box in zip(ids, boxes.tolist()):
        x0, y0, x1, y1 = _tight(lab, mid)
        free = [x0 - 2, y0 - 2, x1 + 2, y1 + 2]          # extent 6: padding round(1.5) = 2
        differs = [i for i in range(4) if box[i] != free[i]]
        assert differs == [sides[mid]] and box[sides[mid]] == limit[sides[mid]]
    assert sorted(sides.values()) == [0, 1, 2, 3]
    whole = C.box_whole_frame()
    ids, boxes = G.roi_boxes(whole)
    assert not bool((whole == 0).any()) and boxes.tolist() == [[0, 0, whole.shape[1] - 1, whole.shape[0] - 1]]


def test_box_thin_objects_and_frames():
    lab = C.box_thin()
    extents = {mid: (_tight(lab, mid)[2] - _tight(lab, mid)[0], _tight(lab, mid)[3] - _tight(lab, mid)[1]) for mid in range(1, 6)}
    assert extents == {1: (0, 0), 2: (0, 0), 3: (14, 0), 4: (0, 10), 5: (0, 0)}
    ids, boxes = G.roi_boxes(lab)
    H, W = lab.shape
    assert boxes[0].tolist() == [0, 0, 0, 0] and boxes[4].tolist() == [W - 1, H - 1, W - 1, H - 1]
    row, col = C.box_thin_frames()
    assert row.shape == (1, 13) and col.shape == (13, 1)
    assert G.roi_boxes(row)[1].tolist() == [[1, 0, 3, 0], [6, 0, 6, 0], [7, 0, 12, 0]]
    assert G.roi_boxes(col)[1].tolist() == [[0, 1, 0, 3], [0, 6, 0, 6], [0, 7, 0, 12]]


def test_box_many_fills_the_table_and_blobs_span():
    lab = C.box_many()
    ids, boxes = G.roi_boxes(lab)
    assert ids == list(range(1, 128)) and boxes.shape == (127, 4)
    first = [int(torch.nonzero(lab.reshape(-1) == mid)[0]) for mid in ids]
    assert first != sorted(first), "ascending id order is not the raster order"
    assert sum(int((lab == mid).sum()) == 1 for mid in ids) >= 25
    blobs = C.box_blobs()
    x0, y0, x1, y1 = _tight(blobs, 6)
    assert int((blobs == 6).sum()) < (x1 - x0 + 1) * (y1 - y0 + 1) // 10, "two blobs far apart, one box"
    assert set(C.box_cases()) == {"padding", "clamp", "whole_frame", "thin", "frame_1xN", "frame_Nx1", "many", "blobs"}


# ---- crops -----------------------------------------------------------------------------------------------------------
def test_sweep_covers_every_extent_and_values_differ_everywhere():
    boxes = C.sweep_boxes(41)
    sizes = {(y1 - y0 + 1, x1 - x0 + 1) for x0, y0, x1, y1 in boxes.tolist()}
    assert sizes == {(h, w) for h in range(1, 41) for w in range(1, 41)}
    assert boxes[:, :2].min() == 0 and boxes[:, 2].max() == C.SWEEP_W - 1 and boxes[:, 3].max() == C.SWEEP_H - 1
    img = C.ramp_noise(3, C.SWEEP_H, C.SWEEP_W, 42)
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1), (0, 2), (2, 0)):      # a shifted or transposed tap reads another value
        a = img[:, dy:, max(dx, 0):img.shape[2] + min(dx, 0)]
        b = img[:, :img.shape[1] - dy, max(-dx, 0):img.shape[2] - max(dx, 0)]
        assert bool((a != b).all()), (dy, dx)
    assert not torch.equal(img[0], img[1]) and not torch.equal(img[1], img[2])
    lab = C.id_pattern(C.SWEEP_H, C.SWEEP_W)
    assert bool((lab[:, 1:] != lab[:, :-1]).all()) and bool((lab[1:] != lab[:-1]).all()) and bool((lab[1:, 1:] != lab[:-1, :-1]).all())


@pytest.mark.parametrize("S", C.SWEEP_S)
def test_bilinear_bound_holds_for_the_float32_oracle(S):
    """The bound the GPU crops are held to is not met by luck: on a seventh of the sweep the oracle's own float32
    F.interpolate stays inside it, against F.interpolate on the float64 copy (largest ratio over the whole sweep: 0.51)."""
    boxes = C.sweep_boxes(41)[S % 7::7]
    img = C.ramp_noise(3, C.SWEEP_H, C.SWEEP_W, 42)
    want = C.ref_bilinear(img.double(), boxes, S)
    got = torch.stack([F.interpolate(img[None, :, y0:y1 + 1, x0:x1 + 1], size=(S, S), mode="bilinear", align_corners=True)[0]
                       for x0, y0, x1, y1 in boxes.tolist()])
    err = (got.double() - want).abs().amax(dim=(1, 2, 3)).numpy()
    assert (err <= C.bilinear_bound(img, boxes)).all()


def test_float32_nearest_indices_are_the_exact_ones():
    """F.interpolate(nearest) computes floor(dst * in / out) in float32; for every pair of sizes of the two sweeps (crop:
    1..40 -> S, paste: S -> 1..40) that is the index exact arithmetic gives, so the reference of the mask crops and of the
    paste does not hang on a float32 rounding."""
    pairs = [(n, S) for n in range(1, C.SWEEP_EXTENT + 1) for S in C.SWEEP_S]
    for n_in, n_out in pairs + [(S, n) for n, S in pairs]:
        got = F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None, None, :], size=(1, n_out), mode="nearest")[0, 0, 0]
        assert got.tolist() == [min(d * n_in // n_out, n_in - 1) for d in range(n_out)], (n_in, n_out)


def test_poisoned_windows_are_clean_inside():
    rgb, depth, lab, boxes = C.poisoned_windows()
    sizes = [(y1 - y0 + 1, x1 - x0 + 1) for x0, y0, x1, y1 in boxes.tolist()]
    assert (1, 1) in sizes and any(h == 1 and w > 1 for h, w in sizes) and any(w == 1 and h > 1 for h, w in sizes)
    inside = torch.zeros(lab.shape, dtype=torch.bool)
    for x0, y0, x1, y1 in boxes.tolist():
        inside[y0:y1 + 1, x0:x1 + 1] = True
    for t in (rgb, depth):
        assert not torch.isnan(t[:, inside]).any() and torch.isnan(t[:, ~inside]).all()
    assert torch.isfinite(C.ref_bilinear(rgb.double(), boxes, 7)).all()


# ---- paste-back ------------------------------------------------------------------------------------------------------
def test_paste_sweep_frames_are_disjoint_and_complete():
    frames = C.paste_sweep_frames()
    sizes = []
    for boxes in frames:
        cover = torch.zeros(64, 72, dtype=torch.int32)
        assert 1 <= len(boxes) <= 127
        for x0, y0, x1, y1 in boxes.tolist():
            assert 0 <= x0 <= x1 < 72 and 0 <= y0 <= y1 < 64
            cover[y0:y1 + 1, x0:x1 + 1] += 1
            sizes.append((y1 - y0 + 1, x1 - x0 + 1))
        assert int(cover.max()) == 1
    assert sorted(sizes) == [(h, w) for h in range(1, 41) for w in range(1, 41)]
    lab = C.paste_labels(3, 16)
    assert bool((lab[:, :, 1:] != lab[:, :, :-1]).all()) and bool((lab[:, 1:] != lab[:, :-1]).all())
    assert 0 <= float(lab.min()) and float(lab.max()) == 126


@pytest.mark.parametrize("S", C.SWEEP_S)
def test_vectorised_paste_reference_is_the_oracle(S):
    """tests.glue_cases.match_all_kept_no_depth against oracle.match_label_crop itself, on every twentieth frame of the
    sweep (first and last included: the 40x40 box and the 1-pixel ones)."""
    frames = C.paste_sweep_frames()
    for boxes in frames[::20] + [frames[-1]]:
        K = len(boxes)
        labels = C.paste_labels(K, S)
        rois = torch.from_numpy(boxes).float()
        want, labels_out = G.match_label_crop(torch.zeros(1, 64, 72), labels, torch.ones(K, S, S), rois, None)
        assert torch.equal(labels_out, labels), "nothing is rejected"
        assert torch.equal(C.match_all_kept_no_depth(labels, rois, 64, 72), want[0])


# ---- matching --------------------------------------------------------------------------------------------------------
def _assert_means_are_exact(labels_crop, mask, depth):
    """float32 mean == float64 mean, cast: the sort keys are defined by the inputs, not by a summation order."""
    keep, meanz, out = C.oracle_keep_meanz(labels_crop, mask, depth)
    for i in range(labels_crop.shape[0]):
        kept = out[i] > -1
        z = depth[i, 2][kept] if kept.any() else depth[i, 2]
        z = z[z > 0]
        sel = depth[i, 2][depth[i, 2] > 0]
        assert bool(((sel * 8) % 1 == 0).all()) and (len(sel) == 0 or (0.5 <= float(sel.min()) and float(sel.max()) < 4))
        m64 = torch.mean(z.double()).float()
        assert torch.equal(meanz[i:i + 1], m64[None]) or (torch.isnan(meanz[i]) and torch.isnan(m64))
    return keep, meanz, out


def test_overlap_case_sits_on_one_half():
    c = C.overlap_case()
    assert c["labels_crop"].shape[-1] <= 16
    for i, clusters in enumerate(C.OVERLAP_CLUSTERS):
        for mid, n, inside in clusters:
            sel = c["labels_crop"][i] == mid
            assert (int(sel.sum()), int(c["mask"][i][sel].sum())) == (n, inside)
    fr = {mid: (inside, n) for mid, n, inside in C.OVERLAP_CLUSTERS[0]}
    assert fr[0] == (4, 8) and fr[127] == (50, 100), "exactly 0.5, for id 0 and for id 127"
    assert fr[5] == (3, 8) and fr[64] == (50, 101), "the nearest fractions below"
    keep, meanz, out = _assert_means_are_exact(c["labels_crop"], c["mask"], c["depth"])
    refined, labels_out = G.match_label_crop(c["initial_masks"], c["labels_crop"], c["mask"], c["rois"], c["depth"])
    assert torch.equal(labels_out, out)
    for i in range(2):
        assert set(labels_out[i][labels_out[i] > -1].tolist()) == C.OVERLAP_KEPT[i]
        assert set(torch.nonzero(keep[i]).reshape(-1).tolist()) == C.OVERLAP_KEPT[i]
    assert bool((labels_out[1] == -1).all()), "ROI 1: every cluster is dropped"
    assert set(torch.unique(refined).tolist()) == {0.0, 1.0, 2.0, 3.0}, "id 0 is kept and renumbered; ROI 1 paints nothing"
    everything = torch.mean(c["depth"][1, 2])
    assert torch.equal(meanz[1], everything) and not torch.isnan(everything), "its mean depth is over all its pixels"


@pytest.mark.parametrize("perm", C.ORDER_PERMS)
def test_order_case_keys_tie_and_are_nan(perm):
    c = C.order_case(perm)
    roles = c["roles"]
    at = {r: roles.index(r) for r in roles}
    keep, meanz, out = _assert_means_are_exact(c["labels_crop"], c["mask"], c["depth"])
    assert meanz[at["near"]] == 1.0 and meanz[at["far"]] == 3.0
    a, b = meanz[at["tie_a"]], meanz[at["tie_b"]]
    assert a.view(torch.int32) == b.view(torch.int32), "bit-equal keys"
    assert not torch.equal(c["depth"][at["tie_a"], 2], c["depth"][at["tie_b"], 2])
    assert torch.isnan(meanz[at["nan"]]) and len(roles) < 64
    assert int(keep[at["nan"]].sum()) == 1 and not bool((c["depth"][at["nan"], 2] > 0).any())
    box = {r: [int(v) for v in c["rois"][at[r]].tolist()] for r in roles}
    area = lambda r: (box[r][2] - box[r][0] + 1) * (box[r][3] - box[r][1] + 1)
    assert area("tie_a") == area("tie_b") and len({area(r) for r in roles}) == 4, "no depth: equal and unequal areas"
    overlap = lambda p, q: box[p][0] <= box[q][2] and box[q][0] <= box[p][2] and box[p][1] <= box[q][3] and box[q][1] <= box[p][3]
    assert overlap("near", "far") and overlap("tie_a", "tie_b") and overlap("nan", "far")
    refined, labels_out = G.match_label_crop(c["initial_masks"], c["labels_crop"], c["mask"], c["rois"], c["depth"])
    assert torch.equal(labels_out, out)
    # which relabelled ids belong to which ROI: paint each one alone
    if perm == (0, 1, 2, 3, 4):
        alone = lambda r: G.match_label_crop(c["initial_masks"], c["labels_crop"][at[r]][None], c["mask"][at[r]][None],
                                             c["rois"][at[r]][None], c["depth"][at[r]][None])[0][0] != 0
        near, far = alone("near"), alone("far")
        nx0, ny0, nx1, ny1 = box["near"]
        both = near & far
        assert both.any(), "near's kept half lies over far"
        dropped = torch.zeros_like(near)
        dropped[ny0:ny1 + 1, nx0:nx1 + 1] = True
        dropped &= ~near & far
        others = torch.zeros_like(near)                    # the boxes of the three ROIs this is not about
        for r in ("tie_a", "tie_b", "nan"):
            others[box[r][1]:box[r][3] + 1, box[r][0]:box[r][2] + 1] = True
        dropped &= ~others
        assert dropped.any(), "near's dropped half lies over far"
        far_only = far & ~others
        far_only[ny0:ny1 + 1, nx0:nx1 + 1] = False
        # ids are handed out in paint order: far (3 clusters) is painted before near although it comes second in the list
        far_ids, near_ids = set(refined[0][far_only].tolist()), set(refined[0][near].tolist())
        assert len(near_ids) == 1 and max(far_ids) < min(near_ids)
        assert set(refined[0][both].tolist()) == near_ids, "the nearer ROI overwrites the farther one"
        assert set(refined[0][dropped].tolist()) <= far_ids, "a dropped cluster does not overwrite"


@pytest.mark.parametrize("K", [1, 2, 127])
def test_stats_case_means_are_exact(K):
    labels, mask, depth = C.stats_case(K)
    keep, meanz, out = _assert_means_are_exact(labels, mask, depth)
    assert keep.shape == (K, 128) and int(keep[:, 4:].sum()) == 0
    if K == 127:
        assert torch.isnan(meanz).sum() >= 127 // 7 and 0 < int(keep[:, :4].sum()) < 4 * K
        _, labels_out = G.match_label_crop(torch.zeros(1, 8, 8), labels, mask, torch.zeros(K, 4), depth)
        assert torch.equal(labels_out, out), "keep is the oracle's own rejection"


def test_match_raw_abi_ids_would_alias_kept_clusters():
    c, raw, clean = C.match_raw_abi()
    foreign = clean == -1
    assert set(raw[foreign].tolist()) == set(C.INVALID_IDS) and torch.equal(raw[~foreign].float(), c["labels_crop"][~foreign])
    assert all(bool(foreign[k].any()) and not bool(foreign[k].all()) for k in range(raw.shape[0]))
    aliased = raw.float()
    aliased[foreign] = torch.remainder(raw[foreign], 128).float()
    want = G.match_label_crop(c["initial_masks"], clean, c["mask"], c["rois"], c["depth"])
    wrong = G.match_label_crop(c["initial_masks"], aliased, c["mask"], c["rois"], c["depth"])
    assert not torch.equal(want[0], wrong[0]), "ids taken modulo 128 would change the refined map"
    assert bool((want[1][foreign] == -1).all())
    keep, meanz, out = C.oracle_keep_meanz(clean, c["mask"], c["depth"])
    assert torch.equal(out, want[1])
