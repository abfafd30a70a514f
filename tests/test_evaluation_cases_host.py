"""The evaluation cases (tests/evaluation_cases.py) and the reference at an explicit radius
(tests/evaluation_reference.py) on the CPU: the reference equals the oracle's brute force over label pairs wherever that
is affordable, and every case contains what it is for.  tests/test_evaluation_gpu.py runs the cases on the device."""
import numpy as np
import pytest

from oracle import evaluation_oracle as EO
from tests import evaluation_cases as EC
from tests import evaluation_reference as ER
from tests.golden.cases import EVAL_CASES, eval_pair

TABLES = ("cont", "bnd_pred", "bnd_gt", "prec_tp", "rec_tp")


def equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in TABLES)


@pytest.mark.parametrize("name", ["permuted", "no_pred", "no_gt", "nothing", "shifted", "merged", "split_extra"])
def test_reference_equals_oracle_on_the_golden_pairs(name):
    assert set(EVAL_CASES) == {"permuted", "no_pred", "no_gt", "nothing", "shifted", "merged", "split_extra"}
    pred, gt = eval_pair(EVAL_CASES[name])
    assert equal(ER.pair_tables(pred, gt, ER.radius_of(pred.shape, 0.003)), EO.pair_tables(pred, gt))


@pytest.mark.parametrize("bound_th", [0.003, 1, 4])
def test_reference_equals_oracle_on_high_labels(bound_th):
    pred, gt, _ = EC.high_labels()
    assert equal(ER.pair_tables(pred, gt, ER.radius_of(pred.shape, bound_th)), EO.pair_tables(pred, gt, bound_th=bound_th))


def test_oracle_default_bound_is_unchanged():
    pred, gt, _ = EC.four_corner()
    assert equal(EO.pair_tables(pred, gt), EO.pair_tables(pred, gt, bound_th=0.003))
    assert ER.radius_of((480, 640), 0.003) == 3 and ER.radius_of((6, 10), 0.003) == 1 and ER.radius_of((6, 10), 32) == 32
    assert ER.radius_of((24, 40), 0) == 0


def test_high_labels_fill_all_four_quadrants():
    pred, gt, th = EC.high_labels()
    assert sorted(np.unique(pred)) == sorted(np.unique(gt)) == list(EC.HIGH_IDS)
    t = ER.pair_tables(pred, gt, ER.radius_of(pred.shape, th))
    lo, hi = slice(1, 64), slice(64, 128)
    for k in ("prec_tp", "rec_tp", "cont"):
        for a in (lo, hi):
            for b in (lo, hi):
                assert t[k][a, b].any(), (k, a, b)
    for k in ("bnd_pred", "bnd_gt"):
        assert t[k][63] > 0 and t[k][64] > 0 and t[k][127] > 0
    assert not equal(t, ER.pair_tables(pred, gt, 4))


def test_four_corner_has_four_distinct_labels_in_one_neighbourhood():
    for make in (EC.four_corner, EC.four_corner_bare):
        pred, gt, _ = make()
        for m in (pred, gt):
            full = [len({m[y, x], m[y, x + 1], m[y + 1, x], m[y + 1, x + 1]} - {0}) == 4
                    for y in range(m.shape[0] - 1) for x in range(m.shape[1] - 1)]
            assert any(full)
            assert (m < 64).any() and (m >= 64).any()
    assert EC.four_corner_bare()[0].shape == (2, 2)


@pytest.mark.parametrize("r", [4, 5, 32])
def test_radius_tables_need_the_disk(r):
    pred, gt, th = EC.radius(r)
    assert th == r and min(pred.shape) < 32 < max(pred.shape)
    disk, sq = ER.pair_tables(pred, gt, r), ER.pair_tables(pred, gt, r, structure=ER.square(r))
    assert not np.array_equal(disk["prec_tp"], sq["prec_tp"]) and not np.array_equal(disk["rec_tp"], sq["rec_tp"])
    assert (disk["prec_tp"] <= sq["prec_tp"]).all() and (disk["rec_tp"] <= sq["rec_tp"]).all()


def test_radius_tables_grow_with_the_radius_and_32_is_not_everything():
    runs = [ER.pair_tables(*EC.radius(r)[:2], r) for r in EC.RADII]
    for a, b in zip(runs, runs[1:]):
        assert (a["prec_tp"] <= b["prec_tp"]).all() and a["prec_tp"].sum() < b["prec_tp"].sum()
        assert (a["rec_tp"] <= b["rec_tp"]).all() and a["rec_tp"].sum() < b["rec_tp"].sum()
    pred, gt, _ = EC.radius(32)
    everything = ER.pair_tables(pred, gt, 64)                # radius 32 is larger than the short side, but not the whole image
    assert runs[-1]["prec_tp"].sum() < everything["prec_tp"].sum()


def test_radius_0_is_the_plain_intersection():
    pred, gt, th = EC.radius(0)
    t = ER.pair_tables(pred, gt, ER.radius_of(pred.shape, th))
    bp, bg = ER.boundaries(pred), ER.boundaries(gt)
    want = np.zeros((128, 128), np.int64)
    for i, g in bg.items():
        for j, p in bp.items():
            want[i, j] = (g & p).sum()
    assert want.any() and np.array_equal(t["prec_tp"], want) and np.array_equal(t["rec_tp"], want)
    assert equal(t, EO.pair_tables(pred, gt, bound_th=0))


def test_tiny_maps_exercise_the_last_row_column_and_corner():
    shapes = {name: EC.CASES[name]()[0].shape for name in ("tiny_1x1", "tiny_1x7", "tiny_7x1", "tiny_2x2")}
    assert shapes == dict(tiny_1x1=(1, 1), tiny_1x7=(1, 7), tiny_7x1=(7, 1), tiny_2x2=(2, 2))
    for name in shapes:
        pred, gt, th = EC.CASES[name]()
        assert pred[-1, -1] != 0 and gt[-1, -1] != 0                                      # a label in the corner ...
        t = ER.pair_tables(pred, gt, ER.radius_of(pred.shape, th))
        assert equal(t, EO.pair_tables(pred, gt, bound_th=th))
        for m, k in ((pred, "bnd_pred"), (gt, "bnd_gt")):                                 # ... which is never a boundary
            assert all(not EO.seg2bmap(m == l)[-1, -1] for l in np.unique(m))
    t = ER.pair_tables(*EC.tiny_1x1()[:2], 1)
    assert t["cont"][5, 5] == 1 and not t["bnd_pred"].any() and not t["prec_tp"].any()
    pred, gt, _ = EC.tiny_1x7()
    t = ER.pair_tables(pred, gt, 1)
    assert t["bnd_pred"][[1, 64, 127]].tolist() == [2, 2, 1] and t["bnd_gt"][[1, 64, 127]].tolist() == [1, 2, 1]
    assert equal({k: (v.T if v.ndim == 2 else v) for k, v in t.items()},
                 {k: (v.T if v.ndim == 2 else v) for k, v in ER.pair_tables(*EC.tiny_7x1()[:2], 1).items()})
    pred, gt, _ = EC.tiny_2x2()
    t = ER.pair_tables(pred, gt, 1)
    assert t["bnd_pred"][[2, 9]].tolist() == [3, 3] and t["bnd_gt"][[2, 9]].tolist() == [2, 3]     # by hand from seg2bmap's rules


def test_one_cell_piles_every_pixel_into_four_cells():
    pred, gt, th = EC.one_cell()
    t = ER.pair_tables(pred, gt, ER.radius_of(pred.shape, th))
    assert t["bnd_pred"][[5, 100]].tolist() == [4095, 4095] and t["bnd_gt"][[5, 100]].tolist() == [4095, 4095]
    for k in ("prec_tp", "rec_tp"):
        assert np.count_nonzero(t[k]) == 4 and (t[k][np.ix_([5, 100], [5, 100])] == 4095).all()
    assert np.count_nonzero(t["cont"]) == 2 and t["cont"][5, 100] == t["cont"][100, 5] == 2048


def test_every_case_is_a_valid_input():
    for name, make in EC.CASES.items():
        pred, gt, th = make()
        assert pred.shape == gt.shape and pred.dtype == gt.dtype == np.int64, name
        assert 0 <= min(pred.min(), gt.min()) and max(pred.max(), gt.max()) < 128, name
        assert 0 <= ER.radius_of(pred.shape, th) <= 32 and max(pred.shape) <= 64, name
