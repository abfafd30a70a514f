"""The five tables of uoc_eval_pair_stats at an explicit radius, from the oracle's own pieces (seg2bmap, disk,
ndimage.binary_dilation): every label's boundary is dilated once, not once per label pair as in
oracle.evaluation_oracle.pair_tables, so radii up to 32 stay cheap.  tests/test_evaluation_cases_host.py proves the two
equal where both are affordable.  Test infrastructure: no torch, no GPU."""
import numpy as np
from scipy import ndimage

from oracle import evaluation_oracle as EO


def square(radius):
    """The wrong structuring element of the same radius: what a kernel without the dx^2 + dy^2 <= r^2 test would use."""
    return np.ones((2 * int(radius) + 1, 2 * int(radius) + 1), dtype=np.uint8)


def radius_of(shape, bound_th):
    """evaluation.py:88-89: a fraction of the diagonal below 1, else pixels."""
    return int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(shape)))


def boundaries(labels):
    """{label: seg2bmap(labels == label)} for the labels present, background excluded."""
    return {int(l): EO.seg2bmap(labels == l) for l in np.unique(labels) if l != 0}


def pair_tables(prediction, gt, radius, structure=None):
    """dict(cont, prec_tp, rec_tp [128,128] indexed [gt, pred]; bnd_pred, bnd_gt [128]), int64."""
    prediction, gt = np.asarray(prediction).astype(np.int64), np.asarray(gt).astype(np.int64)
    assert prediction.shape == gt.shape and prediction.ndim == 2
    assert 0 <= prediction.min() and prediction.max() < 128 and 0 <= gt.min() and gt.max() < 128
    fp = (EO.disk(radius) if structure is None else np.asarray(structure)).astype(bool)
    cont = np.bincount((gt * 128 + prediction).reshape(-1), minlength=128 * 128).reshape(128, 128).astype(np.int64)
    prec_tp, rec_tp = np.zeros((128, 128), np.int64), np.zeros((128, 128), np.int64)
    bnd_pred, bnd_gt = np.zeros(128, np.int64), np.zeros(128, np.int64)
    bp, bg = boundaries(prediction), boundaries(gt)
    dp = {j: ndimage.binary_dilation(b, structure=fp) for j, b in bp.items()}
    dg = {i: ndimage.binary_dilation(b, structure=fp) for i, b in bg.items()}
    for j, b in bp.items():
        bnd_pred[j] = b.sum()
    for i, b in bg.items():
        bnd_gt[i] = b.sum()
        for j in bp:
            prec_tp[i, j] = np.logical_and(bp[j], dg[i]).sum()
            rec_tp[i, j] = np.logical_and(b, dp[j]).sum()
    return dict(cont=cont, prec_tp=prec_tp, rec_tp=rec_tp, bnd_pred=bnd_pred, bnd_gt=bnd_gt)
