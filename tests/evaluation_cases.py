"""Engineered (prediction, ground truth, bound_th) triples for the evaluation kernels (csrc/eval.hip): labels on both
sides of 64, 2x2 neighbourhoods of four distinct labels, radii 0 to 32 (where a disk is not a square, and larger than the
image), maps of one row, one column and one pixel, and thousands of pixels adding into the same few table cells.
tests/test_evaluation_cases_host.py proves on the CPU that each case contains what it is for.  No torch, no GPU."""
import numpy as np

HIGH_IDS = (1, 2, 31, 32, 62, 63, 64, 65, 95, 96, 126, 127)
CORNER_IDS = np.array([[1, 64], [127, 63]], dtype=np.int64)


def tiled(H, W, th, tw, ids, start=0):
    """Tiles of th x tw pixels numbered along the rows, tile k labelled ids[(start + k) % len(ids)]."""
    ys, xs = np.mgrid[0:H, 0:W]
    k = (ys // th) * -(-W // tw) + xs // tw
    return np.asarray(ids, dtype=np.int64)[(start + k) % len(ids)]


def high_labels(bound_th=0.003):
    """40x56: the ground truth in 10x14 tiles, the prediction in 8x8 tiles of the same twelve ids, shifted by (1, 2)."""
    gt = tiled(40, 56, 10, 14, HIGH_IDS)
    pred = np.roll(np.roll(tiled(40, 56, 8, 8, HIGH_IDS, start=5), 1, axis=0), 2, axis=1)
    return pred, gt, bound_th


def four_corner():
    """6x10 of the 2x2 block (1, 64 / 127, 63): every 2x2 neighbourhood holds four distinct labels, below and from 64 up.
    The prediction is the same pattern one pixel to the right, with a background hole."""
    gt = np.tile(CORNER_IDS, (3, 5))
    pred = np.roll(gt, 1, axis=1)
    pred[2:4, 3:6] = 0
    return pred, gt, 0.003


def four_corner_bare():
    """The bare 2x2 map: one pixel with a full neighbourhood, the last row, the last column, the corner."""
    return CORNER_IDS[::-1].copy(), CORNER_IDS.copy(), 0.003


RADII = (0, 1, 4, 5, 32)


def radius(bound_th):
    """24x40, one side shorter than 32: objects in the corners and the middle, so that boundary pixels of the two maps lie at
    offsets inside the square of every radius but outside its disk.  bound_th >= 1 is pixels; 0 is no dilation."""
    assert bound_th in RADII
    gt = np.zeros((24, 40), dtype=np.int64)
    gt[0:5, 0:6] = 3
    gt[17:24, 31:40] = 70
    gt[8:15, 14:24] = 5
    pred = np.zeros((24, 40), dtype=np.int64)
    pred[3:9, 4:11] = 3
    pred[14:20, 27:36] = 100
    pred[9:15, 17:27] = 5
    pred[20:24, 0:4] = 64
    return pred, gt, bound_th


def tiny_1x1():
    return np.array([[5]], dtype=np.int64), np.array([[5]], dtype=np.int64), 0.003


def tiny_1x7():
    """One row: only the east rule; a label in the last column."""
    return np.array([[0, 1, 1, 64, 64, 0, 127]], dtype=np.int64), np.array([[1, 1, 0, 64, 127, 127, 127]], dtype=np.int64), 1


def tiny_7x1():
    """One column: only the south rule; a label in the last row."""
    p, g, _ = tiny_1x7()
    return p.T.copy(), g.T.copy(), 1


def tiny_2x2():
    """Labels in the last row, the last column and the corner only."""
    return np.array([[0, 2], [2, 9]], dtype=np.int64), np.array([[0, 0], [2, 9]], dtype=np.int64), 0.003


def one_cell():
    """64x64 checkerboard of labels 5 and 100 in both maps (the prediction one pixel down, i.e. swapped): every pixel but
    the corner is a boundary pixel of both labels, so 4095 pixels add into the same four cells of each table."""
    ys, xs = np.mgrid[0:64, 0:64]
    gt = np.where((ys + xs) % 2 == 0, 5, 100).astype(np.int64)
    return np.roll(gt, 1, axis=0), gt, 0.003


CASES = {
    "high_labels": high_labels,
    "high_labels_r1": lambda: high_labels(1),
    "high_labels_r4": lambda: high_labels(4),
    "four_corner": four_corner,
    "four_corner_bare": four_corner_bare,
    **{f"radius_{r}": (lambda r=r: radius(r)) for r in RADII},
    "tiny_1x1": tiny_1x1,
    "tiny_1x7": tiny_1x7,
    "tiny_7x1": tiny_7x1,
    "tiny_2x2": tiny_2x2,
    "one_cell": one_cell,
}
