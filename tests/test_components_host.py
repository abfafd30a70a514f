"""Connected components of label maps, the part that needs no GPU: the reference (tests/components_reference.py) against
scipy.ndimage.label and against a naive flood fill, the generated maps really containing what the GPU tests use them
for, and the argument validation of uoc_cc_split, which happens before any device work."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import components_reference as R
from unseenobjectclustering_amd import _native, components

SIZES = [(480, 640), (224, 224), (37, 53)]
TILE = 32                        # the tile edge of the first kernel (csrc/components.hip)


def same_partition(a, b):
    """Two label maps (background: values < 0 resp. == 0 handled by the caller) describe the same partition."""
    pairs = np.unique(np.stack([a.ravel(), b.ravel()]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SIZES)
def test_reference_agrees_with_scipy(H, W, connectivity):
    structure = ndimage.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), dtype=bool)
    for img in R.tabletop(1, H, W, frames=2):
        root_map, comps = R.components(img, connectivity)
        F = R.foreground(img)
        assert np.array_equal(root_map >= 0, F > 0)
        area_of = {root: area for root, area, _ in comps}
        total = 0
        for i in np.unique(F[F > 0]).tolist():
            lab, n = ndimage.label(F == i, structure=structure)
            total += n
            m = lab > 0
            assert same_partition(lab[m], root_map[m])
            sizes = ndimage.sum_labels(np.ones_like(lab), lab, index=np.arange(1, n + 1)).astype(np.int64)
            first = ndimage.minimum(np.arange(H * W).reshape(H, W), lab, index=np.arange(1, n + 1)).astype(np.int64)
            for root, size in zip(first.tolist(), sizes.tolist()):
                assert area_of[root] == size                      # the root is the smallest raster index
            assert all(src == i for root, _, src in comps if root in set(first.tolist()))
        assert total == len(comps)


def flood_fill(img, connectivity):
    F = R.foreground(img)
    H, W = F.shape
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    root_map = np.full((H, W), -1, dtype=np.int64)
    for y0, x0 in itertools.product(range(H), range(W)):          # raster order: the seed is the smallest index
        if not F[y0, x0] or root_map[y0, x0] >= 0:
            continue
        root_map[y0, x0] = y0 * W + x0
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and F[v, u] == F[y0, x0] and root_map[v, u] < 0:
                    root_map[v, u] = y0 * W + x0
                    stack.append((v, u))
    return root_map


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_agrees_with_flood_fill(connectivity):
    rng = np.random.default_rng(5)
    for _ in range(200):
        img = rng.choice(np.array([0, 1, 1, 2, 127, 128, -1]), size=(9, 11))
        assert np.array_equal(R.components(img, connectivity)[0], flood_fill(img, connectivity))
    for bits in range(1 << 12):                                   # every binary 3x4 map: the corner cases of diagonal joins
        img = np.array([(bits >> k) & 1 for k in range(12)]).reshape(3, 4) * 7
        root_map, comps = R.components(img, connectivity)
        assert np.array_equal(root_map, flood_fill(img, connectivity))
        assert sum(a for _, a, _ in comps) == bin(bits).count("1")


def test_split_semantics_on_a_small_map():
    img = np.array([[5, 5, 0, 5, 0, 9],
                    [0, 0, 0, 5, 0, 9],
                    [5, 0, 200, 0, 5, 0],
                    [5, 5, 0, -3, 5, 5]])
    out, table, counts = R.split(img, 4, 1, "all")
    assert out.tolist() == [[1, 1, 0, 2, 0, 3], [0, 0, 0, 2, 0, 3], [4, 0, 0, 0, 5, 0], [4, 4, 0, 0, 5, 5]]
    assert table[1:6].tolist() == [[5, 2, 0, 4], [5, 2, 3, 4], [9, 2, 5, 1], [5, 3, 12, 4], [5, 3, 16, 4]]
    assert counts.tolist() == [5, 0, 5, 0] and not table[6:].any() and not table[0].any()
    out, table, counts = R.split(img, 4, 3, "largest")
    assert out.tolist() == [[0] * 6, [0] * 6, [5, 0, 0, 0, 0, 0], [5, 5, 0, 0, 0, 0]]       # the tie goes to the smaller root
    assert table[5].tolist() == [5, 3, 12, 4] and counts.tolist() == [5, 3, 1, 1]
    out8, _, counts8 = R.split(img, 8, 1, "all")
    assert counts8.tolist() == [4, 0, 4, 0]                       # (2,4) joins (1,3) diagonally


def test_generated_maps_contain_what_they_are_for():
    for H, W in SIZES:
        frames = R.tabletop(1, H, W, frames=2)
        assert set(np.unique(frames).tolist()) >= {-1, 0, 128, 255}                   # ids outside 1..127
        for img in frames:
            root_map, comps = R.components(img, 8)
            m = root_map >= 0
            right = m[:, 1:] & (root_map[:, 1:] == root_map[:, :-1])
            down = m[1:, :] & (root_map[1:, :] == root_map[:-1, :])
            assert right[:, TILE - 1::TILE].any() and down[TILE - 1::TILE, :].any()      # components cross tile borders both ways
            sides = [set(s[s >= 0].tolist()) for s in (root_map[0], root_map[-1], root_map[:, 0], root_map[:, -1])]
            assert set.intersection(*sides)                                              # an object touching all four borders
            per_id = {}
            for _, area, src in comps:
                per_id.setdefault(src, []).append(area)
            assert any(sum(a >= 20 for a in v) >= 2 for v in per_id.values())            # two disjoint blobs sharing an id
            assert any(a < 20 for _, a, _ in comps)                                      # speckle
    _, _, counts = R.split(R.tabletop(1, 480, 640)[0], 8, 1, "all")
    assert counts[2] == 127 and counts[3] > 0                                            # more than 127 non-small components
    for H, W in ((37, 53), (224, 224)):
        _, _, counts = R.split(R.checkerboard(H, W), 4, 1, "all")
        assert counts[2] == 127 and counts[3] == counts[0] - 127
        assert R.split(R.checkerboard(H, W), 8, 1, "all")[2].tolist() == [1, 0, 1, 0]
        for name in ("serpentine", "spiral"):
            for c in (4, 8):
                _, comps = R.components(R.ENGINEERED[name](H, W), c)
                assert len(comps) == 1 and comps[0][0] == 0 and comps[0][1] > H * W // 3
        _, comps = R.components(R.comb_and_u(H, W), 4)
        assert len(comps) == 3 and [c[2] for c in comps] == [11, 13, 12]
        _, comps = R.components(R.stripes(H, W), 8)
        assert len(comps) == W
        d4, d8 = R.components(R.diagonals(H, W), 4)[1], R.components(R.diagonals(H, W), 8)[1]
        assert all(a == 1 for _, a, _ in d4) and len(d8) < len(d4) // 10
        edges = [a for _, a, _ in R.components(R.area_edges(H, W), 8)[1]]
        assert sorted(edges) == [1, 2, 36, 36, 49, 50, 50]                               # area == min_area and min_area - 1 at 2 and 50; a tie
        _, table, counts = R.split(R.area_edges(H, W), 8, 50, "largest")
        assert counts.tolist() == [7, 5, 2, 0] and table[41].tolist() == [41, 50, W + 1, 2]
        _, table, _ = R.split(R.area_edges(H, W), 8, 2, "largest")
        assert table[42].tolist() == [42, 36, 10 * W + 1, 2]                             # the tie: the smaller root
    assert R.split(R.checkerboard(37, 53), 4, 1, "all")[2].tolist() == [980, 0, 127, 853]


def test_abi_validation_without_gpu():
    """Every refusal of uoc_cc_split comes through the error channel before any HIP call; the pointers are never read."""
    lib = _native.lib()
    assert lib.uoc_cc_workspace_bytes(1, 0, 5) == 0 and lib.uoc_cc_workspace_bytes(0, 4, 4) == 0
    assert lib.uoc_cc_workspace_bytes(1, 1 << 16, 1 << 15) == 0                     # H*W = 2^31
    one = lib.uoc_cc_workspace_bytes(1, 480, 640)
    assert one >= 2 * 480 * 640 * 4
    assert lib.uoc_cc_workspace_bytes(12, 480, 640) == 12 * one > lib.uoc_cc_workspace_bytes(2, 480, 640) > one
    P = ctypes.c_void_p
    lab, out, table, counts, ws = P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000)
    big = one

    def call(labels=lab, o=out, t=table, c=counts, w=ws, conn=8, min_area=1, mode=0, nbytes=big, shape=(1, 480, 640)):
        return lib.uoc_cc_split(labels, *shape, conn, min_area, mode, o, t, c, w, nbytes, None)

    for kw in (dict(labels=None), dict(o=None), dict(t=None), dict(c=None), dict(w=None)):
        assert call(**kw) == -22
        assert b"null" in lib.uoc_last_error().lower()
    assert call(o=lab) == -22 and b"alias" in lib.uoc_last_error().lower()
    for conn in (0, 1, 6, 9, -4):
        assert call(conn=conn) == -22 and b"connectivity" in lib.uoc_last_error().lower()
    for min_area in (0, -1):
        assert call(min_area=min_area) == -22 and b"min_area" in lib.uoc_last_error().lower()
    for mode in (2, -1):
        assert call(mode=mode) == -22 and b"mode" in lib.uoc_last_error().lower()
    assert call(nbytes=big - 1) == -22 and b"workspace" in lib.uoc_last_error().lower()
    assert call(nbytes=0) == -22
    assert call(shape=(1, 0, 5)) == -22 and call(shape=(0, 4, 4)) == -22
    assert (_native.CC_ALL, _native.CC_LARGEST) == (R.ALL, R.LARGEST) == (0, 1)


def test_split_components_refuses_cpu_tensors():
    with pytest.raises(_native.NativeError):
        components.split_components(torch.zeros(8, 8, dtype=torch.int32))
    with pytest.raises(_native.NativeError):
        components.split_components(np.zeros((8, 8), dtype=np.int32))
