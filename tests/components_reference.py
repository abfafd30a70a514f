"""The semantics of uoc_cc_split (include/uoc_hip.h) in plain numpy and Python integers — the reference of the GPU tests.

Input L [H,W] of integers.  A pixel is foreground when 1 <= L <= 127; everything else (negative ids, 128, 255) is
background.  connectivity is 4 or 8.  A component is a maximal set of foreground pixels that carry the same id and are
connected through neighbours of that id; different ids never join.  root = the component's smallest raster index
y*W + x, area = its pixel count, src = its raw id, siblings(i) = the number of components of raw id i (small ones
included).  A component is small when area < min_area (min_area >= 1); small components become background.

Mode ALL (0): the non-small components in ascending root order get the new ids 1..127; those beyond the 127th become
background and count as dropped; table[k] = (src, area, root, siblings(src)) for new id k.
Mode LARGEST (1): per raw id the non-small component of largest area (ties: the smaller root) keeps the raw id, the
id's other non-small components become background and count as dropped; table[i] = (i, area, root, siblings(i)).
Unused rows and row 0 are zero.  counts = (found, small, kept, dropped), found == small + kept + dropped.

The method: row runs, then union-find over the runs (a one-pixel-wide path of 10^5 pixels costs nothing special).  No
scipy here, so that the comparison with scipy.ndimage.label in test_components_host.py is independent."""
import numpy as np

ALL, LARGEST = 0, 1
MODES = {"all": ALL, "largest": LARGEST}


def foreground(L):
    L = np.asarray(L).astype(np.int64)
    return np.where((L >= 1) & (L <= 127), L, 0)


def components(L, connectivity):
    """(root_map [H,W] int64 with -1 on the background, list of (root, area, src) in ascending root order)."""
    assert connectivity in (4, 8)
    F = foreground(L)
    H, W = F.shape
    runs = []                      # (y, x0, x1 exclusive, id)
    rows = [[] for _ in range(H)]  # run indices of each row
    for y in range(H):
        row = F[y]
        edges = np.flatnonzero(np.diff(row)) + 1
        starts = np.concatenate(([0], edges))
        ends = np.concatenate((edges, [W]))
        for x0, x1 in zip(starts.tolist(), ends.tolist()):
            c = int(row[x0])
            if c:
                rows[y].append(len(runs))
                runs.append((y, x0, x1, c))
    parent = list(range(len(runs)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    reach = 1 if connectivity == 8 else 0
    for y in range(1, H):
        up = rows[y - 1]
        j = 0
        for r in rows[y]:
            _, x0, x1, c = runs[r]
            while j < len(up) and runs[up[j]][2] + reach <= x0:      # runs ending left of the reach never matter again
                j += 1
            k = j
            while k < len(up) and runs[up[k]][1] < x1 + reach:
                if runs[up[k]][3] == c and runs[up[k]][2] + reach > x0:
                    a, b = find(r), find(up[k])
                    if a != b:
                        parent[max(a, b)] = min(a, b)                # runs are in raster order: the smaller index starts first
                k += 1
    root_map = np.full((H, W), -1, dtype=np.int64)
    info = {}
    for r, (y, x0, x1, c) in enumerate(runs):
        head = find(r)
        hy, hx0 = runs[head][0], runs[head][1]
        root = hy * W + hx0
        root_map[y, x0:x1] = root
        rec = info.setdefault(root, [root, 0, c])
        rec[1] += x1 - x0
    comps = [tuple(info[k]) for k in sorted(info)]
    return root_map, comps


def split(L, connectivity=8, min_area=1, mode=ALL):
    """(out [H,W] int32, table [128,4] int32, counts [4] int32) of one frame."""
    mode = MODES.get(mode, mode)
    assert mode in (ALL, LARGEST) and min_area >= 1
    root_map, comps = components(L, connectivity)
    siblings = [0] * 128
    for _, _, src in comps:
        siblings[src] += 1
    big = [c for c in comps if c[1] >= min_area]
    table = np.zeros((128, 4), dtype=np.int32)
    new_of_root = {}
    if mode == ALL:
        for k, (root, area, src) in enumerate(big[:127], start=1):
            new_of_root[root] = k
            table[k] = (src, area, root, siblings[src])
    else:
        best = {}
        for root, area, src in big:                                   # ascending root: a later one must be strictly larger
            if src not in best or area > best[src][1]:
                best[src] = (root, area)
        for src, (root, area) in best.items():
            new_of_root[root] = src
            table[src] = (src, area, root, siblings[src])
    out = np.zeros(root_map.shape, dtype=np.int32)
    if new_of_root:
        roots = np.array(sorted(new_of_root), dtype=np.int64)
        ids = np.array([new_of_root[r] for r in roots.tolist()], dtype=np.int32)
        pos = np.searchsorted(roots, root_map)
        pos_c = np.minimum(pos, len(roots) - 1)
        hit = roots[pos_c] == root_map
        out = np.where(hit, ids[pos_c], 0).astype(np.int32)
    found, small, kept = len(comps), len(comps) - len(big), len(new_of_root)
    counts = np.array([found, small, kept, len(big) - kept], dtype=np.int32)
    return out, table, counts


def split_batch(L, connectivity=8, min_area=1, mode=ALL):
    """[B,H,W] -> (out [B,H,W], table [B,128,4], counts [B,4])."""
    res = [split(f, connectivity, min_area, mode) for f in np.asarray(L)]
    return tuple(np.stack([r[k] for r in res]) for k in range(3))


# ---- the maps of the tests (seeded; shared by the host and the GPU file) ---------------------------------------------------

def tabletop(seed, H, W, frames=1):
    """[frames,H,W] int32: ellipses with ids redrawn per frame, two disjoint blobs sharing an id, an object touching all
    four image borders, 0.2 % speckle carrying object ids, and ids from {0, -1, 128, 255} sprinkled in as background."""
    rng = np.random.default_rng(7000 * seed + 13 * H + W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    S = float(min(H, W))
    out = np.zeros((frames, H, W), dtype=np.int32)
    for t in range(frames):
        img = out[t]
        n = int(rng.integers(5, 9))
        ids = rng.choice(np.arange(1, 128), size=n + 2, replace=False)
        for k in range(n):
            a, b = rng.uniform(S / 12, S / 4), rng.uniform(S / 12, S / 4)
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            img[((xs - cx) / a) ** 2 + ((ys - cy) / b) ** 2 <= 1.0] = ids[k]
        twin = int(ids[n + 1])                                            # the same id at two places
        r = max(1.5, S / 16)
        for cx, cy in ((0.2 * W, 0.25 * H), (0.8 * W, 0.75 * H)):
            img[(np.abs(xs - cx) <= r) & (np.abs(ys - cy) <= r)] = twin
        speck = rng.random((H, W)) < 0.002
        img[speck] = rng.choice(ids, size=int(speck.sum()))
        junk = rng.random((H, W)) < 0.01
        img[junk] = rng.choice(np.array([0, -1, 128, 255], dtype=np.int32), size=int(junk.sum()))
        if min(H, W) >= 8:                                               # an unbroken ring along all four borders, drawn last
            img[0, :] = img[H - 1, :] = ids[n]
            img[:, 0] = img[:, W - 1] = ids[n]
    return out


def serpentine(H, W):
    """A one-pixel-wide path over every second row, joined alternately at the right and the left end: one component."""
    img = np.zeros((H, W), dtype=np.int32)
    img[0::2, :] = 5
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            img[y, W - 1 if k % 2 == 0 else 0] = 5
    return img


def spiral(H, W):
    """A one-pixel-wide rectangular spiral with one-pixel gaps between its turns, walked from the top-left corner inwards."""
    img = np.zeros((H, W), dtype=np.int32)
    y, x, dy, dx = 0, 0, 0, 1
    img[0, 0] = 9
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            free = 0 <= ny < H and 0 <= nx < W and img[ny, nx] == 0
            if free and not (0 <= ay < H and 0 <= ax < W and img[ay, ax] != 0):
                break
            dy, dx = dx, -dy                                             # turn right
        else:
            return img
        y, x = ny, nx
        img[y, x] = 9


def checkerboard(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.where((ys + xs) % 2 == 1, 3, 0).astype(np.int32)


def comb_and_u(H, W):
    """Upper half: teeth on the even columns that only join in their last row, so the tops of the teeth look like
    separate components until then (a root found late must still win).  Lower half: a U whose arms meet in the last
    image row, and inside it a comb joined at its top."""
    img = np.zeros((H, W), dtype=np.int32)
    half = H // 2
    img[0:half - 1, 0:W:2] = 11
    img[half - 2, :] = 11
    img[half:H, 0] = 13
    img[half:H, W - 1] = 13
    img[H - 1, :] = 13
    img[half, 2:W - 2] = 12
    img[half:H - 2, 2:W - 2:3] = 12
    return img


def stripes(H, W):
    """Two ids in alternating one-pixel columns: they never join."""
    img = np.zeros((H, W), dtype=np.int32)
    img[:, 0::2] = 21
    img[:, 1::2] = 22
    return img


def diagonals(H, W):
    """Diagonal lines four apart, both directions in the two halves: one component each with connectivity 8, one per
    pixel with connectivity 4."""
    ys, xs = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W), dtype=np.int32)
    left = xs < W // 2
    img[left & ((ys - xs) % 4 == 0)] = 31
    img[~left & ((ys + xs) % 4 == 0)] = 32
    return img


def area_edges(H, W):
    """Areas around the thresholds of the tests (min_area 2 and 50): components of 50, 49, 2 and 1 pixels, and two
    components of one id with the same area (the tie LARGEST settles by the smaller root).  Needs H >= 30, W >= 40."""
    img = np.zeros((H, W), dtype=np.int32)
    img[1:6, 1:11] = 41          # 50
    img[1:8, 14:21] = 41         # 49
    img[10:16, 1:7] = 42         # 36 ...
    img[20:26, 30:36] = 42       # ... and 36 again, later in raster order
    img[10, 20:22] = 43          # 2
    img[12, 20] = 43             # 1
    img[18:28, 2:7] = 44         # 50, alone under its id
    return img


ENGINEERED = {"serpentine": serpentine, "spiral": spiral, "checkerboard": checkerboard, "comb_and_u": comb_and_u,
              "stripes": stripes, "diagonals": diagonals, "area_edges": area_edges}
