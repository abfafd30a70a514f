"""Plain numpy restatement of uoc_support_planes (include/uoc_hip.h): the rounds of sequential plane
extraction, written with tests/support_reference.py's candidates, hypothesis, scores, inlier_mask, refine and object_record
(exact integers for the rounds, float64 for refinement and objects), and the three helpers of support.py with plain loops.
Also the scenes of the GPU tests; tests/test_planes_host.py asserts that they contain what they are used for."""
import math

import numpy as np

from tests import support_reference as R

NUM_IDS = R.NUM_IDS
FRINGE = 16
MAX_PLANES = 8
PLANE_INTS = ("found", "candidates", "inliers", "hyp")


def default_min_inliers(H, W):
    return max(3, H * W // 50)


# ---- the rounds ---------------------------------------------------------------------------------------------------------
def fit(labels, xyz, K, num_hyp, tau_mm, rem_mm, min_inliers, seed, objects=True):
    """One frame: labels [H,W] ints, xyz [3,H,W] float32.  Returns dict(count, planes = K dicts as support_reference.fit's
    `plane` (a slot without a plane has found, candidates, inliers, hyp only), info = K dicts (round_candidates, removed,
    cos0, offset0, extent), index [H,W] int64, objects = K dicts {id: record})."""
    assert 1 <= K <= MAX_PLANES and 1 <= tau_mm <= rem_mm <= 1000 and min_inliers >= 3
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    X = np.asarray(xyz, np.float32).reshape(3, -1)
    idx, q = R.candidates(lab, xyz)
    index = np.full(H * W, -2, np.int64)
    index[idx] = -1
    planes = [dict(found=0, candidates=0, inliers=0, hyp=0) for _ in range(K)]
    info = [dict(round_candidates=0, removed=0, cos0=0.0, offset0=0.0, extent=np.zeros(4)) for _ in range(K)]
    objs = [{} for _ in range(K)]
    valid = R.valid_points(xyz)
    flat = lab.reshape(-1)
    count = 0
    for r in range(K):
        planes[r]["candidates"] = info[r]["round_candidates"] = len(q)
        sd = (seed + r) & 0xFFFFFFFF
        sc = R.scores(q, num_hyp, tau_mm, sd)
        if sc.max() < 0 or sc.max() < min_inliers:           # M_r < 3 gives all -1
            break
        h = int(np.argmax(sc))                               # ties go to the lowest h
        n, p0, thr = R.hypothesis(q, h, tau_mm, sd)
        inl = R.inlier_mask(q, (n, p0, thr))
        rem = R.inlier_mask(q, (n, p0, thr // tau_mm * rem_mm))           # thr = tau_mm * L
        assert int(inl.sum()) == sc[h] and not np.any(inl & ~rem)
        index[idx[inl]] = r
        index[idx[rem & ~inl]] = FRINGE + r
        pts = X[:, idx[inl]].T.astype(np.float64)
        pl = R.refine(pts)
        planes[r].update(found=1, inliers=int(sc[h]), hyp=h, **pl)
        planes[r]["rms"] = math.sqrt(max(pl["eig"][2], 0.0))
        a, b = (pts - pl["centroid"]) @ pl["u"], (pts - pl["centroid"]) @ pl["v"]
        p0l = planes[0]
        info[r].update(removed=int(rem.sum()), cos0=float(pl["normal"] @ p0l["normal"]),
                       offset0=float(p0l["normal"] @ pl["centroid"] + p0l["d"]),
                       extent=np.array([a.min(), a.max(), b.min(), b.max()]))
        if objects:
            for l in range(1, NUM_IDS):
                sel = np.nonzero((flat == l) & valid)[0]
                if len(sel):
                    objs[r][l] = R.object_record(X[:, sel].T.astype(np.float64), pl)
        count += 1
        idx, q = idx[~rem], q[~rem]
    return dict(count=count, planes=planes, info=info, index=index.reshape(H, W), objects=objs)


# ---- the helpers, with plain loops ------------------------------------------------------------------------------------------
def _direction(want, like):
    if isinstance(like, int):
        p = want["planes"][like]
        return np.asarray(p["normal"], np.float64) if p["found"] else None
    v = np.asarray(like, np.float64)
    return v / np.linalg.norm(v)


def like_cosines(want, like):
    """Per found plane the signed cosine with the reference direction (None without one)."""
    ref = _direction(want, like)
    return [None if ref is None else float(np.asarray(want["planes"][k]["normal"]) @ ref) for k in range(want["count"])]


def planes_like(want, like, par_deg=15.0):
    K = len(want["planes"])
    out = [False] * K
    for k, c in enumerate(like_cosines(want, like)):
        out[k] = c is not None and c >= math.cos(math.radians(par_deg))
    return out


def standing_on(want, like=0, tol=0.02, par_deg=15.0):
    cls = planes_like(want, like, par_deg)
    out = [-1] * NUM_IDS
    for l in range(1, NUM_IDS):
        best = None
        for k in range(want["count"]):
            o = want["objects"][k].get(l)
            if o is None or not cls[k] or o["height_min"] < -tol:
                continue
            if best is None or o["height_min"] < best[0]:        # strictly: ties stay with the lowest k
                best = (o["height_min"], k)
        if best is not None:
            out[l] = best[1]
    return out


def choose_support(want, up=None, tol=0.02, par_deg=15.0):
    like = 0 if up is None else up
    cls = planes_like(want, like, par_deg)
    on = standing_on(want, like, tol, par_deg)
    best, votes = 0, -1
    for k in range(len(cls)):
        if cls[k]:
            v = sum(1 for l in range(1, NUM_IDS) if on[l] == k)
            if v > votes:
                best, votes = k, v
    return best


# ---- scenes -------------------------------------------------------------------------------------------------------------------
BOARD_T = 0.25                         # the shelf board, metres above the table
BOARD_A, BOARD_B = (-0.60, 0.02), (0.55, 1.40)      # its in-plane range about the foot of the camera
WALL_T = 0.60                          # the side wall rises this far above the table
TABLE_Z = 2.12                         # the table ends where its depth reaches this; behind it the far patch at R.Z_FAR
MATS = (0.0045, 0.015)                 # unlabelled mats on the table, metres thick
SURFACES = {"far": 0, "table": 1, "board": 2, "wall": 3}


def table_axes():
    n = R.PLANE_N
    u = np.array([1.0, 0.0, 0.0]) - n[0] * n
    u /= np.linalg.norm(u)
    return n, u, np.cross(n, u), -R.PLANE_D * n


def _all_free(free, h, w):
    """[H-h+1, W-w+1] bool: the h x w window whose corner is here lies inside `free` (an integral image)."""
    c = np.zeros((free.shape[0] + 1, free.shape[1] + 1), np.int64)
    c[1:, 1:] = free.cumsum(0).cumsum(1)
    return c[h:, w:] - c[:-h, w:] - c[h:, :-w] + c[:-h, :-w] == h * w


def shelves(H, W, seed, wall_at=0.55, back=False, noise=0.0005, holes=0.05, nbox=3):
    """(labels [H,W] int32, xyz [3,H,W] float32, surface [H,W] int: SURFACES): the §13 table, ray-cast; a shelf board
    BOARD_T above it over BOARD_A x BOARD_B; a wall perpendicular to the table, WALL_T high, hiding what lies behind it: a
    side wall at in-plane a = wall_at, or with back=True a back wall at in-plane b = wall_at facing the camera (near
    enough, it covers more pixels than the table does); the far patch where nothing is hit; `nbox` labelled box tops
    lifted 4-15 cm off the table (ids 1..) and as many off the board (ids 11..); two unlabelled mats on the table, 4.5 mm
    and 15 mm thick, which end up in the removal fringe of the table at tau / rem = 3 / 6 and 10 / 20.  Millimetre depth,
    gaussian z noise, `holes` of the pixels without depth."""
    rng = np.random.default_rng(seed)
    n, u, v, foot = table_axes()
    f = 0.9 * max(H, W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(xs - (W - 1) / 2) / f, (ys - (H - 1) / 2) / f, np.ones((H, W))])
    nr, ur = np.tensordot(n, ray, 1), np.tensordot(v if back else u, ray, 1)

    def hit(z, ok):
        return np.where(ok & (z > 0.25), z, np.inf)

    with np.errstate(divide="ignore", invalid="ignore"):
        zt = -R.PLANE_D / nr
        zt = hit(zt, (nr < 0) & (zt < TABLE_Z))
        zb = (BOARD_T - R.PLANE_D) / nr
        pb = ray * zb - foot[:, None, None]
        ab, bb = np.tensordot(u, pb, 1), np.tensordot(v, pb, 1)
        zb = hit(zb, (nr < 0) & (ab >= BOARD_A[0]) & (ab <= BOARD_A[1]) & (bb >= BOARD_B[0]) & (bb <= BOARD_B[1]))
        zw = wall_at / ur
        tw = nr * zw + R.PLANE_D
        zw = hit(zw, (ur > 0) & (tw >= 0) & (tw <= WALL_T) & (zw < TABLE_Z))
    z = np.minimum(np.minimum(zt, zb), zw)
    surf = np.where(z == zw, SURFACES["wall"], np.where(z == zb, SURFACES["board"], SURFACES["table"]))
    surf = np.where(np.isfinite(z), surf, SURFACES["far"])
    z = np.where(np.isfinite(z), z, R.Z_FAR)
    lab = np.zeros((H, W), np.int32)
    lift = np.zeros((H, W))
    bh, bw = max(2, H // 10), max(2, W // 12)
    for name, first in (("table", 1), ("board", 11)):
        for k in range(nbox):
            free = (surf == SURFACES[name]) & (lab == 0)
            spots = np.argwhere(_all_free(free, bh + 2, bw + 2))      # a free rim around it
            if not len(spots):
                break
            y0, x0 = spots[int(rng.integers(len(spots)))] + 1
            lab[y0:y0 + bh, x0:x0 + bw] = first + k
            lift[y0:y0 + bh, x0:x0 + bw] = rng.uniform(0.04, 0.15)
    mh, mw = max(2, H // 16), max(3, W // 16)
    for thick in MATS:
        free = (surf == SURFACES["table"]) & (lab == 0) & (lift == 0)
        spots = np.argwhere(_all_free(free, mh + 2, mw + 2))
        if len(spots):
            y0, x0 = spots[int(rng.integers(len(spots)))] + 1
            lift[y0:y0 + mh, x0:x0 + mw] = thick
    p = ray * z + lift * n[:, None, None]
    zz = np.round((p[2] + noise * rng.standard_normal((H, W))) * 1000.0) / 1000.0
    xyz = (p * (zz / p[2])).astype(np.float32)
    xyz[:, rng.random((H, W)) < holes] = 0.0
    return lab, xyz, surf


def _mm(q):
    return np.asarray(q, np.float32) / np.float32(1000.0)


def stairs(H=32, W=24):
    """Eight frontal strips of H/8 rows each at depths 600 + 40 k + 12 k^2 mm (not in arithmetic progression, so that no
    tilted plane collects a row of every strip), given directly in millimetres: every pure
    hypothesis of a round scores the same H/8 * W, so the tie rule decides, and K = 8 uses every slot."""
    ys, xs = np.mgrid[0:H, 0:W]
    k = ys // (H // 8)
    return np.zeros((H, W), np.int32), _mm(np.stack([4 * xs - 2 * W, 30 * ys, 600 + 40 * k + 12 * k * k]))


def parallel_pair(H=24, W=32):
    """Two frontal planes 15 mm apart (800 and 815 mm) on a checkerboard of pixels, and one object 5 cm in front."""
    ys, xs = np.mgrid[0:H, 0:W]
    xyz = _mm(np.stack([4 * xs - 2 * W, 3 * ys, 800 + 15 * ((xs + ys) & 1)]))
    lab = np.zeros((H, W), np.int32)
    lab[4:8, 5:11] = 4
    xyz[2][lab == 4] = np.float32(0.75)
    return lab, xyz


def grid_plane(H=12, W=16):
    return np.zeros((H, W), np.int32), R._grid_plane(H, W)


def stop_two_left(H=12, W=16):
    """The grid plane and two points far off it: M_1 = 2."""
    lab, xyz = grid_plane(H, W)
    xyz[:, 2, 3] = (0.01, 0.02, 1.9)
    xyz[:, 9, 12] = (-0.03, 0.0, 2.4)
    return lab, xyz


def stop_coincident_left(H=12, W=16):
    """The grid plane and seven copies of one point far off it: every hypothesis of round 1 is degenerate."""
    lab, xyz = grid_plane(H, W)
    for k in range(7):
        xyz[:, (5 * k) % H, (7 * k + 1) % W] = (0.02, -0.01, 2.0)
    return lab, xyz


STOPS = {"grid": grid_plane, "two_left": stop_two_left, "coincident_left": stop_coincident_left}
