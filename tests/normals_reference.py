"""Plain numpy / Python restatement of uoc_normals (include/uoc_hip.h): the semantics the GPU tests check against.
`estimate` is the definition with int64 arrays, `estimate_pixelwise` the same definition again pixel by pixel with Python
ints and math.isqrt; tests/test_normals_host.py holds the two together.  Also the seeded `boxes_scene` and the engineered
frames of the GPU tests; the host test asserts that they contain what they are used for."""
import math

import numpy as np

from tests import placement_reference as S15
from tests import support_reference as S13

NUM_IDS = 128
FACE_WORDS = 40
Q_MAX = 524287
D_MAX = 16383
UP, SIDE, OBLIQUE, DOWN = 1, 2, 3, 4
FACE_FIELDS = ("pixels", "with_normal", "up", "side", "oblique", "down", "grazing", "peak")


def direction_table(A):
    k = np.arange(A, dtype=np.float64)
    return np.stack([np.rint(np.cos(2 * np.pi * k / A) * 16384.0), np.rint(np.sin(2 * np.pi * k / A) * 16384.0)], axis=1).astype(np.int32)


def thresholds(up_deg, side_deg):
    return int(np.rint(np.cos(np.deg2rad(np.float64(up_deg))) * 2.0 ** 28)), int(np.rint(np.sin(np.deg2rad(np.float64(side_deg))) * 2.0 ** 28))


def default_min_pairs(window):
    return max(1, int(window) // 2)


# ---- P: points --------------------------------------------------------------------------------------------------------------
def points(xyz):
    """(valid [H,W] bool, q [3,H,W] int64, zero where not valid)."""
    X = np.asarray(xyz, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(X).all(axis=0) & (X[2] > 0)
        r = np.rint(X * np.float32(16000.0))                    # fp32 product, round half to even
        valid &= (np.abs(r) <= Q_MAX).all(axis=0)
    return valid, np.where(valid, r, 0).astype(np.int64)


def ids(labels, shape):
    if labels is None:
        return np.zeros(shape, np.int64)
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 1) & (lab < NUM_IDS), lab, 0)


# ---- D: pairs ---------------------------------------------------------------------------------------------------------------
def pairs(valid, q, ident, r, jump_mm, axis):
    """(exists [H,W] bool, d [3,H,W] int64, ida [H,W]) of the pairs along `axis` (1: horizontal, 0: vertical)."""
    H, W = valid.shape
    exists = np.zeros((H, W), bool)
    d = np.zeros((3, H, W), np.int64)
    ida = np.zeros((H, W), np.int64)
    n = (H, W)[axis]
    if n <= 2 * r:
        return exists, d, ida
    mid = (slice(None), slice(r, n - r)) if axis == 1 else (slice(r, n - r), slice(None))
    lo = (slice(None), slice(0, n - 2 * r)) if axis == 1 else (slice(0, n - 2 * r), slice(None))
    hi = (slice(None), slice(2 * r, n)) if axis == 1 else (slice(2 * r, n), slice(None))
    dd = q[(slice(None),) + hi] - q[(slice(None),) + lo]
    ok = valid[lo] & valid[hi] & (ident[lo] == ident[hi]) & (np.abs(dd[2]) <= 16 * jump_mm) & (np.abs(dd[0]) <= D_MAX) \
        & (np.abs(dd[1]) <= D_MAX)
    exists[mid] = ok
    d[(slice(None),) + mid] = dd * ok
    ida[mid] = ident[lo]
    return exists, d, ida


# ---- T: tangents --------------------------------------------------------------------------------------------------------------
def tangent(exists, d, ida, ident, s):
    """(T [3,H,W] int64, count [H,W] int64) over the window of half-width s."""
    H, W = exists.shape
    T = np.zeros((3, H, W), np.int64)
    cnt = np.zeros((H, W), np.int64)
    E = np.zeros((H + 2 * s, W + 2 * s), bool)
    D = np.zeros((3, H + 2 * s, W + 2 * s), np.int64)
    I = np.zeros((H + 2 * s, W + 2 * s), np.int64)
    E[s:s + H, s:s + W], D[:, s:s + H, s:s + W], I[s:s + H, s:s + W] = exists, d, ida
    for di in range(2 * s + 1):
        for dj in range(2 * s + 1):
            m = E[di:di + H, dj:dj + W] & (I[di:di + H, dj:dj + W] == ident)
            T += D[:, di:di + H, dj:dj + W] * m
            cnt += m
    return T, cnt


def isqrt_array(S):
    r = np.floor(np.sqrt(S.astype(np.float64))).astype(np.int64)
    for _ in range(4):
        r -= (r * r > S)
        r += ((r + 1) * (r + 1) <= S)
    return r


def frame_axes(plane):
    """(Pq, Uq, Vq) int64 [3] from a plane dict / uoc_plane record through rule F of the placement reference, or None."""
    if plane is None:
        return None
    if not isinstance(plane, dict):
        plane = S15.plane_from_record(plane)
    F = S15.frame_record(plane)
    if F[13] != 1:
        return None
    return F[0:3].copy(), F[4:7].copy(), F[7:10].copy()


def estimate(xyz, labels=None, plane=None, step=2, window=2, jump_mm=30, min_pairs=None, dirs=None, c_up=None, s_side=None,
             parts=False):
    """One frame.  Returns dict(n [H,W,3] int64, info [H,W] int64, faces [128,40] int64, unit [3,H,W] float64)."""
    r, s = int(step), int(window)
    mp = default_min_pairs(s) if min_pairs is None else int(min_pairs)
    dirs = direction_table(16) if dirs is None else np.asarray(dirs, np.int64).reshape(-1, 2)
    if c_up is None:
        c_up, s_side = thresholds(20.0, 20.0)
    X = np.asarray(xyz, np.float32)
    H, W = X.shape[1:]
    valid, q = points(X)
    ident = ids(labels, (H, W))
    TX, nX = tangent(*pairs(valid, q, ident, r, jump_mm, 1), ident, s)
    TY, nY = tangent(*pairs(valid, q, ident, r, jump_mm, 0), ident, s)
    assert np.abs(TX).max(initial=0) < 1 << 21 and np.abs(TY).max(initial=0) < 1 << 21
    N = np.stack([TY[1] * TX[2] - TY[2] * TX[1], TY[2] * TX[0] - TY[0] * TX[2], TY[0] * TX[1] - TY[1] * TX[0]])
    g = np.abs(N).max(axis=0)
    assert g.max(initial=0) < 1 << 43
    k = np.zeros((H, W), np.int64)
    for j in range(14):
        k += g >= (1 << (30 + j))
    n = N >> k                                               # arithmetic: a floor
    has = valid & (nX >= mp) & (nY >= mp) & (n != 0).any(axis=0)
    n = n * has
    graz = has & ((n * (q >> 4)).sum(axis=0) >= 0)
    S = (n * n).sum(axis=0)
    assert S.max(initial=0) < 1 << 62
    cls = np.zeros((H, W), np.int64)
    binz = np.zeros((H, W), np.int64)
    axes = frame_axes(plane)
    if axes is not None:
        Pq, Uq, Vq = (a.astype(np.int64) for a in axes)
        c = np.tensordot(Pq, n, 1)
        L = isqrt_array(S)
        c16, t = c * 16384, int(c_up) * L
        up = c16 >= t
        down = ~up & (-c16 >= t)
        side = ~up & ~down & (np.abs(c16) <= int(s_side) * L)
        cls = np.where(up, UP, np.where(down, DOWN, np.where(side, SIDE, OBLIQUE))) * has
        a, b = np.tensordot(Uq, n, 1), np.tensordot(Vq, n, 1)
        score = a[None] * dirs[:, 0, None, None].astype(np.int64) + b[None] * dirs[:, 1, None, None].astype(np.int64)
        binz = np.argmax(score, axis=0).astype(np.int64) * (cls == SIDE)       # the first maximum: ties to the lowest k
    info = (cls | (graz.astype(np.int64) << 3) | (binz << 8) | (nX << 16) | (nY << 24)) * has
    faces = np.zeros((NUM_IDS, FACE_WORDS), np.int64)
    flat = ident.reshape(-1)
    faces[:, 0] = np.bincount(flat, minlength=NUM_IDS)
    faces[:, 1] = np.bincount(flat[has.reshape(-1)], minlength=NUM_IDS)
    for c_, col in ((UP, 2), (SIDE, 3), (OBLIQUE, 4), (DOWN, 5)):
        faces[:, col] = np.bincount(flat[(cls == c_).reshape(-1)], minlength=NUM_IDS)
    faces[:, 6] = np.bincount(flat[graz.reshape(-1)], minlength=NUM_IDS)
    sd = (cls == SIDE).reshape(-1)
    np.add.at(faces, (flat[sd], 8 + binz.reshape(-1)[sd]), 1)
    faces[:, 7] = np.where(faces[:, 3] > 0, np.argmax(faces[:, 8:], axis=1), -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(has, n.astype(np.float64) / np.sqrt(S.astype(np.float64)), np.nan)
    out = dict(n=np.moveaxis(n, 0, -1), info=info, faces=faces, unit=unit)
    if parts:
        out.update(valid=valid, q=q, id=ident, TX=TX, TY=TY, nX=nX, nY=nY, N=N, k=k, has=has, cls=cls, bin=binz, grazing=graz)
    return out


def estimate_batch(xyz, labels=None, planes=None, **kw):
    """[B,...] inputs; planes: a list of plane dicts / records / None per frame, or None.  Stacked n, info, faces, unit."""
    B = len(xyz)
    res = [estimate(xyz[b], None if labels is None else labels[b], None if planes is None else planes[b], **kw) for b in range(B)]
    return {k: np.stack([r[k] for r in res]) for k in ("n", "info", "faces", "unit")}


# ---- the same definition, pixel by pixel ------------------------------------------------------------------------------------
def estimate_pixelwise(xyz, labels=None, plane=None, step=2, window=2, jump_mm=30, min_pairs=None, dirs=None, c_up=None,
                       s_side=None):
    r, s = int(step), int(window)
    mp = default_min_pairs(s) if min_pairs is None else int(min_pairs)
    dirs = [(int(a), int(b)) for a, b in (direction_table(16) if dirs is None else np.asarray(dirs).reshape(-1, 2))]
    if c_up is None:
        c_up, s_side = thresholds(20.0, 20.0)
    X = np.asarray(xyz, np.float32)
    H, W = X.shape[1:]
    lab = None if labels is None else np.asarray(labels)
    axes = frame_axes(plane)
    if axes is not None:
        Pq, Uq, Vq = ([int(v) for v in a] for a in axes)

    def point(y, x):
        if not (0 <= y < H and 0 <= x < W):
            return None
        v = [X[c, y, x] for c in range(3)]
        if not all(np.isfinite(t) for t in v) or not v[2] > 0:
            return None
        qq = [float(np.rint(np.float32(t) * np.float32(16000.0))) for t in v]
        if any(abs(t) > Q_MAX for t in qq):
            return None
        return [int(t) for t in qq]

    def ident(y, x):
        if lab is None:
            return 0
        l = int(lab[y, x])
        return l if 1 <= l <= 127 else 0

    def pair(y, x, dy, dx):
        a, b = point(y - dy, x - dx), point(y + dy, x + dx)
        if a is None or b is None or ident(y - dy, x - dx) != ident(y + dy, x + dx):
            return None
        d = [b[c] - a[c] for c in range(3)]
        if abs(d[2]) > 16 * jump_mm or abs(d[0]) > D_MAX or abs(d[1]) > D_MAX:
            return None
        return d, ident(y - dy, x - dx)

    n_out = np.zeros((H, W, 3), np.int64)
    info = np.zeros((H, W), np.int64)
    faces = np.zeros((NUM_IDS, FACE_WORDS), np.int64)
    for y in range(H):
        for x in range(W):
            me = ident(y, x)
            faces[me, 0] += 1
            q = point(y, x)
            if q is None:
                continue
            T, cnt = [[0, 0, 0], [0, 0, 0]], [0, 0]
            for my in range(y - s, y + s + 1):
                for mx in range(x - s, x + s + 1):
                    for t, (dy, dx) in enumerate(((0, r), (r, 0))):
                        p = pair(my, mx, dy, dx)
                        if p is not None and p[1] == me:
                            T[t] = [T[t][c] + p[0][c] for c in range(3)]
                            cnt[t] += 1
            if cnt[0] < mp or cnt[1] < mp:
                continue
            tx, ty = T
            N = [ty[1] * tx[2] - ty[2] * tx[1], ty[2] * tx[0] - ty[0] * tx[2], ty[0] * tx[1] - ty[1] * tx[0]]
            k = max(0, max(abs(v) for v in N).bit_length() - 30)
            n = [v >> k for v in N]
            if not any(n):
                continue
            graz = int(sum(n[c] * (q[c] >> 4) for c in range(3)) >= 0)
            cls = b_ = 0
            if axes is not None:
                c = sum(n[i] * Pq[i] for i in range(3))
                L = math.isqrt(sum(v * v for v in n))
                if c * 16384 >= c_up * L:
                    cls = UP
                elif -c * 16384 >= c_up * L:
                    cls = DOWN
                elif abs(c) * 16384 <= s_side * L:
                    cls = SIDE
                    a, b = sum(n[i] * Uq[i] for i in range(3)), sum(n[i] * Vq[i] for i in range(3))
                    sc = [a * cx + b * cy for cx, cy in dirs]
                    b_ = sc.index(max(sc))
                    faces[me, 8 + b_] += 1
                else:
                    cls = OBLIQUE
                faces[me, 1 + cls] += 1
            faces[me, 1] += 1
            faces[me, 6] += graz
            n_out[y, x] = n
            info[y, x] = cls | graz << 3 | b_ << 8 | cnt[0] << 16 | cnt[1] << 24
    for a in range(NUM_IDS):
        hist = [int(v) for v in faces[a, 8:]]
        faces[a, 7] = hist.index(max(hist)) if faces[a, 3] > 0 else -1
    return dict(n=n_out, info=info, faces=faces)


def angle_deg(n, ref):
    """Angle in degrees between integer normals [...,3] and the direction ref, float64."""
    v = np.asarray(n, np.float64)
    ref = np.asarray(ref, np.float64) / np.linalg.norm(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (v @ ref) / np.linalg.norm(v, axis=-1)
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def plane_axes():
    """(u, v): in-plane axes of the tabletop plane, u from the x axis as uoc_support_plane builds it, v = n x u."""
    n = S13.PLANE_N
    u = np.array([1.0, 0.0, 0.0]) - n[0] * n
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


def table_plane():
    """The generating plane of tabletop / boxes_scene as a plane dict (float32 fields) for rule F."""
    u, v = plane_axes()
    n = S13.PLANE_N
    centroid = -S13.PLANE_D * n                         # the foot of the camera on the plane
    return dict(found=1, normal=n.astype(np.float32), d=np.float32(S13.PLANE_D), centroid=centroid.astype(np.float32),
                u=u.astype(np.float32), v=v.astype(np.float32))


MIRROR = (10, 14)     # rows, columns of the mirrored patch in the bottom-left corner of boxes_scene


def boxes_scene(H, W, seed, nobj=5, noise=0.0005, holes=0.05, mirror=True):
    """(labels [H,W] int32, xyz [3,H,W] float32): the tilted plane of support_reference.tabletop, ray-cast, carrying `nobj`
    upright cuboids with random yaw (so that side faces exist), a wall at Z_FAR, gaussian z noise, z in whole millimetres
    and `holes` of the pixels without depth.  With `mirror` the columns of the bottom-left MIRROR patch are reversed, labels
    and points alike: there the cloud is mirrored, every normal faces away from the camera (grazing) and down."""
    rng = np.random.default_rng(seed)
    f = 0.9 * max(H, W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(xs - (W - 1) / 2) / f, (ys - (H - 1) / 2) / f, np.ones((H, W))])
    n = S13.PLANE_N
    u, v = plane_axes()
    denom = np.tensordot(n, ray, 1)
    with np.errstate(divide="ignore"):
        z = np.where(denom < 0, -S13.PLANE_D / np.where(denom < 0, denom, -1.0), np.inf)
    z = np.where((z > 0.25) & (z < S13.Z_CUT), z, S13.Z_FAR)
    lab = np.zeros((H, W), np.int32)
    for k in range(nobj):
        # a spot on the plane in front of the camera, 0.6 .. 1.0 m deep
        zc = rng.uniform(0.6, 1.0)
        xc = rng.uniform(-0.25, 0.25) * zc
        yc = -(S13.PLANE_D + n[0] * xc + n[2] * zc) / n[1]
        c = np.array([xc, yc, zc])
        yaw = rng.uniform(0.0, np.pi)
        e1, e2 = np.cos(yaw) * u + np.sin(yaw) * v, -np.sin(yaw) * u + np.cos(yaw) * v
        half = (rng.uniform(0.04, 0.09), rng.uniform(0.04, 0.09))
        height = rng.uniform(0.06, 0.16)
        tmin, tmax = np.full((H, W), -np.inf), np.full((H, W), np.inf)
        for axis, lo, hi in ((e1, -half[0], half[0]), (e2, -half[1], half[1]), (n, 0.0, height)):
            o, d = -float(axis @ c), np.tensordot(axis, ray, 1)          # the ray starts at the camera: p = t * ray
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (lo - o) / d, (hi - o) / d
            tmin, tmax = np.maximum(tmin, np.minimum(t0, t1)), np.minimum(tmax, np.maximum(t0, t1))
        hit = (tmin <= tmax) & (tmin > 0.25) & (tmin < z)
        z = np.where(hit, tmin, z)
        lab[hit] = k + 1
    zz = np.round((z + noise * rng.standard_normal((H, W))) * 1000.0) / 1000.0
    xyz = (ray * zz).astype(np.float32)
    xyz[:, rng.random((H, W)) < holes] = 0.0
    if mirror:
        mh, mw = min(MIRROR[0], H), min(MIRROR[1], W)
        xyz[:, H - mh:, :mw] = xyz[:, H - mh:, :mw][:, :, ::-1].copy()
        lab[H - mh:, :mw] = lab[H - mh:, :mw][:, ::-1].copy()
    return lab, xyz


def frontal(H, W, z_mm=700, pitch_mm=2):
    """A frontal plane z = z_mm with x, y on a millimetre lattice: every normal is exactly (0, 0, -c)."""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([(xs - W // 2) * pitch_mm, (ys - H // 2) * pitch_mm, np.full((H, W), z_mm)]).astype(np.float32) / np.float32(1000.0)


def frontal_plane_tuple():
    """(normal, d, centroid, u, v) of the plane z = 0.7 m with the normal towards the camera."""
    return (np.array([0.0, 0.0, -1.0]), 0.7, np.array([0.0, 0.0, 0.7]), np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0]))


def plane_dict(normal, d, centroid, u, v):
    return dict(found=1, normal=np.asarray(normal, np.float32), d=np.float32(d), centroid=np.asarray(centroid, np.float32),
                u=np.asarray(u, np.float32), v=np.asarray(v, np.float32))


def case_tie(H=12, W=16):
    """A surface whose normal lies in the support plane at exactly 45 degrees between u and v.  The surface is z = 700 + x:
    columns 2 mm apart in x and 2 mm in z, rows 2 mm apart in y;
    N is proportional to (1, 0, -1).  With the support plane normal (0, 1, 0), u = (1, 0, 0), v = (0, 0, -1) this gives
    c = 0 (SIDE), a = b: with A = 4 the bins 0 and 1 tie and the lower wins."""
    ys, xs = np.mgrid[0:H, 0:W]
    xyz = np.stack([2 * xs - W, 2 * ys - H, 700 + 2 * xs]).astype(np.float32) / np.float32(1000.0)
    plane = plane_dict((0.0, 1.0, 0.0), 0.0, (0.0, 0.0, 0.7), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    return xyz, plane


def case_mirrored(H=12, W=16):
    """The grid plane with its columns reversed: a mirrored cloud, every pixel with a normal is grazing."""
    return np.ascontiguousarray(S13._grid_plane(H, W)[:, :, ::-1])


def case_collinear(H=10, W=12):
    """Every point on one line: every tangent is parallel, N = 0, no pixel has a normal."""
    i = (np.mgrid[0:H, 0:W][0] * 3 + np.mgrid[0:H, 0:W][1]).astype(np.float64)
    return np.stack([i, 2 * i, 500 + 3 * i]).astype(np.float32) / np.float32(1000.0)


def case_range(H=12, W=16):
    """The grid plane with coordinates at the edge of the 20-bit range (+-32.767 m is valid: q = 524272; 32.7679375 m is
    q = 524287, the last valid value; 32.768 m is not), and pair components of exactly 16383 and 16384 sixteenths."""
    xyz = S13._grid_plane(H, W).copy()
    edge = [(32.767, 0.0, 1.0), (-32.767, 0.0, 1.0), (0.0, 32.767, 1.0), (0.0, 0.0, 32.767), (524287 / 16000.0, 0.0, 1.0),
            (32.768, 0.0, 1.0), (-32.768, 0.0, 1.0), (0.0, -32.768, 1.0), (0.0, 0.0, 32.768), (0.0, 0.0, 33.0), (-40.0, 0.0, 1.0)]
    for k, val in enumerate(edge):
        xyz[:, k % H, (3 * k) % W] = val
    # row H-3: x steps so that the pair across column 5 (step 1: columns 4 and 6) spans 16383/16 mm, across column 9 16384/16 mm
    xyz[0, H - 3, 4], xyz[0, H - 3, 6] = 0.0, np.float32(16383 / 16000.0)
    xyz[0, H - 3, 8], xyz[0, H - 3, 10] = 0.0, np.float32(16384 / 16000.0)
    return xyz


def case_nasty(H=40, W=56, seed=5):
    """A boxes scene with NaN, inf, zero and negative z, NaN x, labels 0, 128, -1, 1000 on the background, id 127 and a
    one-pixel object."""
    rng = np.random.default_rng(seed)
    lab, xyz = boxes_scene(H, W, seed, nobj=4)
    bg = lab == 0
    lab[bg] = rng.choice(np.array([0, 128, -1, 1000], np.int32), size=int(bg.sum()))
    c = rng.random((H, W)) < 0.08
    xyz[2][c] = rng.choice(np.array([0.0, -0.5, np.nan, np.inf, -np.inf], np.float32), size=int(c.sum()))
    xyz[0][rng.random((H, W)) < 0.01] = np.nan
    lab[lab == 1] = 127
    lab[H // 2, W // 2] = 50
    return lab, xyz


def case_all_ids(H=48, W=64):
    """127 ids at once: the boxes scene cut into 4 x 4 blocks."""
    _, xyz = boxes_scene(H, W, 3, mirror=False)
    ys, xs = np.mgrid[0:H, 0:W]
    return (((ys // 4) * (W // 4) + xs // 4) % 127 + 1).astype(np.int32), xyz


def plane_record(plane):
    """A plane dict (or None: a frame without a plane) as a uoc_plane record, 21 int32 words: the inverse of the placement
    reference's plane_from_record."""
    rec = np.zeros(21, np.float32)
    out = rec.view(np.int32)
    if plane is not None:
        rec[4:7], rec[7], rec[8:11] = plane["normal"], plane["d"], plane["centroid"]
        rec[15:18], rec[18:21] = plane["u"], plane["v"]
        out[0] = int(plane["found"])
    return out
