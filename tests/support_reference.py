"""Plain numpy restatement of uoc_support_plane (include/uoc_hip.h): the semantics the GPU tests check against.  Steps A
and B (candidates, hypotheses, scores, winner) are exact integers (int64 arrays, Python ints, math.isqrt); steps C and D
(refinement, objects) are float64 with numpy's own eigen-solver.  Also the seeded tabletop scenes and the engineered
cases of the GPU tests; tests/test_support_host.py asserts that they contain what they are used for."""
import math

import numpy as np

NUM_IDS = 128
Q_MAX = 32767


# ---- steps A, B: integers --------------------------------------------------------------------------------------------
def mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample_indices(h, M, seed):
    return [(mix(seed ^ (((3 * h + k) * 0x9E3779B9) & 0xFFFFFFFF)) * M) >> 32 for k in range(3)]


def valid_points(xyz):
    """[H*W] bool: finite x, y, z and z > 0.  xyz [3,H,W] float32."""
    X = np.asarray(xyz, np.float32).reshape(3, -1)
    with np.errstate(invalid="ignore"):
        return np.isfinite(X).all(axis=0) & (X[2] > 0)


def candidates(labels, xyz):
    """(raster indices [M], q [M,3] int64) of the candidates of one frame."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    X = np.asarray(xyz, np.float32).reshape(3, -1)
    ok = ~((lab >= 1) & (lab < NUM_IDS)) & valid_points(xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(X * np.float32(1000.0))                     # fp32 product, round half to even
        ok &= (np.abs(r) <= Q_MAX).all(axis=0)
    idx = np.nonzero(ok)[0]
    return idx, r[:, idx].T.astype(np.int64)


def hypothesis(q, h, tau_mm, seed):
    """(n' as Python ints, p0, tau_mm * L) of hypothesis h, or None when it is degenerate."""
    p = [[int(v) for v in q[i]] for i in sample_indices(h, len(q), seed)]
    a = [p[1][k] - p[0][k] for k in range(3)]
    b = [p[2][k] - p[0][k] for k in range(3)]
    n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    g = max(abs(v) for v in n)
    s = max(0, g.bit_length() - 30)
    n = [(abs(v) >> s) * (1 if v > 0 else -1) for v in n]
    if not any(n):
        return None
    L = math.isqrt(sum(v * v for v in n))
    return n, p[0], tau_mm * L


def inlier_mask(q, hyp):
    n, p0, thr = hyp
    dot = (q - np.array(p0, np.int64)) @ np.array(n, np.int64)       # below 2^49: exact in int64
    return np.abs(dot) <= thr


def scores(q, num_hyp, tau_mm, seed):
    """int64 [num_hyp]: inliers per hypothesis, -1 for a degenerate one (all -1 when M < 3)."""
    out = np.full(num_hyp, -1, np.int64)
    if len(q) < 3:
        return out
    for h in range(num_hyp):
        hyp = hypothesis(q, h, tau_mm, seed)
        if hyp is not None:
            out[h] = int(inlier_mask(q, hyp).sum())
    return out


# ---- steps C, D: float64 ------------------------------------------------------------------------------------------------
def sign_rule(e):
    k = int(np.argmax(np.abs(e)))          # the first maximum
    return -e if e[k] < 0 else e


def refine(pts):
    """pts [n,3] float64 -> dict normal, d, centroid, eig (descending, never negative), u, v; `points` and `cov` keep the
    input and its fp64 covariance for the gap-independent checker (tests/stats_cases.py)."""
    c = pts.mean(axis=0)
    dd = pts - c
    cov = dd.T @ dd / len(pts)
    w, vec = np.linalg.eigh(cov)
    w = np.maximum(w, 0.0)
    normal = vec[:, 0]
    d = -float(normal @ c)
    if d < 0:
        normal, d = -normal, -d
    elif d == 0:
        normal, d = sign_rule(normal), 0.0
    for axis in range(2):
        e = np.zeros(3)
        e[axis] = 1.0
        u = e - normal[axis] * normal
        if np.linalg.norm(u) >= 1e-6:
            break
    u = u / np.linalg.norm(u)
    return dict(normal=normal, d=d, centroid=c, eig=w[::-1].copy(), u=u, v=np.cross(normal, u), points=pts, cov=cov)


def object_record(pts, pl):
    """Valid points [n,3] float64 of one id against the refined plane (`points` keeps them for the checker)."""
    t = pts @ pl["normal"] + pl["d"]
    ab = np.stack([(pts - pl["centroid"]) @ pl["u"], (pts - pl["centroid"]) @ pl["v"]], axis=1)
    foot = ab.mean(axis=0)
    r = ab - foot
    cov = r.T @ r / len(pts)
    w, vec = np.linalg.eigh(cov)
    gap = float(w[1] - w[0])
    e = np.array([1.0, 0.0])
    if gap > 0:
        e = vec[:, 1]
        e = -e if (e[1] if abs(e[1]) > abs(e[0]) else e[0]) < 0 else e
    ep = np.array([-e[1], e[0]])
    proj = np.stack([r @ e, r @ ep, t], axis=1)
    lo, hi = proj.min(axis=0), proj.max(axis=0)
    mid = (lo + hi) / 2
    m_ab = foot + mid[0] * e + mid[1] * ep
    center = pl["centroid"] + m_ab[0] * pl["u"] + m_ab[1] * pl["v"] + mid[2] * pl["normal"]
    return dict(count=len(pts), height_min=t.min(), height_max=t.max(), foot=foot, cov2=np.array([cov[0, 0], cov[0, 1], cov[1, 1]]),
                axis=e, half=(hi - lo) / 2, center=center, lam0=float(w[1]), gap=gap, points=pts)


def fit(labels, xyz, num_hyp, tau_mm, seed, height_map=False):
    """One frame: labels [H,W] ints, xyz [3,H,W] float32.  Returns dict(plane=..., objects={id: record}, height=[H,W]
    float64 with NaN or None, scores=int64 [num_hyp]); plane has found, candidates, inliers, hyp and, when found, the
    float fields as float64; xyz = the input as [3, H*W] float32."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    X = np.asarray(xyz, np.float32).reshape(3, -1)
    idx, q = candidates(lab, xyz)
    sc = scores(q, num_hyp, tau_mm, seed)
    plane = dict(found=0, candidates=len(q), inliers=0, hyp=0)
    height = np.full(H * W, np.nan) if height_map else None
    objects = {}
    if sc.max() >= 0:
        h = int(np.argmax(sc))                 # the first maximum: ties go to the lowest h
        inl = idx[inlier_mask(q, hypothesis(q, h, tau_mm, seed))]
        assert len(inl) == sc[h]
        plane.update(found=1, inliers=int(sc[h]), hyp=h, **refine(X[:, inl].T.astype(np.float64)))
        plane["rms"] = math.sqrt(max(plane["eig"][2], 0.0))
        valid = valid_points(xyz)
        if height_map:
            height[valid] = X[:, valid].T.astype(np.float64) @ plane["normal"] + plane["d"]
        flat = lab.reshape(-1)
        for l in range(1, NUM_IDS):
            sel = np.nonzero((flat == l) & valid)[0]
            if len(sel):
                objects[l] = object_record(X[:, sel].T.astype(np.float64), plane)
    return dict(plane=plane, objects=objects, height=None if height is None else height.reshape(H, W), scores=sc, xyz=X)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.06, -0.80, -0.597])
PLANE_N = PLANE_N / np.linalg.norm(PLANE_N)
PLANE_D = 0.55
Z_CUT, Z_FAR = 1.5, 4.0      # the table ends where its depth reaches Z_CUT; behind it a wall at Z_FAR, farther than the
                             # plane gets inside any of the test images, so the two never meet


def tabletop(H, W, seed, nobj=6, noise=0.0005, holes=0.05):
    """(labels [H,W] int32, xyz [3,H,W] float32): a pinhole camera over the tilted plane PLANE_N.p + PLANE_D = 0,
    ray-cast per pixel (a true plane in XYZ), a wall at Z_FAR where the plane leaves the depth range (z >= Z_CUT), `nobj` labelled
    rectangles lifted 4-15 cm off the plane along its normal, gaussian z noise, z in whole millimetres as a depth sensor
    delivers it, and `holes` of the pixels without depth (0, 0, 0)."""
    rng = np.random.default_rng(seed)
    f = 0.9 * max(H, W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    rx, ry = (xs - (W - 1) / 2) / f, (ys - (H - 1) / 2) / f
    denom = PLANE_N[0] * rx + PLANE_N[1] * ry + PLANE_N[2]
    with np.errstate(divide="ignore"):
        z = np.where(denom < 0, -PLANE_D / np.where(denom < 0, denom, -1.0), np.inf)
    z = np.where((z > 0.25) & (z < Z_CUT), z, Z_FAR)
    lab = np.zeros((H, W), np.int32)
    lift = np.zeros((H, W))
    for k in range(nobj):
        bh, bw = max(1, int(H * rng.uniform(0.08, 0.2))), max(1, int(W * rng.uniform(0.06, 0.16)))
        y0, x0 = int(rng.integers(H // 3, max(H // 3 + 1, H - bh))), int(rng.integers(0, max(1, W - bw)))
        lab[y0:y0 + bh, x0:x0 + bw] = k + 1
        lift[y0:y0 + bh, x0:x0 + bw] = rng.uniform(0.04, 0.15)
    p = np.stack([rx * z, ry * z, z]) + lift * PLANE_N[:, None, None]      # PLANE_N points at the camera side
    zz = np.round((p[2] + noise * rng.standard_normal((H, W))) * 1000.0) / 1000.0
    scale = zz / p[2]
    xyz = np.stack([p[0] * scale, p[1] * scale, zz]).astype(np.float32)
    xyz[:, rng.random((H, W)) < holes] = 0.0
    return lab, xyz


def _grid_plane(H, W):
    """A frontal tilted plane given directly in millimetres: q = (4x - 2W, 3y, 600 + x + 2y)."""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([4 * xs - 2 * W, 3 * ys, 600 + xs + 2 * ys]).astype(np.float32) / np.float32(1000.0)


def case_m0(H=8, W=9):
    return np.zeros((H, W), np.int32), np.zeros((3, H, W), np.float32)


def case_m2(H=8, W=9):
    lab, xyz = case_m0(H, W)
    xyz[:, 1, 2] = (0.1, 0.2, 0.9)
    xyz[:, 6, 7] = (-0.1, 0.1, 0.7)
    return lab, xyz


def case_m3(H=8, W=9):
    lab, xyz = case_m2(H, W)
    xyz[:, 4, 0] = (0.3, -0.2, 0.8)
    lab[2, 2], xyz[:, 2, 2] = 5, (0.0, 0.0, 0.5)          # one object point to measure
    return lab, xyz


def case_collinear(H=8, W=9):
    i = np.arange(H * W).reshape(H, W)
    xyz = np.stack([i, 2 * i, 500 + 3 * i]).astype(np.float32) / np.float32(1000.0)
    return np.zeros((H, W), np.int32), xyz


def case_coincident(H=8, W=9):
    xyz = np.empty((3, H, W), np.float32)
    xyz[:] = np.array([0.1, -0.05, 0.75], np.float32)[:, None, None]
    lab = np.zeros((H, W), np.int32)
    lab[0, :3] = 9
    return lab, xyz


def case_range(H=12, W=16):
    """The grid plane with coordinates at the int16 edge: +-32.767 m are candidates, +-32.768 m and beyond are not;
    32.7675 m and the half-millimetre values probe the rounding."""
    xyz = _grid_plane(H, W)
    lab = np.zeros((H, W), np.int32)
    edge = [(32.767, 0.0, 1.0), (-32.767, 0.0, 1.0), (0.0, 32.767, 1.0), (0.0, -32.767, 1.0), (0.0, 0.0, 32.767),
            (32.768, 0.0, 1.0), (-32.768, 0.0, 1.0), (0.0, 32.768, 1.0), (0.0, -32.768, 1.0), (0.0, 0.0, 32.768),
            (32.7675, 0.0, 1.0), (0.0, 0.0, 33.0), (-33.0, 0.0, 1.0), (0.0005, 0.0015, 0.0025)]
    for k, v in enumerate(edge):
        xyz[:, k % H, (3 * k) % W] = v
    lab[H - 2:, 6:9] = 7
    return lab, xyz


def case_nasty(H=40, W=56, seed=5):
    """A tabletop with NaN, inf, zero and negative z (and NaN x) among the background and the object pixels, background
    ids 0, 128, -1 and 1000, an object with one valid point (id 50) and one with none (id 51)."""
    rng = np.random.default_rng(seed)
    lab, xyz = tabletop(H, W, seed, nobj=4)
    bg = lab == 0
    lab[bg] = rng.choice(np.array([0, 128, -1, 1000], np.int32), size=int(bg.sum()))
    c = rng.random((H, W)) < 0.08
    xyz[2][c] = rng.choice(np.array([0.0, -0.5, np.nan, np.inf, -np.inf], np.float32), size=int(c.sum()))
    xyz[0][rng.random((H, W)) < 0.01] = np.nan
    lab[0, 0:3] = 50
    xyz[:, 0, 0:3] = 0.0
    xyz[:, 0, 1] = (0.01, -0.2, 0.9)
    lab[1, 0:3] = 51
    xyz[2, 1, 0:3] = (0.0, np.nan, -1.0)
    return lab, xyz


def case_all_objects(H=20, W=24):
    lab, xyz = tabletop(H, W, 3)
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys // 4) * 6 + xs // 4 + 1).astype(np.int32), xyz


def case_origin_plane(H=16, W=20):
    """The plane x = 0, through the camera origin: d == 0, the normal's sign comes from the sign rule and u from the y
    axis.  One object 5 cm off it."""
    ys, xs = np.mgrid[0:H, 0:W]
    xyz = np.stack([np.zeros((H, W)), (ys * 7 + xs - 60) / 1000.0, (500 + 11 * xs + ys) / 1000.0]).astype(np.float32)
    lab = np.zeros((H, W), np.int32)
    lab[3:6, 4:9] = 3
    xyz[0][lab == 3] = 0.05
    return lab, xyz


ENGINEERED = {"m0": case_m0, "m2": case_m2, "m3": case_m3, "collinear": case_collinear, "coincident": case_coincident,
              "range": case_range, "nasty": case_nasty, "all_objects": case_all_objects, "origin_plane": case_origin_plane}
