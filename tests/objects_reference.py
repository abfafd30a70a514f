"""float64 numpy restatement of uoc_objects (include/uoc_hip.h): the semantics the GPU tests check against.

A pixel of object l has label l in [1, 127]; a valid point is such a pixel with finite x, y, z and z > 0."""
import numpy as np

NUM_IDS = 128


def subsample_ranks(count, m):
    """In-object ranks kept by max_points_per_object = m: floor(j*count/m), j < m, when count > m > 0; else all."""
    if m is None or m <= 0 or count <= m:
        return np.arange(count, dtype=np.int64)
    j = np.arange(m, dtype=np.int64)
    return (j * np.int64(count)) // np.int64(m)


def sign_rule(e):
    """Flip e so that its component of largest magnitude is positive (ties: lowest index)."""
    k = int(np.argmax(np.abs(e)))          # argmax returns the first maximum
    return -e if e[k] < 0 else e


def eig_frame(cov):
    """(eigenvalues descending, axes [3,3] with column k = e_k) under the sign rule and e2 = e0 x e1."""
    w, v = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")
    w, v = np.maximum(w[order], 0.0), v[:, order]      # eigenvalues of a covariance: never negative (include/uoc_hip.h)
    e0, e1 = sign_rule(v[:, 0]), sign_rule(v[:, 1])
    return w, np.stack([e0, e1, np.cross(e0, e1)], axis=1)


def object_record(pts):
    """Float statistics of one object's valid points [n,3] (float64 in, float64 out); `points` keeps the input for the
    gap-independent checker (tests/stats_cases.py)."""
    n = len(pts)
    z3 = np.zeros(3)
    if n == 0:
        return dict(centroid=z3, cov=np.zeros((3, 3)), aabb_min=z3, aabb_max=z3, eig=z3, axes=np.zeros((3, 3)),
                    obb_center=z3, obb_half=z3, points=np.zeros((0, 3)))
    p = pts.astype(np.float64)
    c = p.mean(axis=0)
    d = p - c
    cov = d.T @ d / n
    w, ax = eig_frame(cov)
    proj = d @ ax
    lo, hi = proj.min(axis=0), proj.max(axis=0)
    return dict(centroid=c, cov=cov, aabb_min=p.min(axis=0), aabb_max=p.max(axis=0), eig=w, axes=ax,
                obb_center=c + ax @ ((lo + hi) / 2), obb_half=(hi - lo) / 2, points=p)


def extract(labels, xyz, attrs=None, max_points_per_object=None):
    """labels [B,H,W] ints, xyz [B,3,H,W] float32, attrs [B,C,H,W] or None.
    Returns (records: list over frames of dict id -> record for every id with pixels > 0, points [P,3] float32,
    point_attr [P,C] float32 or None, pixel_index [P] int64, offsets dict (b, id) -> (offset, kept))."""
    labels = np.asarray(labels).astype(np.int64)
    B, H, W = labels.shape
    recs, pts_out, att_out, pix_out, offsets = [], [], [], [], {}
    total = 0
    for b in range(B):
        lab = labels[b].reshape(-1)
        X = np.asarray(xyz[b]).reshape(3, -1)
        finite = np.isfinite(X).all(axis=0) & (X[2] > 0)
        frame = {}
        for l in range(1, NUM_IDS):
            mask = lab == l
            pixels = int(mask.sum())
            if pixels == 0:
                offsets[(b, l)] = (total, 0)
                continue
            idx = np.nonzero(mask)[0]
            ys, xs = idx // W, idx % W
            vidx = np.nonzero(mask & finite)[0]
            r = object_record(X[:, vidx].T.astype(np.float64))
            r.update(pixels=pixels, count=len(vidx), box=np.array([xs.min(), ys.min(), xs.max(), ys.max()]))
            keep = vidx[subsample_ranks(len(vidx), max_points_per_object)]
            offsets[(b, l)] = (total, len(keep))
            total += len(keep)
            pts_out.append(X[:, keep].T)
            pix_out.append(keep)
            if attrs is not None:
                A = np.asarray(attrs[b]).reshape(np.asarray(attrs[b]).shape[0], -1)
                att_out.append(A[:, keep].T)
            frame[l] = r
        recs.append(frame)
    pts = np.concatenate(pts_out).astype(np.float32) if pts_out else np.zeros((0, 3), np.float32)
    pix = np.concatenate(pix_out) if pix_out else np.zeros((0,), np.int64)
    att = None
    if attrs is not None:
        C = np.asarray(attrs).shape[1]
        att = np.concatenate(att_out).astype(np.float32) if att_out else np.zeros((0, C), np.float32)
    return recs, pts, att, pix, offsets
