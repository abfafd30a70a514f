"""fp64 numpy restatement of the label-confidence stage (include/uoc_hip.h): test infrastructure.

assign(): d = 0.5 (1 - X Z^T) in float64, best = argmin (ties to the lowest seed), rival = argmin over the seeds of another
label (ties to the lowest seed, -1 without one), margin = d[rival] - d[best] (1.0 without a rival), the "largest cluster
becomes label 0" swap on labels and second.  paste() and objects() are exact integer restatements of uoc_conf_paste and
uoc_conf_objects.

Tolerance of the margin (derived): with unit rows and C channels an fp32 dot product is within C * 2^-24 of the exact one,
d adds two roundings, the margin is a difference of two per-component minima (each 1-Lipschitz in d) plus one rounding:
|margin_gpu - margin_fp64| <= (C + 4) * 2^-24, across a flip of the argmin too (the margin is continuous there).  TOL
doubles it for seeds normalised in fp32 and the unspecified internal rounding of the MFMA."""
import numpy as np

ONE = 65536


def tol(channels):
    return 2.0 * (channels + 4) * 2.0 ** -24


def flat(X):
    """[n,64] or the planes [2,n,64] -> [n,C] float64."""
    X = np.asarray(X, np.float64)
    return X if X.ndim == 2 else np.concatenate(list(X), axis=1)


def swap_label(seed_labels_hit, num_unique):
    """The label that changes places with 0: counts over the labels in range(num_unique) only, first maximum wins."""
    num = min(int(num_unique), 128)
    if num <= 0:
        return 0
    counts = np.bincount(seed_labels_hit[(seed_labels_hit >= 0) & (seed_labels_hit < num)], minlength=num)[:num]
    return int(np.argmax(counts))


def apply_swap(lab, big):
    out = lab.copy()
    if big != 0:
        out[lab == 0] = big
        out[lab == big] = 0
    return out


def assign(X, Z, seed_labels, num_unique=None):
    """One field.  Returns dict(labels, margin, second, closest, rival, gap23): gap23 = the fp64 gap between the second and
    the third per-label minimum (inf with fewer than three labels), what `second` hinges on."""
    X, Z = flat(X), flat(Z)
    sl = np.asarray(seed_labels, np.int64)
    if num_unique is None:
        num_unique = len(np.unique(sl))
    d = 0.5 * (1.0 - X @ Z.T)                                    # [n, m]
    n = d.shape[0]
    best = np.argmin(d, axis=1)                                  # first minimum
    c1 = sl[best]
    other = sl[None, :] != c1[:, None]
    has = other.any(axis=1)
    dm = np.where(other, d, np.inf)
    rival = np.where(has, np.argmin(dm, axis=1), -1)
    rows = np.arange(n)
    margin = np.where(has, dm[rows, np.maximum(rival, 0)] - d[rows, best], 1.0)
    labs = np.unique(sl)
    per = np.stack([d[:, sl == l].min(axis=1) for l in labs], axis=1)
    per.sort(axis=1)
    gap23 = per[:, 2] - per[:, 1] if per.shape[1] >= 3 else np.full(n, np.inf)
    big = swap_label(c1, num_unique)
    second = np.where(has, apply_swap(np.where(has, sl[np.maximum(rival, 0)], 0), big), -1)
    return dict(labels=apply_swap(c1, big).astype(np.int32), margin=margin, second=second.astype(np.int32),
                closest=best.astype(np.int32), rival=rival.astype(np.int32), gap23=gap23)


def src_index(c, S, length):
    """Nearest-resize source index of frame offset c in a crop of S over `length` frame pixels: float32 operations as on the
    device (floor(c * (S / length)), clamped)."""
    scale = np.float32(S) / np.float32(length)
    return np.minimum(np.floor(np.asarray(c, np.float32) * scale).astype(np.int64), S - 1)


def paste_source(labels_crop, boxes, plan, K, S, H, W):
    """Per frame pixel the (k, crop index) that paints it along the plan (order [K] then map [K,128]), (-1, -1) where nothing
    does, and the painted id (0 there): later ROIs of the order overwrite earlier ones."""
    order, idmap = np.asarray(plan[:K]), np.asarray(plan[K:K + K * 128]).reshape(K, 128)
    lab = np.asarray(labels_crop).reshape(K, S * S)
    src_k = np.full((H, W), -1, np.int64)
    src_i = np.full((H, W), -1, np.int64)
    ident = np.zeros((H, W), np.int32)
    for k in order:
        x0, y0, x1, y1 = [int(v) for v in boxes[k]]
        sy = src_index(np.arange(y1 - y0 + 1), S, y1 - y0 + 1)
        sx = src_index(np.arange(x1 - x0 + 1), S, x1 - x0 + 1)
        idx = sy[:, None] * S + sx[None, :]
        l = lab[k][idx]
        ok = (l >= 0) & (l < 128)
        v = np.where(ok, idmap[k][np.clip(l, 0, 127)], 0)
        hit = v != 0
        win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        src_k[win] = np.where(hit, k, src_k[win])
        src_i[win] = np.where(hit, idx, src_i[win])
        ident[win] = np.where(hit, v, ident[win])
    return src_k, src_i, ident


def paste(values_crop, labels_crop, boxes, plan, K, S, H, W, out):
    """uoc_conf_paste on a copy of `out` [H,W]."""
    src_k, src_i, _ = paste_source(labels_crop, boxes, plan, K, S, H, W)
    vals = np.asarray(values_crop).reshape(K, S * S)
    res = np.array(out, copy=True)
    hit = src_k >= 0
    res[hit] = vals[src_k[hit], src_i[hit]]
    return res


def quantise(conf):
    c = np.asarray(conf, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~(c >= 0)
        prod = np.where(bad | (c >= 1), np.float32(0), c) * np.float32(ONE)      # exact: a power of two
        q = np.where(c >= 1, ONE - 1, prod.astype(np.int64))
    return np.where(bad, 0, q).astype(np.int64)


def objects(labels, conf, weak_q):
    """uoc_conf_objects: [B,128,4] int64."""
    labels, q = np.asarray(labels), quantise(conf)
    B = labels.shape[0]
    out = np.zeros((B, 128, 4), np.int64)
    for b in range(B):
        l, qq = labels[b].reshape(-1), q[b].reshape(-1)
        for i in range(128):
            sel = qq[l == i]
            if sel.size:
                out[b, i] = (sel.size, sel.sum(), sel.min(), int((sel < weak_q).sum()))
    return out


def final_margin(refined, labels1, margin1, pasted):
    """The three-case rule of the final map: refined != 0 -> the pasted crop margin; refined == 0 and (filtered) stage-1
    label 0 -> the stage-1 margin; refined == 0 and stage-1 label != 0 -> 0.0."""
    return np.where(refined != 0, pasted, np.where(labels1 == 0, margin1, np.float32(0))).astype(np.float32)
