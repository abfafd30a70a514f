"""Prints the tables of profiles/stats_error.md: for the engineered cases of tests/stats_cases.py and the seeded scenes, per
field of the gap-independent checker the derived bound, how much of it the float64 reference uses once rounded to float32
(CPU) and how much the kernels use (GPU; measured and written down, never fed back into a bound), the same for the
comparison of the step C and D sums with the reference (`ref.` rows), and per mutant the smallest miss over the cases
that must reject it.  Without a GPU the kernel columns stay empty.

    python scripts/stats_error.py [--out table.md]
"""
import argparse
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import objects_reference as OR  # noqa: E402
from tests import stats_cases as S  # noqa: E402
from tests import support_reference as R  # noqa: E402

OBJECT_KEYS = ("centroid", "cov", "eig", "axes", "obb_half", "obb_center")
PLANE_OBJECT_KEYS = ("height_min", "height_max", "foot", "cov2", "axis", "half", "center")


def rounded(rec, keys):
    return {k: np.asarray(rec[k], np.float64).astype(np.float32) for k in keys}


class Table:
    """(scene, field) -> [smallest bound, largest bound, largest reference value / bound, largest kernel value / bound]."""

    def __init__(self):
        self.rows = {}

    def add(self, scene, metrics, column):
        for name, value, bound in metrics:
            row = self.rows.setdefault((scene, name), [math.inf, 0.0, 0.0, None])
            ratio = value / bound if bound > 0 else (math.inf if value > 0 else 0.0)
            row[0], row[1] = min(row[0], bound), max(row[1], bound)
            row[column] = ratio if row[column] is None else max(row[column], ratio)

    def lines(self):
        out = ["| scene | field | bound (smallest .. largest) | reference / bound | kernel / bound |", "|---|---|---|---|---|"]
        for (scene, name), (lo, hi, ref, ker) in self.rows.items():
            out.append("| %s | %s | %.2e .. %.2e | %.2f | %s |" % (scene, name, lo, hi, ref, "-" if ker is None else "%.2f" % ker))
        return out


def to_dev(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def object_scene(table, scene, lab, xyz, dev):
    recs = OR.extract(lab, xyz)[0]
    kernel = None
    if dev is not None:
        from unseenobjectclustering_amd import objects as O
        objs = O.extract_objects(*to_dev(dev, lab, xyz), min_points=0)
        f = {k: getattr(objs, k).cpu().numpy() for k in ("centroid", "cov", "eigenvalues", "axes", "obb_half", "obb_center")}
        keys = list(zip(objs.frame.cpu().tolist(), objs.label.cpu().tolist()))
        kernel = {key: dict({k: f[k][i] for k in f}, eig=f["eigenvalues"][i]) for i, key in enumerate(keys)}
    for b, frame in enumerate(recs):
        for l, r in frame.items():
            if r["count"] >= 1:
                table.add(scene, S.object_metrics(rounded(r, OBJECT_KEYS), r["points"], r), 2)
                if kernel is not None:
                    table.add(scene, S.object_metrics(kernel[(b, l)], r["points"], r), 3)


def plane_scene(table, scene, lab, xyz, num_hyp, tau_mm, seed, dev):
    ref = R.fit(lab, xyz, num_hyp, tau_mm, seed, height_map=True)
    p = ref["plane"]
    if not p["found"]:
        return
    valid = ~np.isnan(ref["height"]).reshape(-1)
    sources = [(2, rounded(p, S.PLANE_EXACT), {l: rounded(o, PLANE_OBJECT_KEYS) for l, o in ref["objects"].items()},
                ref["height"].reshape(-1).astype(np.float32))]
    if dev is not None:
        from unseenobjectclustering_amd import support
        res = support.fit_plane(*to_dev(dev, lab, xyz), num_hyp=num_hyp, tau=tau_mm / 1000.0, seed=seed, height_map=True)
        got = {k: getattr(res, k)[0].cpu().numpy() for k in support.PLANE_FIELDS + support.OBJECT_FIELDS}
        sources.append((3, got, {l: {k: got[k][l] for k in PLANE_OBJECT_KEYS} for l in ref["objects"]},
                        res.height[0].cpu().numpy().reshape(-1)))
    for column, plane, objects, height in sources:
        full = dict(plane, height=height.reshape(ref["height"].shape))
        for k in PLANE_OBJECT_KEYS:                                     # the [128, ...] layout of the GPU result
            full[k] = {l: o[k] for l, o in objects.items()}
        table.add(scene, [(re.sub(r"^ref\.\d+\.", "ref.object.", n), v, b) for n, v, b in S.plane_reference_metrics(full, ref)], column)
        table.add(scene, [("plane." + n, v, b) for n, v, b in S.plane_metrics(plane, p["points"], p)], column)
        table.add(scene, [("plane." + n, v, b) for n, v, b in S.height_metrics(height[valid], plane, ref["xyz"].T[valid])], column)
        for l, o in ref["objects"].items():
            table.add(scene, [("object." + n, v, b) for n, v, b in S.plane_object_metrics(objects[l], plane, o["points"])], column)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0") if torch.cuda.is_available() else None
    table = Table()
    for group in S.object_groups():
        lab, xyz, _ = S.object_group_frames(group)
        object_scene(table, "cases " + group, lab, xyz, dev)
    from tests.test_objects_gpu import synthetic
    for H, W, ids in ((7, 13, "all"), (24, 32, "all"), (48, 64, "gaps"), (480, 640, "all")):
        lab, xyz, _ = synthetic(2, H, W, seed=H * 7 + W, ids=ids)
        object_scene(table, "seeded %dx%d" % (H, W), lab, xyz, dev)
    for name in S.PLANE_NAMES:
        for tiny in (False, True):
            for placement in S.PLACEMENTS:
                lab, xyz = S.plane_scene_frame(name, tiny, placement)
                plane_scene(table, "plane " + name, lab, xyz, 16, 10, 1, dev)
    for H, W, seed, tau_mm, num_hyp in ((24, 32, 1, 10, 64), (61, 83, 1, 10, 64), (61, 83, 2, 3, 256)):
        lab, xyz = R.tabletop(H, W, seed, noise=0.0015 if tau_mm == 3 else 0.0005)
        plane_scene(table, "tabletop %dx%d" % (H, W), lab, xyz, num_hyp, tau_mm, seed, dev)
    lines = ["kernel columns: %s" % ("measured on " + torch.cuda.get_device_name(0) if dev is not None else "no GPU, not measured"), ""]
    lines += table.lines()
    worst = {c: max(((r[c], k) for k, r in table.rows.items() if r[c] is not None), default=(0.0, None)) for c in (2, 3)}
    lines += ["", "largest reference / bound %.2f %s; largest kernel / bound %s" % (
        worst[2][0], worst[2][1], "-" if worst[3][1] is None else "%.2f %s" % worst[3]), ""]
    lines += ["| mutant | cases | rejected by the exact comparison | smallest checker miss (x bound) |", "|---|---|---|---|"]
    rows = S.mutant_rows()
    for mutant in S.MUTANT_CASES:
        mine = [r for r in rows if r[0] == mutant]
        lines.append("| %s | %s | %d of %d | %.3g |" % (mutant, ", ".join("%s%s" % (r[1], " (translated)" if r[2] else "") for r in mine),
                                                     sum(r[3] for r in mine), len(mine), min(r[4] for r in mine)))
    lab, xyz, _ = synthetic(2, 24, 32, seed=24 * 7 + 32)
    sets = {(b, l): r["points"].astype(np.float32) for b, frame in enumerate(OR.extract(lab, xyz)[0]) for l, r in frame.items()
            if r["count"] >= 3}
    flipped = [r for r in S.sign_rule_rows(sets) if r[1]]
    lines.append("| no_sign_rule | %d seeded 24x32 objects whose axes it changes | - | %.3g |" % (len(flipped), min(r[2] for r in flipped)))
    for mutant, exact, ratio, metric in S.plane_mutant_rows()[1:]:
        lines.append("| %s (step D) | the 4096-point plate of the frontal scene | %d of 1 | %.3g (%s) |" % (mutant, exact, ratio, metric))
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
