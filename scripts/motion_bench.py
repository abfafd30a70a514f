"""motion.register GPU time (HIP events) at B = 1 and B = 12 frames, G = 256, on a 480x640 tabletop scene of the test
generator (tests/placement_reference.py) with the plane fitted and the placement stage run on the device for the scene
and for the scene with one object's points moved: one pair over 32 rotations and a radius of 8 cells, then 16 pairs over
64 rotations and a radius of 16; against the same step in numpy on the host (the reference restatement).

    python scripts/motion_bench.py [--reps 500] [--host-reps 1] [--frames 1 12] [--grid 256] [--cell-mm 10]
                                   [--frame-ms 5.86] [--case NAME] [--out result.json]

(the JSON result line is always printed; --out also writes it to a file)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import motion_reference as R  # noqa: E402
from tests import placement_reference as PR  # noqa: E402
from unseenobjectclustering_amd import motion, placement  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def gpu_time(before, after, pairs, angles, radius, reps):
    for _ in range(10):
        motion.register(before, after, pairs, angles=angles, radius=radius)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        motion.register(before, after, pairs, angles=angles, radius=radius)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cell-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--case", default=None, help="measure this case alone (one_pair_A32_R8 or pairs16_A64_R16): for a kernel trace")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, cell = args.grid, args.cell_mm
    lab, xyz = PR.tabletop(H, W, args.seed)
    res = {"size": f"{H}x{W}", "grid": G, "cell_mm": cell, "reps": args.reps, "frame_ms": args.frame_ms}

    def placements(B):
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dx = torch.from_numpy(np.stack([xyz] * B)).to(dev)
        fitted = fit_plane(dl, dx)
        before = placement.free_space(dl, dx, fitted, grid=G, cell=cell / 1000.0)
        cells = before.cells[0].cpu().numpy()
        ids = [int(i) for i in np.argsort(-cells[1:], kind="stable") + 1 if cells[i] > 0]
        _, _, u, v = placement.plane_axes(before.planes, 0)
        moved = xyz.copy()
        valid = (lab == ids[0]) & (xyz[2] > 0)
        moved[:, valid] += ((5 * cell / 1000.0 * u - 3 * cell / 1000.0 * v)[:, None]).astype(np.float32)      # 5 cells along u, 3 back along v
        after = placement.free_space(dl, torch.from_numpy(np.stack([moved] * B)).to(dev), fitted, grid=G, cell=cell / 1000.0)
        return before, after, ids, cells

    cases = {}
    for B in args.frames:
        before, after, ids, cells = placements(B)
        many = [(a, b) for a in ids for b in ids][:16]
        many = (many * 16)[:16]
        cases = {"one_pair_A32_R8": ([(ids[0], ids[0])], 32, 8, args.reps), "pairs16_A64_R16": (many, 64, 16, max(args.reps // 10, 10))}
        if args.case is not None:
            cases = {args.case: cases[args.case]}
        res["cells"] = {str(i): int(cells[i]) for i in ids}
        for name, (pairs, angles, radius, reps) in cases.items():
            med, p10, p90 = gpu_time(before, after, pairs, angles, radius, reps)
            out = motion.register(before, after, pairs, angles=angles, radius=radius)
            res[f"{name}_B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                                   "share_of_frame": med / B / (args.frame_ms * 1e3), "reps": reps}
            res.setdefault(f"{name}_best", out.best[0].cpu().tolist())       # every frame is a copy of the one scene
            assert out.best.cpu().tolist() == [res[f"{name}_best"]] * B
            print(f"{name}_B{B}", res[f"{name}_B{B}"], flush=True)
    # the host comparison: the one scene, B = 1
    if args.host_reps > 0:
        before, after, ids, _ = placements(1)
        grids = [getattr(p, k)[0].cpu().numpy() for p in (before, after) for k in ("state", "owner")]
        fr = before.frame[0].cpu().numpy()
        for name, (pairs, angles, radius, _) in cases.items():
            if len(pairs) == 1:            # the whole step, as the tests run it
                t = []
                for _ in range(args.host_reps):
                    t0 = time.perf_counter()
                    want = R.motion(*grids, R.rotation_table(angles), radius, pairs, fr, fr)
                    t.append((time.perf_counter() - t0) * 1e3)
                assert want["best"].tolist() == res[f"{name}_best"], (want["best"].tolist(), res[f"{name}_best"])
                res[f"{name}_host_numpy_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
            else:                          # minutes on a host: one rotation of every pair, times the rotations
                table, t = R.rotation_table(angles), 0.0
                for a, b in pairs:
                    ca, cb = R.cells_of(grids[0], grids[1], a), R.cells_of(grids[2], grids[3], b)
                    ma, mb = (grids[0] == 2) & (grids[1] == a), (grids[2] == 2) & (grids[3] == b)
                    t0 = time.perf_counter()
                    R.costs(ca, cb, ma, mb, R.pivot(ca), R.pivot(cb), int(table[1, 0]), int(table[1, 1]), radius)
                    t += (time.perf_counter() - t0) * 1e3
                res[f"{name}_host_numpy_ms"] = {"median": t * angles, "estimated_from": "one rotation of every pair, times the rotations"}
            if f"{name}_B1" in res:
                res[f"{name}_host_over_gpu"] = res[f"{name}_host_numpy_ms"]["median"] * 1e3 / res[f"{name}_B1"]["gpu_us_median"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
