"""footprint.fit GPU time (HIP events) at B = 1 and B = 12 frames, G = 256, on a 480x640 tabletop scene of the test
generator (tests/placement_reference.py) with the plane fitted and the placement stage run on the device: one
conservative 30 cm x 6 cm rectangle over 16 orientations, then 8 rectangles at the half-extent limit over 32; split over
the two launch groups by the library's own profiler (uoc_prof_*) in a pass of its own; against the same step in numpy on
the host (the reference restatement) plus the copies a host version pays.

    python scripts/footprint_bench.py [--reps 1000] [--host-reps 5] [--frames 1 12] [--grid 256] [--cell-mm 10]
                                      [--frame-ms 5.86] [--out result.json]

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

from tests import footprint_reference as R  # noqa: E402
from tests import placement_reference as PR  # noqa: E402
from unseenobjectclustering_amd import _native, footprint  # noqa: E402
from unseenobjectclustering_amd.placement import free_space  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it
LIMIT = [(16384, 0), (0, 16384), (11585, 11585), (16383, 1), (14000, 8000), (8000, 14000), (12000, 11000), (16000, 3000)]


def gpu_time(placed, rects, angles, reps):
    for _ in range(30):
        footprint.fit(placed, rects, angles=angles)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        footprint.fit(placed, rects, angles=angles)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def kernel_split(placed, rects, angles, reps):
    """us per call and launch group, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        footprint.fit(placed, rects, angles=angles)
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith("footprint_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cell-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, cell = args.grid, args.cell_mm
    lab, xyz = PR.tabletop(H, W, args.seed)
    cases = {"box_30x6_A16": ([footprint.rect(0.30, 0.06, cell)], 16),
             "limit_F8_A32": ([R.record(HL, HW, ignore=f % 3, mode=f % 2, ai=G // 2, aj=G // 2) for f, (HL, HW) in enumerate(LIMIT)], 32)}
    res = {"size": f"{H}x{W}", "grid": G, "cell_mm": cell, "reps": args.reps, "frame_ms": args.frame_ms}
    for B in args.frames:
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dx = torch.from_numpy(np.stack([xyz] * B)).to(dev)
        placed = free_space(dl, dx, fit_plane(dl, dx), grid=G, cell=cell / 1000.0)
        for name, (rects, angles) in cases.items():
            med, p10, p90 = gpu_time(placed, rects, angles, args.reps)
            out = footprint.fit(placed, rects, angles=angles)
            res[f"{name}_B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                                   "share_of_frame": med / B / (args.frame_ms * 1e3), "kernels_us": kernel_split(placed, rects, angles, 200)}
            res.setdefault(f"{name}_best", out.best[0].cpu().tolist())       # every frame is a copy of the one scene
            assert out.best.cpu().tolist() == [res[f"{name}_best"]] * B
            print(f"{name}_B{B}", res[f"{name}_B{B}"], flush=True)
    # the host comparison: the one scene, B = 1, taken once
    dl, dx = torch.from_numpy(lab[None]).to(dev), torch.from_numpy(xyz[None]).to(dev)
    placed = free_space(dl, dx, fit_plane(dl, dx), grid=G, cell=cell / 1000.0)
    st, ow, d2, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "dist2", "frame"))
    res["free_cells"] = int((st == 1).sum())
    if args.host_reps > 0:
        for name, (rects, angles) in cases.items():
            t = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                want = R.footprint(st, ow, d2, R.direction_table(angles), rects, 1, fr)
                t.append((time.perf_counter() - t0) * 1e3)
            assert want["best"].tolist() == res[f"{name}_best"], (want["best"].tolist(), res[f"{name}_best"])
            res[f"{name}_host_numpy_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
            if f"{name}_B1" in res:
                res[f"{name}_host_over_gpu"] = float(np.median(t)) * 1e3 / res[f"{name}_B1"]["gpu_us_median"]
        t2 = []
        for _ in range(5):                 # what the host version pays on top: the three grids to the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in ("state", "owner", "dist2"):
                getattr(placed, k)[0].cpu().numpy()
            t2.append((time.perf_counter() - t0) * 1e3)
        res["host_copies_ms"] = float(np.median(t2))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
