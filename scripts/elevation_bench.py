"""heights GPU time (HIP events) at B = 1 and B = 12 frames, 480x640, G = 256, on a tabletop scene of the test generator
(tests/placement_reference.py) with the plane fitted and the placement stage run on the device, split over the two launch
groups by the library's own profiler (uoc_prof_*), against the same step in numpy on the host (the reference restatement)
plus the copies a host version pays; and the atomic traffic of the two point passes, counted by the reference: the
operations of the scene before and after the wave-level combining.

    python scripts/elevation_bench.py [--reps 1000] [--host-reps 5] [--frames 1 12] [--grid 256] [--cell-mm 10]
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

from tests import elevation_reference as R  # noqa: E402
from unseenobjectclustering_amd import _native  # noqa: E402
from unseenobjectclustering_amd.elevation import heights, on_top  # noqa: E402
from unseenobjectclustering_amd.placement import free_space  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def gpu_time(lab, xyz, placed, reps, **kw):
    for _ in range(30):
        heights(lab, xyz, placed, **kw)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        heights(lab, xyz, placed, **kw)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def kernel_split(lab, xyz, placed, reps, **kw):
    """us per call and launch group, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        heights(lab, xyz, placed, **kw)
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith("elevation_")}


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
    lab, xyz = R.tabletop(H, W, args.seed)
    res = {"size": f"{H}x{W}", "grid": G, "cell_mm": cell, "step_mm": 5, "min_pts": 2, "reps": args.reps, "frame_ms": args.frame_ms}
    for B in args.frames:
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dx = torch.from_numpy(np.stack([xyz] * B)).to(dev)
        placed = free_space(dl, dx, fit_plane(dl, dx), grid=G, cell=cell / 1000.0)
        queries = [on_top(placed, 0.03), on_top(placed, 0.03, id=1), on_top(placed, 0.05, id=0)]
        kw = dict(queries=queries)
        res["queries"] = len(queries)
        med, p10, p90 = gpu_time(dl, dx, placed, args.reps, **kw)
        out = heights(dl, dx, placed, **kw)
        res[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                        "share_of_frame": med / B / (args.frame_ms * 1e3), "kernels_us": kernel_split(dl, dx, placed, 200, **kw)}
        res["answers"] = out.answers[0].cpu().tolist()
        res["info"] = out.info[0].cpu().tolist()
        F, tau = placed.frame[0].cpu().numpy(), placed.tau_mm
        print(f"B{B}", res[f"B{B}"], flush=True)
    before, after = R.atomic_events(lab, xyz, F, G, cell, tau, 5, 256)      # 480x640: the vector-load path, 256 pixels per wave turn
    res["atomics"] = {"operations": before, "after_wave_combining": after,
                      "after_at_64_pixels": R.atomic_events(lab, xyz, F, G, cell, tau, 5, 64)[1]}
    if args.host_reps > 0:
        t = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = R.heights(lab, xyz, F, G, cell, tau, 5, 2, queries)
            t.append((time.perf_counter() - t0) * 1e3)
        assert want["answers"].tolist() == res["answers"], (want["answers"].tolist(), res["answers"])
        dl, dx = torch.from_numpy(lab).to(dev), torch.from_numpy(xyz).to(dev)
        t2 = []
        for _ in range(5):                 # what the host version pays on top: the map and the XYZ planes to the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dl.cpu().numpy()
            dx.cpu().numpy()
            t2.append((time.perf_counter() - t0) * 1e3)
        res.update(host_numpy_ms=float(np.median(t)), host_numpy_ms_min=float(min(t)), host_numpy_ms_max=float(max(t)),
                   host_copies_ms=float(np.median(t2)))
        if "B1" in res:
            res["host_over_gpu"] = res["host_numpy_ms"] * 1e3 / res["B1"]["gpu_us_median"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
