"""relate GPU time (HIP events) at B = 1 and B = 12 frames, 480x640, on a tabletop scene of the test generator
(tests/relations_reference.py), against the same step in numpy on the host (the reference restatement: shifted-array
pair tables, then loops over the ids) plus the copies a host version pays, and the split per launch group from the
library's own profiler (uoc_prof_*).

    python scripts/relations_bench.py [--reps 1000] [--host-reps 5] [--frames 1 12] [--connectivity 8] [--gap-mm 15]
                                      [--min-pairs 8] [--frame-ms 5.86] [--out result.json]

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

from tests import relations_reference as R  # noqa: E402
from unseenobjectclustering_amd import _native  # noqa: E402
from unseenobjectclustering_amd.relations import relate  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def gpu_time(lab, xyz, reps, **kw):
    for _ in range(30):
        relate(lab, xyz, **kw)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        relate(lab, xyz, **kw)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def kernel_split(lab, xyz, reps, **kw):
    """us per call and launch group, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        relate(lab, xyz, **kw)
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith("relations_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--gap-mm", type=int, default=15)
    ap.add_argument("--min-pairs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", choices=["tabletop", "checkerboard"], default="tabletop")
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(connectivity=args.connectivity, gap=args.gap_mm / 1000.0, min_pairs=args.min_pairs)
    lab, xyz = R.tabletop(H, W, args.seed) if args.scene == "tabletop" else R.checkerboard(H, W)
    res = {"size": f"{H}x{W}", "scene": args.scene, "reps": args.reps, "connectivity": args.connectivity, "gap_mm": args.gap_mm,
           "min_pairs": args.min_pairs, "frame_ms": args.frame_ms}
    for B in args.frames:
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dx = torch.from_numpy(np.stack([xyz] * B)).to(dev)
        med, p10, p90 = gpu_time(dl, dx, args.reps, **kw)
        out = relate(dl, dx, **kw)
        res[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                        "share_of_frame": med / B / (args.frame_ms * 1e3), "kernels_us": kernel_split(dl, dx, 200, **kw)}
        res["layers"] = out.layer[0].cpu().tolist()
        print(f"B{B}", res[f"B{B}"], flush=True)
    if args.host_reps > 0:
        t = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = R.relations(lab, xyz[2], args.connectivity, args.gap_mm, args.min_pairs)
            t.append((time.perf_counter() - t0) * 1e3)
        assert want["layer"].tolist() == res["layers"], (want["layer"].tolist(), res["layers"])
        dl, dx = torch.from_numpy(lab).to(dev), torch.from_numpy(xyz).to(dev)
        t2 = []
        for _ in range(5):                 # what the host version pays on top: the map and the z plane to the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dl.cpu().numpy()
            dx[2].cpu().numpy()
            t2.append((time.perf_counter() - t0) * 1e3)
        res.update(host_numpy_ms=float(np.median(t)), host_copies_ms=float(np.median(t2)))
        if "B1" in res:
            res["host_over_gpu"] = res["host_numpy_ms"] * 1e3 / res["B1"]["gpu_us_median"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
