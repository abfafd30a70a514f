"""fit_plane GPU time (HIP events) at B = 1 and B = 12 frames, 480x640, num_hyp 256, on a tabletop scene of the test
generator (tests/support_reference.py), against the same step in numpy on the host (the reference restatement: integer
scoring of every hypothesis, fp64 refinement, per-object statistics) plus the copies a host version pays, and the split
per kernel class from the library's own profiler (uoc_prof_*).

    python scripts/plane_bench.py [--reps 1000] [--host-reps 3] [--frames 1 12] [--num-hyp 256] [--tau-mm 10]
                                  [--height-map] [--out result.json]

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

from tests import support_reference as R  # noqa: E402
from unseenobjectclustering_amd import _native  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def gpu_time(lab, xyz, reps, **kw):
    for _ in range(30):
        fit_plane(lab, xyz, **kw)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one fit, launch gaps included
        e0.record()
        fit_plane(lab, xyz, **kw)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def kernel_split(lab, xyz, reps, **kw):
    """us per call and kernel class, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        fit_plane(lab, xyz, **kw)
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith("plane_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--num-hyp", type=int, default=256)
    ap.add_argument("--tau-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--height-map", action="store_true")
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(num_hyp=args.num_hyp, tau=args.tau_mm / 1000.0, seed=args.seed, height_map=args.height_map)
    lab, xyz = R.tabletop(H, W, args.seed)
    res = {"size": f"{H}x{W}", "reps": args.reps, "num_hyp": args.num_hyp, "tau_mm": args.tau_mm, "height_map": args.height_map,
           "frame_ms": args.frame_ms}
    for B in args.frames:
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dx = torch.from_numpy(np.stack([xyz] * B)).to(dev)
        med, p10, p90 = gpu_time(dl, dx, args.reps, **kw)
        out = fit_plane(dl, dx, **kw)
        res[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                        "share_of_frame": med / B / (args.frame_ms * 1e3), "kernels_us": kernel_split(dl, dx, 200, **kw)}
        res["plane"] = {k: int(getattr(out, k)[0]) for k in ("found", "candidates", "inliers", "hyp")}
        print(f"B{B}", res[f"B{B}"], flush=True)
    if args.host_reps > 0:
        t = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = R.fit(lab, xyz, args.num_hyp, args.tau_mm, args.seed, height_map=args.height_map)
            t.append((time.perf_counter() - t0) * 1e3)
        assert {k: want["plane"][k] for k in res["plane"]} == res["plane"], (want["plane"], res["plane"])
        dl, dx = torch.from_numpy(lab).to(dev), torch.from_numpy(xyz).to(dev)
        t2 = []
        for _ in range(5):                 # what the host version pays on top: the map and the XYZ planes to the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dl.cpu().numpy()
            dx.cpu().numpy()
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
