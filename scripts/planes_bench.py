"""fit_planes GPU time (HIP events) at B = 1 and B = 12 frames, 480x640, num_hyp 256, K = 1, 2, 4, on the `shelves`
scene of the test generator (tests/planes_reference.py: table, shelf board, side wall), with fit_plane in the same process
as the yardstick, and the split per launch group from the library's own profiler (uoc_prof_*).

    python scripts/planes_bench.py [--reps 500] [--frames 1 12] [--planes 1 2 4] [--num-hyp 256] [--tau-mm 10] [--out result.json]

(the JSON result line is always printed; --out also writes it to a file)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import planes_reference as P  # noqa: E402
from unseenobjectclustering_amd import _native  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane, fit_planes  # noqa: E402

H, W = 480, 640


def gpu_time(call, reps):
    for _ in range(30):
        call()
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one fit, launch gaps included
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return {"gpu_us_median": float(np.median(per)), "gpu_us_p10": float(np.percentile(per, 10)),
            "gpu_us_p90": float(np.percentile(per, 90))}


def kernel_split(call, reps, prefix):
    """us per call and launch group, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith(prefix)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 2, 4], help="max_planes to measure")
    ap.add_argument("--num-hyp", type=int, default=256)
    ap.add_argument("--tau-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(num_hyp=args.num_hyp, tau=args.tau_mm / 1000.0, seed=args.seed)
    res = {"size": f"{H}x{W}", "reps": args.reps, "num_hyp": args.num_hyp, "tau_mm": args.tau_mm, "rem_mm": 2 * args.tau_mm}
    for B in args.frames:
        frames = [P.shelves(H, W, s + 1)[:2] for s in range(B)]
        dl = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        dx = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
        row = {"fit_plane": gpu_time(lambda: fit_plane(dl, dx, **kw), args.reps)}
        row["fit_plane"]["groups_us"] = kernel_split(lambda: fit_plane(dl, dx, **kw), 200, "plane_")
        one = fit_plane(dl, dx, **kw)
        for K in args.planes:
            call = lambda: fit_planes(dl, dx, max_planes=K, **kw)      # noqa: E731
            out = fit_planes(dl, dx, max_planes=K, **kw)
            assert torch.equal(out.records[:, 0], one.records)          # the anchor, before anything is timed
            row[f"K{K}"] = gpu_time(call, args.reps)
            row[f"K{K}"]["groups_us"] = kernel_split(call, 200, "planes_")
            row[f"K{K}"]["no_objects"] = gpu_time(lambda: fit_planes(dl, dx, max_planes=K, objects=False, **kw), args.reps)
            row[f"K{K}"]["count"] = out.count.cpu().tolist()
            row[f"K{K}"]["round_candidates"] = out.round_candidates[0].cpu().tolist()
            row[f"K{K}"]["removed"] = out.removed[0].cpu().tolist()
        res[f"B{B}"] = row
        print(f"B{B}", json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
