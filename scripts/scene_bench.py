"""scene.Memory.update GPU time (HIP events) at G = 256 with B = 1 and B = 12 frames and at G = 512 with B = 1, on a
480x640 tabletop scene of the test generator (tests/placement_reference.py): the placement stage runs on the device for
the scene and for the scene with an image band hidden, and the memory is updated with the two in turn (so that every call
keeps, flags and observes cells).  For scale: the same box's placement.free_space call on the same frames, and the numpy
reference's step (tests/scene_reference.py) on the same grids.

    python scripts/scene_bench.py [--reps 500] [--host-reps 3] [--cases 256:1 256:12 512:1] [--cell-mm 10]
                                  [--frame-ms 5.86] [--no-free-space] [--out result.json]

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

from tests import placement_reference as PR  # noqa: E402
from tests import scene_reference as R  # noqa: E402
from unseenobjectclustering_amd import placement, scene  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def gpu_time(fn, reps):
    for _ in range(10):
        fn(0), fn(1)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        fn(k & 1)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return {"gpu_us_median": float(np.median(per)), "gpu_us_p10": float(np.percentile(per, 10)), "gpu_us_p90": float(np.percentile(per, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=["256:1", "256:12", "512:1"], help="GRID:FRAMES to measure")
    ap.add_argument("--cell-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--queries", type=int, default=1, help="placement queries per call (0..16)")
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--no-free-space", action="store_true", help="do not time placement.free_space: for a kernel trace of the stage alone")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lab, xyz = PR.tabletop(H, W, args.seed)
    hidden = xyz.copy()
    hidden[:, 200:280, :] = 0.0
    res = {"size": f"{H}x{W}", "cell_mm": args.cell_mm, "reps": args.reps, "frame_ms": args.frame_ms, "queries": args.queries}
    for case in args.cases:
        G, B = (int(x) for x in case.split(":"))
        cell = args.cell_mm * 256 // G / 1000.0          # the same table on every grid
        qs = [(16, 0, 0, placement.WIDEST)] * args.queries
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dxs = [torch.from_numpy(np.stack([x] * B)).to(dev) for x in (xyz, hidden)]
        fitted = fit_plane(dl, dxs[0])
        placed = [placement.free_space(dl, dx, fitted, grid=G, cell=cell, queries=qs) for dx in dxs]
        mem = scene.Memory(G, max_age=30, streams=B, device=dev)
        name = f"G{G}_B{B}"
        res[name] = gpu_time(lambda k: mem.update(placed[k], queries=qs), args.reps)
        res[name]["gpu_us_per_frame"] = res[name]["gpu_us_median"] / B
        res[name]["share_of_frame"] = res[name]["gpu_us_median"] / B / (args.frame_ms * 1e3)
        if not args.no_free_space:
            res[name]["free_space"] = gpu_time(lambda k: placement.free_space(dl, dxs[k], fitted, grid=G, cell=cell, queries=qs), args.reps)
        mem.reset()
        outs = [mem.update(placed[k], queries=qs) for k in (0, 1)]
        res[name]["info"] = [o.info[0].cpu().tolist() for o in outs]
        print(name, res[name], flush=True)
        if args.host_reps > 0:             # the reference's step on stream 0's grids
            grids = [(p.state[:1].cpu().numpy(), p.owner[:1].cpu().numpy(), p.frame[:1].cpu().numpy()) for p in placed]
            st, t = R.new_state(1, G), []
            for k in range(2 + args.host_reps):
                s, o, fr = grids[k & 1]
                R._CLEARANCE.clear()
                t0 = time.perf_counter()
                want = R.step(st, s, o, fr, None, 30, 1, qs)
                t.append((time.perf_counter() - t0) * 1e3)
                if k < 2:
                    assert want["info"][0].tolist() == res[name]["info"][k], (want["info"][0].tolist(), res[name]["info"][k])
            res[name]["host_numpy_ms"] = {"median": float(np.median(t[2:])), "min": float(min(t[2:])), "max": float(max(t[2:]))}
            res[name]["host_over_gpu"] = res[name]["host_numpy_ms"]["median"] * 1e3 / res[name]["gpu_us_median"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
