"""grasp.candidates GPU time (HIP events) at B = 1 and B = 12 frames, 480x640, G = 256, default parameters, on a tabletop
scene of the placement test generator (tests/placement_reference.py) with the plane fitted and the grid rasterised on the
device, split over the two launch groups by the library's own profiler (uoc_prof_*), against the same step in numpy on
the host (the reference restatement, tests/grasp_reference.py) plus the read-back of the two grids a host version pays.

    python scripts/grasp_bench.py [--reps 1000] [--host-reps 5] [--frames 1 12] [--grid 256] [--cell-mm 10]
                                  [--frame-ms 5.86] [--limits] [--out result.json]

--limits measures the largest configuration instead of the default one: 32 directions, 8 offsets, and at 10 mm cells an
opening of 64, a gap of 4, fingers of 8 and a pad half-length of 4 cells (six chunks of directions in candidate_kernel).

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

from tests import grasp_reference as GR  # noqa: E402
from tests import placement_reference as PR  # noqa: E402
from unseenobjectclustering_amd import _native  # noqa: E402
from unseenobjectclustering_amd.grasp import candidates  # noqa: E402
from unseenobjectclustering_amd.placement import free_space  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it
LIMITS = dict(angles=32, offsets=8, max_open=0.64, gap=0.04, finger=0.08, pad=0.08)     # in cells of 10 mm: 64, 4, 8, 4


def gpu_time(placed, reps, kw):
    for _ in range(30):
        candidates(placed, **kw)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        candidates(placed, **kw)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def kernel_split(placed, reps, kw):
    """us per call and launch group, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        candidates(placed, **kw)
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith("grasp_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cell-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--limits", action="store_true", help="the largest configuration instead of the default one")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, cell = args.grid, args.cell_mm
    kw = {k: (v if isinstance(v, int) else v * cell / 10) for k, v in LIMITS.items()} if args.limits else {}
    lab, xyz = PR.tabletop(H, W, args.seed)
    res = {"size": f"{H}x{W}", "grid": G, "cell_mm": cell, "reps": args.reps, "frame_ms": args.frame_ms}
    for B in args.frames:
        dl = torch.from_numpy(np.stack([lab] * B)).to(dev)
        dx = torch.from_numpy(np.stack([xyz] * B)).to(dev)
        placed = free_space(dl, dx, fit_plane(dl, dx), grid=G, cell=cell / 1000.0)
        med, p10, p90 = gpu_time(placed, args.reps, kw)
        out = candidates(placed, **kw)
        res[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                        "share_of_frame": med / B / (args.frame_ms * 1e3), "kernels_us": kernel_split(placed, 200, kw)}
        print(f"B{B}", res[f"B{B}"], flush=True)
    st, ow = placed.state[0].cpu().numpy(), placed.owner[0].cpu().numpy()
    best = out.best[0].cpu().numpy()
    cfg = dict(M=out.offsets, Wmax=out.max_open, gap=out.gap, F=out.finger, Hp=out.pad, unknown_blocks=int(out.unknown_blocks))
    res.update(params={"A": out.angles, **cfg}, objects=int((best[:, 5] > 0).sum()), graspable=int(best[:, 0].sum()),
               candidates_ok=int(best[:, 7].sum()))
    if args.host_reps > 0:
        t = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = GR.grasp(st, ow, GR.direction_table(out.angles), **cfg)
            t.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(want["best"], best) and np.array_equal(want["cand"], out.cand[0].cpu().numpy())
        t2 = []
        for _ in range(5):                 # what the host version pays on top: the two grids to the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            placed.state[0].cpu().numpy()
            placed.owner[0].cpu().numpy()
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
