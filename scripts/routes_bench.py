"""routes.plan GPU time (HIP events) at B = 1 and B = 12 frames, G = 256, on a 480x640 tabletop scene of the test generator
(tests/placement_reference.py) with the plane fitted and the placement stage run on the device: one query (a 3 cm disc
from the middle of the free space to the reachable cell that costs the most) and eight (four radii, with and without an
ignored object, one without a target), then the G = 256 serpentine of the tests as the worst case; split over the two launch groups by the library's own profiler (uoc_prof_*) in
a pass of its own; the relaxation sweeps each case took (the workspace's diagnostic words); against the same step on the
host (the heap Dijkstra of the reference restatement) plus the copies a host version pays.

    python scripts/routes_bench.py [--reps 1000] [--host-reps 3] [--frames 1 12] [--grid 256] [--cell-mm 10]
                                   [--frame-ms 5.86] [--out result.json]

(the JSON result line is always printed; --out also writes it to a file.  UOC_LIB_PATH selects another build of the
library: the A/B of where the field lives runs this script on two builds in turn.)
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
from tests import routes_reference as R  # noqa: E402
from unseenobjectclustering_amd import _native, routes  # noqa: E402
from unseenobjectclustering_amd.placement import free_space, need2  # noqa: E402
from unseenobjectclustering_amd.support import fit_plane  # noqa: E402

H, W = 480, 640
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def gpu_time(call, reps):
    for _ in range(30):
        call()
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one call, launch gaps included
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def kernel_split(call, reps):
    """us per call and launch group, from the events the library records around its launch groups."""
    _native.prof_enable(True)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / r["launches"], 2) for r in rep if r["kernel"].startswith("routes_")}


def sweeps_of(state, owner, frame, queries, ub):
    """The relaxation sweeps per (frame, query): the first B*Q int32 words of the workspace after a call."""
    cost, info, path, ws = routes._call(state, owner, frame, queries, ub, 1024)
    B, Q = int(info.shape[0]), int(info.shape[1])
    return ws[:4 * B * Q].view(torch.int32).reshape(B, Q).cpu().tolist()


def measure(res, name, state, owner, frame, queries, ub, reps, frame_ms):
    call = lambda: routes.routes_records(state, owner, frame, queries, ub, 1024)      # noqa: E731
    med, p10, p90 = gpu_time(call, reps)
    B = int(state.shape[0])
    res[name] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                 "share_of_frame": med / B / (frame_ms * 1e3), "kernels_us": kernel_split(call, min(reps, 200)),
                 "sweeps": sweeps_of(state, owner, frame, queries, ub)[0]}
    print(name, res[name], flush=True)
    return call()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cell-mm", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--serpentine-reps", type=int, default=50)
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    G, cell = args.grid, args.cell_mm
    lab, xyz = PR.tabletop(H, W, args.seed)
    res = {"size": f"{H}x{W}", "grid": G, "cell_mm": cell, "reps": args.reps, "frame_ms": args.frame_ms,
           "library": os.path.basename(_native.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    dl, dx = torch.from_numpy(lab[None]).to(dev), torch.from_numpy(xyz[None]).to(dev)
    placed = free_space(dl, dx, fit_plane(dl, dx), grid=G, cell=cell / 1000.0)
    st, ow, d2, fr = (getattr(placed, k)[0].cpu().numpy() for k in ("state", "owner", "dist2", "frame"))
    n2 = need2(0.03, cell / 1000.0)
    room = np.argwhere((st == 1) & (d2 >= n2))                  # where the 3 cm disc fits
    src = tuple(int(x) for x in room[len(room) // 2])
    field = routes.plan(placed, [routes.query(0.03, src, None, cell)]).cost[0, 0].cpu().numpy()
    assert (field >= 0).sum() > len(room) // 2, "the source lies in a pocket"
    far = np.argwhere(field == field.max())[0]                  # the target: the reached cell that costs the most
    dst = tuple(int(x) for x in far)
    ids = [int(a) for a in np.unique(ow[st == 2]) if a >= 1][:2] or [1, 2]
    one = [routes.query(0.03, src, dst, cell)]
    half = np.argwhere((field >= field.max() // 2) & (field >= 0))[0]
    mid = tuple(int(x) for x in half)
    eight = one + [routes.query(0.0, src, dst, cell), routes.query(0.02, mid, dst, cell), routes.query(0.05, mid, src, cell),
                   routes.query(0.03, mid, None, cell), routes.query(0.03, dst, src, cell, ignore=ids[0]),
                   routes.query(0.02, src, mid, cell, ignore=ids[-1]), routes.query(0.03, dst, mid, cell)]
    res.update(free_cells=int((st == 1).sum()), source=src, target=dst)
    cases = {"one_query": one, "eight_queries": eight}
    for B in args.frames:
        pb = free_space(dl.expand(B, -1, -1).contiguous(), dx.expand(B, -1, -1, -1).contiguous(),
                        fit_plane(dl.expand(B, -1, -1).contiguous(), dx.expand(B, -1, -1, -1).contiguous()), grid=G, cell=cell / 1000.0)
        for name, queries in cases.items():
            cost, info, path = measure(res, f"{name}_B{B}", pb.state, pb.owner, pb.frame, queries, True, args.reps, args.frame_ms)
            res.setdefault(f"{name}_info", info[0].cpu().tolist())          # every frame is a copy of the one scene
            assert info.cpu().tolist() == [res[f"{name}_info"]] * B
    # the worst case: the serpentine of the tests, costs above 65535
    sst, sow = (torch.from_numpy(a[None]).to(dev) for a in R.serpentine(G))
    snake = [R.record(0, (0, 0), R.serpentine_end(G)[0])]
    cost, info, path = measure(res, "serpentine_B1", sst, sow, None, snake, True, args.serpentine_reps, args.frame_ms)
    res["serpentine_info"] = info[0].cpu().tolist()
    # the host comparison: the one scene, B = 1
    if args.host_reps > 0:
        for name, queries in cases.items():
            t = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                want = R.routes(st, ow, [tuple(q) for q in queries], 1, 1024, fr)
                t.append((time.perf_counter() - t0) * 1e3)
            assert want["info"].tolist() == res[f"{name}_info"], (want["info"].tolist(), res[f"{name}_info"])
            res[f"{name}_host_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
            if f"{name}_B1" in res:
                res[f"{name}_host_over_gpu"] = float(np.median(t)) * 1e3 / res[f"{name}_B1"]["gpu_us_median"]
        t0 = time.perf_counter()
        want = R.routes(*R.serpentine(G), snake, 1, 1024)
        res["serpentine_host_ms"] = (time.perf_counter() - t0) * 1e3
        assert want["info"].tolist() == res["serpentine_info"]
        t2 = []
        for _ in range(5):                 # what the host version pays on top: the grids to the host
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
