"""identity.describe and Identifier.update GPU time (HIP events) at B = 1 and B = 12 streams, 480x640, against the same
work in numpy on the host (tests/identity_reference.py: the votes by np.add.at, the matching in Python integers — what a
user writes today, after copying the tracked map and the image to the host).

Input: demo-like synthetic streams — 7 coloured ellipses with byte noise drifting over a grey table, tracked ahead of the
timed loop by a Tracker whose tables are kept per frame; one ellipse jumps every 12 frames, so the identity step has
newcomers and lost entries to match.  Stream b starts b frames into the sequence, played forwards and backwards.

    python scripts/identity_bench.py [--reps 2000] [--host-reps 10] [--streams 1 12] [--out result.json]

Profile the kernels separately, one batch size per run (the kernels have the same names at every B):
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/identity_bench.py --reps 200 --host-reps 0 --streams 1
and summarise the trace with scripts/rocpd_stats.py.  Registers, LDS and occupancy per kernel come from the compiler:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -c unseenobjectclustering_amd/csrc/identity.hip -Rpass-analysis=kernel-resource-usage
(the JSON result line is always printed; --out also writes it to a file; profiles/identity.md quotes both)
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

from tests import identity_reference as ir  # noqa: E402
from unseenobjectclustering_amd import _native, identity  # noqa: E402
from unseenobjectclustering_amd.tracking import Tracker  # noqa: E402

H, W, T, OBJECTS = 480, 640, 48, 7
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def sequence(seed=0):
    """labels [T,H,W] int32, images [T,H,W,3] uint8, xyz [T,3,H,W] float32."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    objs = [dict(a=rng.uniform(30, 70), b=rng.uniform(30, 70), cx=rng.uniform(80, W - 80), cy=rng.uniform(80, H - 80),
                 vx=rng.uniform(-3, 3), vy=rng.uniform(-3, 3), colour=rng.integers(20, 236, size=3)) for _ in range(OBJECTS)]
    labels = np.zeros((T, H, W), dtype=np.int32)
    images = np.zeros((T, H, W, 3), dtype=np.uint8)
    xyz = np.zeros((T, 3, H, W), dtype=np.float32)
    for t in range(T):
        ids = rng.choice(np.arange(1, 20), size=OBJECTS, replace=False)
        img = np.full((H, W, 3), 90, dtype=np.int64)
        z = np.full((H, W), 1.0, dtype=np.float32)
        for k, o in enumerate(objs):
            jump = 200.0 * ((t // 12) % 2) if k == 0 else 0.0
            m = ((xs - o["cx"] - t * o["vx"] - jump) / o["a"]) ** 2 + ((ys - o["cy"] - t * o["vy"]) / o["b"]) ** 2 <= 1.0
            labels[t][m], img[m], z[m] = ids[k], o["colour"], 0.9
        images[t] = np.clip(img + rng.integers(-6, 7, size=img.shape), 0, 255)
        xyz[t, 2] = z
    return labels, images, xyz


def frame_index(i):
    """0, 1, ..., T-1, T-2, ..., 1, 0, 1, ...: forwards and backwards."""
    i %= 2 * T - 2
    return i if i < T else 2 * T - 2 - i


def timed(fn, batches, reps, warm=60):
    for i in range(warm):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(reps):             # one call per event pair: the time of one call, launch gaps included
        item = batches[(warm + i) % len(batches)]
        e0.record()
        fn(item)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def gpu_times(dev_seq, B, reps):
    labels, images, xyz = dev_seq
    tracker = Tracker(min_iou=0.3, max_age=5, streams=B)
    batches = []
    for i in range(2 * T - 2):        # tracked maps and the tracker's table per frame, built ahead of the timed loops
        j = torch.tensor([frame_index(i + b) for b in range(B)], device=labels.device)
        tracked = tracker.update(labels[j].contiguous())
        batches.append((tracked, _native.Fields(streams=B, table=tracker.table.clone()), images[j].contiguous(), xyz[j].contiguous()))
    ident = identity.Identifier(streams=B)
    describe = timed(lambda it: identity.describe(it[0], it[2], it[3]), batches, reps)
    update = timed(lambda it: ident.update(it[0], it[1], it[2], it[3]), batches, reps)
    return describe, update, ident.identities(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the calls are reported as a share of")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seq = sequence()
    dev_seq = tuple(torch.from_numpy(x).to(dev) for x in seq)
    res = {"frames": f"synthetic, {OBJECTS} drifting coloured ellipses, one jumping, {H}x{W}", "reps": args.reps, "frame_ms": args.frame_ms}
    for B in args.streams:
        describe, update, live = gpu_times(dev_seq, B, args.reps)
        res[f"B{B}"] = {"describe_us_median": describe[0], "describe_us_p10": describe[1], "describe_us_p90": describe[2],
                        "update_us_median": update[0], "update_us_p10": update[1], "update_us_p90": update[2],
                        "update_us_per_frame": update[0] / B, "share_of_frame": update[0] / B / (args.frame_ms * 1e3),
                        "identities": int(live["entry"].size), "pids_handed_out": live["next_pid"] - 1, "evicted": live["evicted"]}
        if args.host_reps > 0:
            from tests.tracking_reference import ReferenceTracker
            trackers = [ReferenceTracker(0.3, 5) for _ in range(B)]
            idents = [ir.ReferenceIdentifier() for _ in range(B)]
            t_desc, t_step = [], []
            for i in range(args.host_reps):
                d = s = 0.0
                for b in range(B):
                    j = frame_index(i + b)
                    tracked = trackers[b].step(seq[0][j])
                    t0 = time.perf_counter()
                    sig = ir.describe(tracked, seq[1][j], seq[2][j])
                    t1 = time.perf_counter()
                    idents[b].step(trackers[b].table32(), sig)
                    idents[b].relabel(tracked)
                    d, s = d + (t1 - t0), s + (time.perf_counter() - t1)
                t_desc.append(d * 1e3)
                t_step.append(s * 1e3)
            host = float(np.median(t_desc)) + float(np.median(t_step))
            res[f"B{B}"].update(host_describe_ms=float(np.median(t_desc)), host_step_ms=float(np.median(t_step)),
                                host_over_gpu=host * 1e3 / update[0])
        print(B, res[f"B{B}"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
