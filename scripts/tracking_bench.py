"""Tracker.update GPU time (HIP events) at B = 1 and B = 12 streams, 480x640, against the same step in numpy on the host
(tests/tracking_reference.py: contingency table by bincount, the matching in Python integers — what a user writes today,
after copying two label maps to the host and before copying the renumbered one back).

Input: demo-like synthetic streams — 7 ellipses drifting over a 480x640 frame, raw ids re-drawn every frame; stream b
starts b frames into the sequence, which is played forwards and backwards so that the motion never jumps.

    python scripts/tracking_bench.py [--reps 3000] [--host-reps 40] [--streams 1 12] [--out result.json]

Profile the kernels separately, one batch size per run (the kernels have the same names at every B):
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/tracking_bench.py --reps 200 --host-reps 0 --streams 1
and summarise the trace with scripts/rocpd_stats.py.
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

from tests.tracking_reference import ReferenceTracker  # noqa: E402
from unseenobjectclustering_amd.tracking import Tracker  # noqa: E402

H, W, T, OBJECTS = 480, 640, 48, 7
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def sequence(seed=0):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    objs = [dict(a=rng.uniform(30, 70), b=rng.uniform(30, 70), cx=rng.uniform(80, W - 80), cy=rng.uniform(80, H - 80),
                 vx=rng.uniform(-3, 3), vy=rng.uniform(-3, 3)) for _ in range(OBJECTS)]
    frames = np.zeros((T, H, W), dtype=np.int32)
    for t in range(T):
        ids = rng.choice(np.arange(1, 20), size=OBJECTS, replace=False)
        for k, o in enumerate(objs):
            m = ((xs - o["cx"] - t * o["vx"]) / o["a"]) ** 2 + ((ys - o["cy"] - t * o["vy"]) / o["b"]) ** 2 <= 1.0
            frames[t][m] = ids[k]
    return frames


def frame_index(i):
    """0, 1, ..., T-1, T-2, ..., 1, 0, 1, ...: forwards and backwards."""
    i %= 2 * T - 2
    return i if i < T else 2 * T - 2 - i


def gpu_time(frames_dev, B, reps):
    tr = Tracker(min_iou=0.3, max_age=5, streams=B)
    idx = [torch.tensor([frame_index(i + b) for b in range(B)], device=frames_dev.device) for i in range(2 * T - 2)]
    batches = [frames_dev[j].contiguous() for j in idx]            # built ahead: only update() is between the events
    for i in range(60):
        tr.update(batches[i % len(batches)])
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(reps):             # one step per event pair: the time of one update, launch gaps included
        lab = batches[(60 + i) % len(batches)]
        e0.record()
        tr.update(lab)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    live = tr.tracks(0)
    return (float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))), live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3000)
    ap.add_argument("--host-reps", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = sequence()
    frames_dev = torch.from_numpy(frames).to(dev)
    res = {"frames": f"synthetic, {OBJECTS} drifting ellipses, {H}x{W}", "reps": args.reps, "frame_ms": args.frame_ms}
    for B in args.streams:
        (med, p10, p90), live = gpu_time(frames_dev, B, args.reps)
        res[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                        "share_of_frame": med / B / (args.frame_ms * 1e3), "live_tracks": int(live["slot"].size),
                        "uids_handed_out": live["next_uid"] - 1}
        if args.host_reps > 0:
            refs = [ReferenceTracker(0.3, 5) for _ in range(B)]
            t = []
            for i in range(args.host_reps):
                t0 = time.perf_counter()
                for b in range(B):
                    refs[b].step(frames[frame_index(i + b)])
                t.append((time.perf_counter() - t0) * 1e3)
            lab = frames_dev[:B].contiguous()
            t2 = []
            for _ in range(5):            # what the host version pays on top: the map to the host, the renumbered one back
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lab.cpu().numpy()
                torch.from_numpy(frames[:B]).to(dev)
                torch.cuda.synchronize()
                t2.append((time.perf_counter() - t0) * 1e3)
            host = float(np.median(t[3:] if len(t) > 6 else t))
            res[f"B{B}"].update(host_numpy_ms=host, host_copies_ms=float(np.median(t2)), host_over_gpu=host * 1e3 / med)
        print(B, res[f"B{B}"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
