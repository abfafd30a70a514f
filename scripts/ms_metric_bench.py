"""Per-call mean-shift clustering time for both embedding metrics at 480x640 (100 seeds, 10 iterations), B = 1 and
B = 12 fields per call: the whole uoc_ms_cluster_ex call and its hill-climbing stage alone (uoc_ms_hill_climb_ex).
Prints one JSON line; --out also writes it to a file.

    python scripts/ms_metric_bench.py [--reps 20] [--out profiles/ms_metric_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unseenobjectclustering_amd import _native, synth  # noqa: E402
from unseenobjectclustering_amd.utils import mean_shift as MS  # noqa: E402


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, m, iters = 480, 640, 100, 10
    n = H * W
    fields = np.stack([synth.embedding_field(100 + i, H, W, 64, 4 + i % 4, 0.05)[0] for i in range(12)])
    L = _native.lib()
    out = {"shape": [H, W], "num_seeds": m, "iters": iters, "reps": args.reps, "device": torch.cuda.get_device_name(dev)}
    for B in (1, 12):
        X = torch.from_numpy(fields[:B]).to(dev).contiguous()
        firsts = [(7919 * (i + 1)) % n for i in range(B)]
        ws = MS._workspace(dev, L.uoc_ms_workspace_bytes(B, n, m))
        for metric in ("cosine", "euclidean"):
            met = _native.metric_code(metric)
            _, _, Z0, _ = MS.cluster_batch(X, firsts, 20.0, m, 0, 0.04, return_parts=True, metric=metric)   # the seeds
            Z = Z0.clone()

            def cluster():
                MS.cluster_batch(X, firsts, 20.0, m, iters, 0.04, metric=metric)

            def climb():
                Z.copy_(Z0)
                rc = L.uoc_ms_hill_climb_ex(_native.ptr(X), B, n, _native.ptr(Z), m, 20.0, iters, met, _native.ptr(ws),
                                            ws.numel(), _native.stream_ptr(dev))
                _native.check(rc, "uoc_ms_hill_climb_ex")

            med, lo = _time(cluster, args.reps)
            hmed, hlo = _time(climb, args.reps)
            out[f"B{B}_{metric}_cluster_us"] = round(med, 1)
            out[f"B{B}_{metric}_cluster_min_us"] = round(lo, 1)
            out[f"B{B}_{metric}_hill_climb_us"] = round(hmed, 1)
            out[f"B{B}_{metric}_hill_climb_min_us"] = round(hlo, 1)
        out[f"B{B}_hill_climb_ratio"] = round(out[f"B{B}_euclidean_hill_climb_us"] / out[f"B{B}_cosine_hill_climb_us"], 3)
        out[f"B{B}_cluster_ratio"] = round(out[f"B{B}_euclidean_cluster_us"] / out[f"B{B}_cosine_cluster_us"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
