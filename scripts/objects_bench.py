"""uoc_objects GPU time (HIP events) at B = 1 and B = 12, 480x640, against the same extraction in numpy on the host
(tests/objects_reference.py: a loop over the ids with boolean masks and np.linalg.eigh, which is what a user writes today).

Input: the demo frame's XYZ planes and the refined label map of tests/golden/demo.npz, repeated B times.

    python scripts/objects_bench.py [--reps 200] [--host-reps 3] [--out result.json]

Profile the kernels separately: rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/objects_bench.py --reps 50 --host-reps 0
(the JSON result line is always printed; --out also writes it to a file)
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import objects_reference as R  # noqa: E402
from unseenobjectclustering_amd import _native, io as uio  # noqa: E402
from unseenobjectclustering_amd import objects as O  # noqa: E402


def demo_inputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "demo.npz"))
    d = os.path.join(ROOT, "tests", "golden", "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    s = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    return np.asarray(g["refined"]).astype(np.int32).reshape(1, 480, 640), s["depth"].numpy()


def gpu_time(lab, xyz, reps, points=True):
    dev = lab.device
    B, H, W = lab.shape
    lib = _native.lib()
    n = B * H * W
    rec = torch.empty((B, 128, O._W), dtype=torch.int32, device=dev)
    pts = torch.empty((n, 3), device=dev) if points else None
    pix = torch.empty((n,), dtype=torch.int32, device=dev) if points else None
    tot = torch.empty((1,), dtype=torch.int32, device=dev)
    nws = lib.uoc_objects_workspace_bytes(B, H, W)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    st = _native.stream_ptr(dev)
    P = _native.ptr

    def call():
        _native.check(lib.uoc_objects(P(lab), P(xyz), None, 0, B, H, W, 0, P(rec), P(pts), None, P(pix), ctypes.c_long(n), P(tot),
                                      P(ws), nws, st), "uoc_objects")
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):            # one call per event pair: the time of one extraction, launch gaps included
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lab1, xyz1 = demo_inputs()
    res = {"frame": "tests/golden/demo (refined map), 480x640", "reps": args.reps}
    for B in (1, 12):
        lab = torch.from_numpy(np.repeat(lab1, B, 0)).to(dev).contiguous()
        xyz = torch.from_numpy(np.repeat(xyz1, B, 0)).to(dev).contiguous()
        med, p10, p90 = gpu_time(lab, xyz, args.reps)
        rmed, _, _ = gpu_time(lab, xyz, args.reps, points=False)
        res[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_records_only": rmed}
        if args.host_reps > 0:
            lab_h, xyz_h = np.repeat(lab1, B, 0), np.repeat(xyz1, B, 0)
            t = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                R.extract(lab_h, xyz_h)
                t.append((time.perf_counter() - t0) * 1e3)
            t2 = []
            for _ in range(args.host_reps):      # what a user pays first today: label map and XYZ to the host
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lab.cpu().numpy(), xyz.cpu().numpy()
                t2.append((time.perf_counter() - t0) * 1e3)
            res[f"B{B}"].update(host_numpy_ms=float(np.median(t)), d2h_copy_ms=float(np.median(t2)))
        print(B, res[f"B{B}"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
