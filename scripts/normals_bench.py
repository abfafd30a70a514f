"""GPU time (HIP events) of uoc_normals on the 480x640 boxes scene of the tests (tests/normals_reference.boxes_scene): one
frame and twelve, at the default stencil (step 2, window 2) and at the largest (step 8, window 4), with and without the
fp32 unit normals; the two launch groups alone from the library's own profiler (uoc_prof_*) in a pass of its own; and the
numpy reference on this machine's CPU for the same frame.  Warm-up first, then one event pair per call; median, 10th and
90th percentile.  Before anything is timed the B = 1 result is compared with the reference bit for bit.

    python scripts/normals_bench.py [--reps 300] [--out result.json]

(the JSON result line is always printed; --out also writes it to a file.)
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

from tests import normals_reference as R  # noqa: E402
from unseenobjectclustering_amd import _native, normals  # noqa: E402


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
    return {"median_us": float(np.median(per)), "p10_us": float(np.percentile(per, 10)), "p90_us": float(np.percentile(per, 90))}


def kernel_split(call, reps, names):
    """us per launch group, from the events the library records around its launches."""
    _native.prof_enable(True)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    rep = _native.prof_report()
    _native.prof_enable(False)
    return {r["kernel"]: round(1e3 * r["total_ms"] / reps, 2) for r in rep if r["kernel"] in names}


def raw_call(dev, X, L, P, step, window, jump_mm, unit):
    """The bare C call on preallocated buffers: what a steady-state caller pays."""
    B, _, H, W = X.shape
    lib = _native.lib()
    nws = lib.uoc_normals_workspace_bytes(B, H, W)
    packed = torch.empty((B, H, W, 4), dtype=torch.int32, device=dev)
    un = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if unit else None
    faces = torch.empty((B, 128, 40), dtype=torch.int32, device=dev)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dirs = np.ascontiguousarray(normals.direction_table(16))
    c_up, s_side = normals.thresholds(20.0, 20.0)
    st, p = _native.stream_ptr(dev), _native.ptr
    mp = max(1, window // 2)

    def call():
        return lib.uoc_normals(p(X), p(L), p(P), B, H, W, step, window, jump_mm, mp, dirs.ctypes.data, 16, c_up, s_side, p(packed), p(un),
                               p(faces), p(ws), nws, st)
    assert call() == 0
    return call, packed, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = 480, 640
    res = {"reps": args.reps, "library": os.path.basename(_native.LIB_PATH), "device": torch.cuda.get_device_name(0), "frame": [H, W]}
    scenes = [R.boxes_scene(H, W, seed) for seed in range(1, 13)]
    lab = np.stack([s[0] for s in scenes])
    xyz = np.stack([s[1] for s in scenes])
    plane = R.table_plane()
    rec = np.stack([R.plane_record(plane)] * 12)
    for step, window, jump_mm in ((2, 2, 30), (8, 4, 30)):
        t0 = time.perf_counter()
        want = R.estimate(xyz[0], lab[0], plane, step=step, window=window, jump_mm=jump_mm)
        res[f"numpy_reference_s_r{step}_s{window}"] = time.perf_counter() - t0
        for B in (1, 12):
            X, L, P = (torch.from_numpy(a[:B].copy()).to(dev) for a in (xyz, lab, rec))
            for unit in (False, True):
                call, packed, faces = raw_call(dev, X, L, P, step, window, jump_mm, unit)
                torch.cuda.synchronize()
                got = packed[0].cpu().numpy()
                assert np.array_equal(got[..., :3], want["n"]) and np.array_equal(got[..., 3], want["info"])
                assert np.array_equal(faces[0].cpu().numpy(), want["faces"])
                name = f"r{step}_s{window}_B{B}" + ("_unit" if unit else "")
                res[name] = gpu_time(call, args.reps)
                res[name]["kernels_us"] = kernel_split(call, min(args.reps, 200), ("normals_pixels", "normals_faces"))
                res[name]["with_normal"] = int(faces[:, :, 1].sum())
                print(name, res[name], flush=True)
    # without labels and without a plane: the bare normals
    X = torch.from_numpy(xyz[:1].copy()).to(dev)
    call, _, _ = raw_call(dev, X, None, None, 2, 2, 30, False)
    res["r2_s2_B1_bare"] = gpu_time(call, args.reps)
    # the wrapper, allocations included
    L, P = torch.from_numpy(lab[:1].copy()).to(dev), torch.from_numpy(rec[:1].copy()).to(dev)
    fitted = type("Fitted", (), {"records": P})()
    res["estimate_B1"] = gpu_time(lambda: normals.estimate(X, L, fitted), args.reps)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
