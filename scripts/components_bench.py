"""split_components GPU time (HIP events) at B = 1 and B = 12 frames, 480x640, against the same step on the host: a
scipy.ndimage.label loop over the ids of the map plus the map's copy to the host and the result's copy back — what a
user writes today.

Inputs at 480x640:
  demo        the demo frame's refined label map (tests/golden/demo through the two-stage path, calibrated synthetic weights)
  speckled    synthetic: 8 ellipses and 0.2 % speckle carrying their ids
  serpentine  a one-pixel-wide path over the whole map, one component: the longest union chain (worst case)
  checkerboard  153 600 one-pixel components with connectivity 4: the most roots (worst case)

    python scripts/components_bench.py [--reps 2000] [--host-reps 10] [--frames 1 12] [--inputs demo speckled ...]
                                       [--mode largest] [--min-area 20] [--connectivity 8] [--out result.json]

Profile the kernels separately, one batch size per run (the kernels have the same names at every B):
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/components_bench.py --reps 200 --host-reps 0 --frames 1 --inputs speckled
and summarise the trace with scripts/rocpd_stats.py.
(the JSON result line is always printed; --out also writes it to a file)
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import components_reference as R  # noqa: E402
from unseenobjectclustering_amd.components import split_components  # noqa: E402

H, W, OBJECTS = 480, 640, 8
FRAME_MS = 5.86          # the segmentation's time per frame (bench.py --steps 20 --warmup 5); --frame-ms overrides it


def speckled(seed=0):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W), dtype=np.int32)
    for k in range(OBJECTS):
        a, b = rng.uniform(30, 70), rng.uniform(30, 70)
        cx, cy = rng.uniform(80, W - 80), rng.uniform(80, H - 80)
        img[((xs - cx) / a) ** 2 + ((ys - cy) / b) ** 2 <= 1.0] = k + 1
    speck = rng.random((H, W)) < 0.002
    img[speck] = rng.integers(1, OBJECTS + 1, size=int(speck.sum()))
    return img


def demo_map(dev):
    """The refined label map of the first demo frame."""
    from unseenobjectclustering_amd import io as uio, networks, synth
    from unseenobjectclustering_amd.fcn.config import cfg
    from unseenobjectclustering_amd.fcn.test_dataset import test_sample
    cfg.device = dev
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    net = networks.seg_resnet34_8s_embedding(2, 64, sd).eval()
    demo = os.path.join(ROOT, "tests", "golden", "demo")
    color, depth = sorted(glob.glob(os.path.join(demo, "*-color.png")))[0], sorted(glob.glob(os.path.join(demo, "*-depth.png")))[0]
    cam_file = os.path.join(demo, "camera_params.json")
    cam = json.load(open(cam_file)) if os.path.exists(cam_file) else dict(synth.DEMO_CAMERA)
    np.random.seed(cfg.RNG_SEED)
    out_label, refined = test_sample(uio.read_sample(color, depth, cam), net, net)
    final = refined if refined is not None else out_label
    return final[0].cpu().numpy().astype(np.int32)


def host_split(img, connectivity):
    """The scipy loop: label every id's mask; returns the number of components."""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), dtype=bool)
    found = 0
    for i in np.unique(img):
        if 1 <= i <= 127:
            found += ndimage.label(img == i, structure=structure)[1]
    return found


def gpu_time(lab, reps, **kw):
    for _ in range(30):
        split_components(lab, **kw)
    torch.cuda.synchronize()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):              # one call per event pair: the time of one split, launch gaps included
        e0.record()
        split_components(lab, **kw)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per)), float(np.percentile(per, 10)), float(np.percentile(per, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 12], help="batch sizes to measure")
    ap.add_argument("--inputs", nargs="+", default=["demo", "speckled", "serpentine", "checkerboard"])
    ap.add_argument("--mode", default="largest", choices=["all", "largest"])
    ap.add_argument("--min-area", type=int, default=20)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--frame-ms", type=float, default=FRAME_MS, help="frame time the step is reported as a share of")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(connectivity=args.connectivity, min_area=args.min_area, mode=args.mode)
    res = {"size": f"{H}x{W}", "reps": args.reps, "frame_ms": args.frame_ms, **kw}
    for name in args.inputs:
        conn = 4 if name == "checkerboard" else args.connectivity      # connectivity 8 makes the checkerboard one component
        kw["connectivity"] = conn
        img = {"demo": lambda: demo_map(dev), "speckled": speckled, "serpentine": lambda: R.serpentine(H, W),
               "checkerboard": lambda: R.checkerboard(H, W)}[name]()
        entry = {"connectivity": conn}
        for B in args.frames:
            lab = torch.from_numpy(np.stack([img] * B)).to(dev)
            med, p10, p90 = gpu_time(lab, args.reps, **kw)
            _, _, counts = split_components(lab, **kw)
            entry[f"B{B}"] = {"gpu_us_median": med, "gpu_us_p10": p10, "gpu_us_p90": p90, "gpu_us_per_frame": med / B,
                              "share_of_frame": med / B / (args.frame_ms * 1e3)}
            entry["counts"] = dict(zip(("found", "small", "kept", "dropped"), counts[0].cpu().tolist()))
        if args.host_reps > 0:
            t = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                found = host_split(img, conn)
                t.append((time.perf_counter() - t0) * 1e3)
            assert found == entry["counts"]["found"], (found, entry["counts"])
            lab = torch.from_numpy(img).to(dev)
            t2 = []
            for _ in range(5):             # what the host version pays on top: the map to the host, the result back
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lab.cpu().numpy()
                torch.from_numpy(img).to(dev)
                torch.cuda.synchronize()
                t2.append((time.perf_counter() - t0) * 1e3)
            entry.update(host_scipy_ms=float(np.median(t)), host_copies_ms=float(np.median(t2)))
            if "B1" in entry:
                entry["host_over_gpu"] = entry["host_scipy_ms"] * 1e3 / entry["B1"]["gpu_us_median"]
        res[name] = entry
        print(name, entry, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
