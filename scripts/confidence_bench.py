"""GPU time (HIP events) of the label-confidence entries: uoc_ms_confidence against uoc_ms_assign on the same inputs — one
480x640 field and seven 224x224 crops, 100 converged seeds each, the fields of the golden cases' generator — then
uoc_conf_paste (seven ROIs into a 480x640 frame) and uoc_conf_objects (one 480x640 frame, nine ids in blocks and nine ids
as per-pixel noise); the kernels alone from the library's own profiler (uoc_prof_*) in a pass of its own.  Warm-up first,
then one event pair per call; median, 10th and 90th percentile.

    python scripts/confidence_bench.py [--reps 300] [--out result.json]

(the JSON result line is always printed; --out also writes it to a file.)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from unseenobjectclustering_amd import _native, confidence as CF, synth  # noqa: E402
from unseenobjectclustering_amd.utils import mean_shift as MS  # noqa: E402


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


def clustering_case(dev, seeds, H, W, objects):
    """B fields of the test generator with their converged seeds -> the raw calls of the two assignments on them."""
    X = torch.stack([torch.from_numpy(synth.embedding_field(s, H, W, 64, objects + s % 3, 0.05)[0]) for s in seeds]).to(dev)
    B, n = X.shape[0], X.shape[1]
    firsts = [(977 * k + 13) % n for k in range(B)]
    labels, _, Z, sl = MS.cluster_batch(X, firsts, 20.0, 100, 10, 0.04, return_parts=True, metric="cosine")
    L = _native.lib()
    ordered = torch.sort(sl, dim=1).values
    nu = (1 + (ordered[:, 1:] != ordered[:, :-1]).sum(dim=1)).to(torch.int32)
    out = [torch.empty((B, n), dtype=torch.int32, device=dev) for _ in range(4)]
    margin = torch.empty((B, n), dtype=torch.float32, device=dev)
    ws_a = MS._workspace(dev, L.uoc_ms_workspace_bytes(B, n, 100))
    nws = L.uoc_ms_confidence_workspace_bytes(B, n, 100, 1)
    ws_c = torch.empty(nws, dtype=torch.uint8, device=dev)
    st = _native.stream_ptr(dev)
    p = _native.ptr

    def assign():
        return L.uoc_ms_assign(p(X), B, n, p(Z), p(sl), p(nu), 100, p(out[0]), p(out[1]), p(ws_a), ws_a.numel(), st)

    def confidence():
        return L.uoc_ms_confidence(p(X), 1, B, n, p(Z), p(sl), p(nu), 100, 0, p(out[0]), p(margin), p(out[2]), p(out[1]), p(out[3]),
                                   p(ws_c), nws, st)
    assert assign() == 0
    want = out[0].clone()
    assert confidence() == 0 and torch.equal(out[0], want) and torch.equal(out[0], labels)
    return assign, confidence, margin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"reps": args.reps, "library": os.path.basename(_native.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    for name, seeds, H, W, objects in (("frame_480x640_B1", [1], 480, 640, 6), ("crops_224x224_B7", [2, 3, 4, 5, 6, 7, 8], 224, 224, 3)):
        assign, confidence, margin = clustering_case(dev, seeds, H, W, objects)
        rec = {"assign": gpu_time(assign, args.reps), "confidence": gpu_time(confidence, args.reps)}
        rec["assign"]["kernels_us"] = kernel_split(assign, min(args.reps, 200), ("assign", "relabel"))
        rec["confidence"]["kernels_us"] = kernel_split(confidence, min(args.reps, 200), ("ms_confidence", "relabel"))
        rec["call_ratio"] = rec["confidence"]["median_us"] / rec["assign"]["median_us"]
        rec["kernel_ratio"] = rec["confidence"]["kernels_us"]["ms_confidence"] / rec["assign"]["kernels_us"]["assign"]
        res[name] = rec
        print(name, rec, flush=True)
    # the glue: seven 224x224 crops pasted into a 480x640 frame, and the per-id summary of one frame
    H, W, K, S = 480, 640, 7, 224
    t = _native.RoiTable()
    t.K = K
    for k in range(K):
        x0, y0 = 40 + 80 * k, 60 + 45 * (k % 3)
        t.box[k][0], t.box[k][1], t.box[k][2], t.box[k][3] = x0, y0, min(x0 + 120, W - 1), min(y0 + 160, H - 1)
    table = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev)
    labels_crop = torch.from_numpy(np.random.default_rng(0).integers(0, 3, size=(K, S * S)).astype(np.int32)).to(dev)
    plan = torch.zeros((K + K * 128,), dtype=torch.int32, device=dev)
    plan[:K] = torch.arange(K, dtype=torch.int32)
    plan[K:].view(K, 128)[:, 1] = torch.arange(1, K + 1, dtype=torch.int32)          # cluster 1 of every crop is kept
    values = torch.rand((K, S * S), device=dev)
    frame = torch.ones((H * W,), device=dev)
    paste = lambda: CF.paste_values(values, labels_crop, table, plan, K, H, W, frame)      # noqa: E731
    res["paste_480x640_K7"] = gpu_time(paste, args.reps)
    conf = torch.rand((1, H, W), device=dev)
    res["glue_kernels_us"] = {"paste": kernel_split(paste, 200, ("conf_glue",))}
    ys, xs = np.mgrid[0:H, 0:W]
    maps = {"blocks": ((ys // 96) * 3 + xs // 214) % 9,                       # nine ids in 96 x 214 blocks: one or two ids per wave
            "noise": np.random.default_rng(1).integers(0, 9, size=(H, W))}   # nine ids per wave: the worst case of the per-wave combine
    for kind, ids in maps.items():
        lab = torch.from_numpy(ids.astype(np.int32)[None]).to(dev)
        objects = lambda: CF.object_stats(lab, conf, 1311)                                   # noqa: E731
        res[f"objects_480x640_B1_{kind}"] = gpu_time(objects, args.reps)
        res["glue_kernels_us"][f"objects_{kind}"] = kernel_split(objects, 200, ("conf_glue",))
    print({k: v for k, v in res.items() if k.startswith(("paste", "objects", "glue"))}, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
