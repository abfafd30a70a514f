#!/usr/bin/env python
"""Benchmark of the hot path: end-to-end two-stage RGB-D segmentation at 640x480.

    python bench.py --gpus N --steps K --warmup W          weak scaling: K frames per GPU
    python bench.py --gpus N --frames F --warmup W         strong scaling: F frames sharded in contiguous blocks of
                                                           ceil(F/N) (BASELINE.json configs[4]: --frames 1024 --gpus 8)
    ... --full                                             also the legs listed below (roofline, cpu_baseline, parity,
                                                           latency, sustained, pcie_inclusive_frames_per_s) and the side file
    ... --dump-outputs DIR                                 after the timed steps: DIR/label_map.npy, the [480, 640] label
                                                           map of the last timed frame as float32

For N > 1 either launch it under torch.distributed.run (the driver does; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*
are read from the environment) or call it bare: without WORLD_SIZE in the environment `python bench.py --gpus N`
re-executes itself under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`.

One step = one synthetic 640x480 RGB-D frame through the whole path on one GPU (throughput schedule: --inflight streams,
each working on launch sets of --frames-per-launch frames; the one-frame-at-a-time latency is reported next to it):
RGB-D ResNet34-8s embedding -> mean-shift (100 seeds, 10 iterations) -> depth filter -> ROI
crops -> second network on the K crops -> K batched mean-shifts -> match/paste (BASELINE.json
configs[3]; configs[4] = the same sharded over N GPUs with one RCCL all_gather of the label maps).
Global frame g is `synth.palette_frame(10000 + g)` with the first-seed RNG seeded by `runner.frame_rng_seed(g)` on
every rank count, so the gathered [F,480,640] uint8 block does not depend on the sharding.
Inputs are resident in HBM when the timed region starts; the timed region includes the (collective and the) D2H of
the label-map block.  Weights are the calibrated synthetic set (synth.calibrated_state_dict):
random-init backbone of the reference architecture + closed-form calibration so that synthetic
frames segment into their objects and stage 2 really runs (K ~ 6-8 ROIs per frame).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the steps and prints the contract fields (the
other blocks are null).  With --full, besides the contract fields:
  roofline      the kernel class with the largest share of GPU time in a profiled pass over the same frames (HIP
                events on the launch stream, csrc/prof.hip)
  cpu_baseline  the CPU oracle (torch-CPU restatement of the reference path) on the FIRST frames of the timed set,
                same frames / seeds / weights as the GPU leg (bounded sample)
  parity        the GPU label maps of those frames against the oracle's (agreement up to label permutation), split the way
                north_star's two clauses can jointly hold: embed_max_err (HIP vs oracle embeddings, stage 1 and crops),
                exact_given_oracle_embeddings (the oracle's embeddings through the HIP clustering / ROI / paste kernels:
                bit-exact), stage1_exact and the end-to-end mismatched pixels per frame
  latency       one frame at a time on one stream (frames_per_launch 1, streams 1), same frames (N = 1)
  sustained     the same block of frames looped for >= 10 s, with clock / power samples (N = 1)
  pcie_inclusive_frames_per_s   the timed frames again as RAW samples (uint8 BGR + uint16 depth, 1.5 MB per frame) uploaded
                per frame from pinned host memory and prepared on the device (uoc_prep_rgbd) (N = 1)
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

H, W = 480, 640
FIRST_PALETTE_SEED = 10_000
PEAK_HBM_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s
PEAK_FP32_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense fp32 MFMA (= vector) peak


# ----------------------------------------------------------------------------------------------------------------
# workload: global frame index -> inputs
# ----------------------------------------------------------------------------------------------------------------
def _palette(g):
    from unseenobjectclustering_amd import synth
    s = FIRST_PALETTE_SEED + g
    fr = synth.palette_frame(s, H, W, 5 + s % 3)
    return fr["image_color"], fr["depth"]


def _block(total, rank, world):
    """This rank's contiguous frame block — runner.shard_range without importing the package (bench.main asserts equality)."""
    per = (total + world - 1) // world
    return min(rank * per, total), min((rank + 1) * per, total)


def host_frames(lo, hi):
    """Synthetic inputs of the global frames [lo, hi) as numpy arrays (a process pool for big blocks)."""
    idx = list(range(lo, hi))
    if len(idx) > 32:
        import multiprocessing as mp
        try:
            ncpu = len(os.sched_getaffinity(0))
        except AttributeError:
            ncpu = os.cpu_count() or 1
        with mp.get_context("fork").Pool(max(1, min(32, ncpu // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))))) as pool:
            return pool.map(_palette, idx, chunksize=4)
    return [_palette(g) for g in idx]


# ----------------------------------------------------------------------------------------------------------------
# CPU leg: the oracle on the first frames of the timed set (child process)
# ----------------------------------------------------------------------------------------------------------------
def cpu_model_name():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


# UOC_BENCH_CPU_SECONDS: a longer CPU sample for parity statistics over more frames (default: the bounded ~30 s sample)
CPU_SAMPLE_SECONDS = float(os.environ.get("UOC_BENCH_CPU_SECONDS", "30"))


def cpu_baseline(frames, out_path):
    """The oracle's two-stage test_sample on the host cores (torch CPU ops = the reference's ops), on global frames
    0..frames-1 of the benchmark set with the runner's per-frame RNG seeds.  Label maps go to `out_path` (npz)."""
    from oracle import backbone_oracle as BO, glue_oracle as GO
    from unseenobjectclustering_amd import runner, synth
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    # The oracle is many small torch ops; beyond ~64 threads the intra-op pool only adds synchronisation cost (with
    # all 256+ hardware threads of the bench box a frame took minutes instead of seconds), so the thread count is
    # capped at 64 and both numbers are reported: `cores` = threads used, `host_cores` = what the box has.  A job given
    # fewer cores than the box has says so through OMP_NUM_THREADS, which then caps the count as well.
    omp = os.environ.get("OMP_NUM_THREADS", "")
    torch.set_num_threads(max(1, min(ncpu, 64, int(omp) if omp.isdigit() and int(omp) > 0 else 64)))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    captured = []

    def net(img, label, depth):
        f = BO.segnet_forward(sd, img, depth)
        captured.append((img, depth, f))
        return f
    inputs = host_frames(0, frames)
    maps, stage1 = [], []
    embed_dir = os.path.join(os.path.dirname(out_path), "embed") if out_path else None
    if embed_dir:
        os.makedirs(embed_dir, exist_ok=True)
    t0 = time.time()
    spent_saving = 0.0
    for g, (img, dep) in enumerate(inputs):
        del captured[:]
        out, refined = GO.test_sample(torch.from_numpy(img), torch.from_numpy(dep), net, net,
                                      np.random.RandomState(runner.frame_rng_seed(g)))
        maps.append((refined if refined is not None else out)[0].numpy().astype(np.int32))
        stage1.append(out[0].numpy().astype(np.int32))
        if embed_dir and len(captured) == 2:      # the oracle's embeddings and its own crops, for the decomposed parity check
            t1 = time.time()
            np.save(os.path.join(embed_dir, f"f1_{g}.npy"), captured[0][2].numpy())
            np.save(os.path.join(embed_dir, f"rgb_c_{g}.npy"), captured[1][0].numpy())
            np.save(os.path.join(embed_dir, f"dep_c_{g}.npy"), captured[1][1].numpy())
            np.save(os.path.join(embed_dir, f"f2_{g}.npy"), captured[1][2].numpy())
            spent_saving += time.time() - t1
        if time.time() - t0 - spent_saving > CPU_SAMPLE_SECONDS:          # bounded sample: stop after ~30 s of CPU work
            break
    t0 += spent_saving
    dt = time.time() - t0
    done = len(maps)
    if out_path:
        np.savez_compressed(out_path, final=np.stack(maps), stage1=np.stack(stage1))
    return {"value": round(done / dt, 4), "unit": "frames/s", "cores": torch.get_num_threads(), "host_cores": ncpu,
            "cpu_model": cpu_model_name(), "kind": "port",
            "sample": f"global frames 0..{done - 1} of the GPU leg's set (same inputs, RNG seeds and weights), full "
                      f"two-stage path, oracle/ (torch CPU fp32, {torch.get_num_threads()} threads)"}


def cpu_baseline_subprocess(frames, out_path, limit_s=300):
    """Runs the CPU leg in a child process so a slow host can never stall the GPU benchmark."""
    limit_s = max(limit_s, 2.0 * CPU_SAMPLE_SECONDS + 120.0)
    fail = {"value": None, "unit": "frames/s", "cores": None, "cpu_model": cpu_model_name(), "kind": "port"}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", str(frames),
                            "--cpu-out", out_path], capture_output=True, text=True, timeout=limit_s)
        for ln in reversed(r.stdout.strip().splitlines()):
            if ln.startswith("{"):
                return json.loads(ln)
        return dict(fail, sample="failed: " + r.stderr[-200:])
    except subprocess.TimeoutExpired:
        return dict(fail, sample=f"timed out after {limit_s}s on this host")


def _mismatched_pixels(a, b):
    """Pixels on which two partitions disagree under the best one-to-one relabelling (Hungarian on the contingency table)."""
    from scipy.optimize import linear_sum_assignment
    a, b = np.asarray(a).astype(np.int64).ravel(), np.asarray(b).astype(np.int64).ravel()
    ka, kb = int(a.max()) + 1, int(b.max()) + 1
    table = np.bincount(a * kb + b, minlength=ka * kb).reshape(ka, kb)
    r, c = linear_sum_assignment(-table)
    return int(a.size - table[r, c].sum())


def parity_report(gpu_maps, cpu_npz, network=None, network_crop=None, device=None):
    """The GPU leg against the oracle on the shared frames, split where north_star's two clauses meet:
    embeddings (<= 1e-3) | the integer path GIVEN the oracle's embeddings (bit-exact) | end to end (measured)."""
    from oracle import mean_shift_oracle as O
    z = np.load(cpu_npz)
    want, want1 = z["final"], z["stage1"]
    n = min(len(want), len(gpu_maps))
    agree, exact, mism = [], True, []
    for i in range(n):
        bad = _mismatched_pixels(gpu_maps[i], want[i])
        agree.append(1.0 - bad / want[i].size)
        mism.append(bad)
        exact = exact and bool(O.labels_equal_up_to_permutation(gpu_maps[i].astype(np.int64), want[i].astype(np.int64)))
    # every pixel that differs must be a near-tie of the oracle's own run (oracle/margins.py; committed per bench frame in
    # tests/golden/bench_margins): margin of its nearest-seed decision <= TAU.  tests/test_headline_parity_gpu.py proves
    # this over all 1024 frames; here it is re-checked on the frames of this run.
    from oracle import margins as MG
    near = MG.load_bench_margins(ROOT, frames=range(n))
    beyond, beyond_px = 0, {}
    for i in range(n):
        if mism[i] and i in near:
            bad = MG.label_changes(want[i], gpu_maps[i])
            over = bad[MG.lookup_margins(near[i]["idxF"], near[i]["valF"], bad) > MG.TAU]
            beyond += int(len(over))
            if len(over):
                beyond_px[i] = over
        elif mism[i]:
            beyond += mism[i]
            beyond_px[i] = MG.label_changes(want[i], gpu_maps[i])
    # pixels beyond the margin: the FROZEN perturbation protocol of tests/test_headline_parity_gpu.py (oracle/margins.py:
    # PERTURB_RUNS seeded runs of the oracle at 1x the measured embedding error, oracle embeddings only).  What it explains is
    # "unresolved by the oracle"; a frame that needs the escalation (more runs / 2x / 4x eps) is REPORTED as escalated;
    # what even that does not cover is unexplained.  Bounded: at most two frames (~1 min of oracle each).
    escalated, unexplained = [], 0
    if beyond_px:
        from oracle import backbone_oracle as BO
        from unseenobjectclustering_amd import runner as _runner, synth as _synth
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in _synth.calibrated_state_dict().items()}
        cpu_net = lambda image, label, depth: BO.segnet_forward(sd, image, depth)
        for i in sorted(beyond_px)[:2]:
            img, dep = (torch.from_numpy(a) for a in _palette(i))
            changed, base, info, _ = MG.unresolved_pixels(img, dep, cpu_net, _runner.frame_rng_seed(i), 2.5e-6)
            px = beyond_px[i]
            ok = np.isin(px, changed) | (info["marginF"].reshape(-1)[px] <= MG.TAU)
            if not ok.all():
                extra, _, _ = MG.escalated_pixels(img, dep, cpu_net, _runner.frame_rng_seed(i), base, 2.5e-6, px[~ok])
                escalated.append(i)
                unexplained += int((~ok & ~np.isin(px, extra)).sum())
        unexplained += sum(len(beyond_px[i]) for i in sorted(beyond_px)[2:])
    rep = {"frames": n, "label_agreement_min": round(min(agree), 6) if agree else None,
           "mismatched_pixels": mism, "mismatches_beyond_margin": beyond, "margin_tau": MG.TAU,
           "escalated_frames": escalated, "unexplained_pixels": unexplained,
           "perturbation_protocol": f"{MG.PERTURB_RUNS} seeded oracle runs at 1x eps = 2.5e-6, oracle embeddings only",
           "exact_up_to_permutation": exact if n else None,
           "against": "oracle/ (torch-CPU restatement pinned to the reference by tests/golden), same frames/seeds/weights"}
    embed_dir = os.path.join(os.path.dirname(cpu_npz), "embed")
    if network is None or not os.path.isdir(embed_dir):
        return rep
    from unseenobjectclustering_amd import runner
    from unseenobjectclustering_amd.fcn import test_dataset as TD
    worst, s1_exact, given_exact, used, given_bad, given_beyond = 0.0, True, True, 0, [], 0
    # the oracle's maps of the same frames from ANOTHER host (tests/golden/bench_oracle: the build container, 4 threads)
    import glob
    fixture = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "bench_oracle", "frames_*.npz"))):
        zf = np.load(path)
        if int(zf["first"]) < n:
            first, fin = int(zf["first"]), zf["final"]       # an NpzFile decompresses the whole array on every access
            for i in range(min(len(fin), n - first)):
                fixture[first + i] = fin[i].copy()
    given_bad_fix, oracle_vs_fix = [], []
    for g in range(n):
        if not os.path.exists(os.path.join(embed_dir, f"f2_{g}.npy")):
            continue
        used += 1
        img, dep = (torch.from_numpy(a) for a in _palette(g))
        f1, f2 = (torch.from_numpy(np.load(os.path.join(embed_dir, f"{k}_{g}.npy"))) for k in ("f1", "f2"))
        rgb_c, dep_c = (torch.from_numpy(np.load(os.path.join(embed_dir, f"{k}_{g}.npy"))) for k in ("rgb_c", "dep_c"))
        # (a) HIP embeddings on the oracle's inputs (the frame, and the oracle's own crops)
        e1 = network(img.to(device), None, dep.to(device)).cpu()
        e2 = network_crop(rgb_c.to(device), None, dep_c.to(device)).cpu()
        worst = max(worst, float((e1 - f1).abs().max()), float((e2 - f2).abs().max()))
        # (b) the oracle's embeddings through the HIP integer path
        np.random.seed(runner.frame_rng_seed(g))
        out_b, ref_b = TD.test_sample(dict(image_color=img, depth=dep), lambda *a: f1.to(device), lambda *a: f2.to(device))
        fin_b = (ref_b if ref_b is not None else out_b)[0].numpy()
        given_exact = given_exact and bool(O.labels_equal_up_to_permutation(out_b[0].numpy(), want1[g])) \
            and bool(O.labels_equal_up_to_permutation(fin_b, want[g]))
        given_bad.append(_mismatched_pixels(fin_b, want[g]))
        if given_bad[-1] and g in near:      # the oracle's own last pixels move with the thread count / host: margin rule here too
            bad_px = MG.label_changes(want[g], fin_b)
            given_beyond += int((MG.lookup_margins(near[g]["idxF"], near[g]["valF"], bad_px) > MG.TAU).sum())
        elif given_bad[-1]:
            given_beyond += given_bad[-1]
        if g in fixture:
            given_bad_fix.append(_mismatched_pixels(fin_b, fixture[g]))
            oracle_vs_fix.append(_mismatched_pixels(want[g], fixture[g]))
        # (c) stage 1 of the full HIP path
        np.random.seed(runner.frame_rng_seed(g))
        out_c, _ = TD.test_sample(dict(image_color=img, depth=dep), network, None)
        s1_exact = s1_exact and bool(O.labels_equal_up_to_permutation(out_c[0].numpy(), want1[g]))
    rep.update({"decomposed_frames": used, "embed_max_err": worst, "embed_tolerance": 1e-3,
                "exact_given_oracle_embeddings": given_exact if used else None,
                "given_oracle_embeddings_mismatched_pixels": given_bad, "given_oracle_embeddings_beyond_margin": given_beyond,
                "stage1_exact": s1_exact if used else None,
                "given_oracle_embeddings_mismatched_pixels_vs_fixture_oracle": given_bad_fix or None,
                "this_oracle_run_vs_fixture_oracle_mismatched_pixels": oracle_vs_fix or None,
                "note": "mismatched_pixels = end to end (HIP embeddings -> HIP integer path); *given_oracle_embeddings* = the "
                        "oracle's stage-1 and crop embeddings through the HIP clustering / ROI / match / paste kernels, against "
                        "THIS run's oracle maps; *_vs_fixture_oracle = against the same oracle run on another host "
                        "(tests/golden/bench_oracle), and this_oracle_run_vs_fixture_oracle = the two oracle runs against each "
                        "other.  Bench frame 0 holds one pixel at which the oracle itself is not reproducible: "
                        "its torch-CPU result differs between 1 and 4 threads on this host and between hosts "
                        "(profiles/r03_oracle_thread_sensitivity_gpu_box.json); against the committed 4-thread oracle fixture the "
                        "HIP integer path is bit-exact on all 24 frames tested (tests/test_headline_parity_gpu.py).  "
                        "Histogram over 1024 frames: profiles/r03_parity_histogram.json"})
    return rep


# ----------------------------------------------------------------------------------------------------------------
# device telemetry for the sustained leg
# ----------------------------------------------------------------------------------------------------------------
class SmiSampler(threading.Thread):
    """Samples sclk / power of GPU `index` through rocm-smi while the sustained loop runs."""

    def __init__(self, index, period=1.0):
        super().__init__(daemon=True)
        self.index, self.period, self.samples, self._stop_evt = index, period, [], threading.Event()

    def run(self):
        while not self._stop_evt.is_set():
            try:
                r = subprocess.run(["rocm-smi", "-d", str(self.index), "--showclocks", "--showpower", "--json"],
                                   capture_output=True, text=True, timeout=10)
                card = next(iter(json.loads(r.stdout).values()))
                s = {}
                for k, v in card.items():
                    kl = k.lower()
                    if kl.startswith("sclk clock speed"):
                        s["sclk_mhz"] = int("".join(ch for ch in str(v) if ch.isdigit()) or 0)
                    elif "power" in kl and "(w)" in kl:
                        s["power_w"] = float(v)
                if s:
                    self.samples.append(s)
            except Exception:       # noqa: BLE001 - telemetry is best effort
                pass
            self._stop_evt.wait(self.period)

    def stop(self):
        self._stop_evt.set()
        self.join(timeout=15)
        return self.samples


def frame_roofline(rois, sec_per_frame):
    """Whole-frame position against both rooflines.  Algorithmic work per frame from SURVEY.md 8(d) (the reference's
    formulation: farthest-point sampling re-reads X every step, convolutions are direct): clustering 8.98 GB + 1.43 GB per
    ROI; backbone 424.4 GFLOP + 69.3 per ROI, clustering 86.5 GFLOP + 14.1 per ROI.
    `mfma_frac` is the EXECUTED-flop fraction (a fraction of a roofline cannot exceed 1): the Winograd-eligible
    convolutions (2 x 208.1 GFLOP of stage 1, 68.0 of a ROI's 69.3) execute 36/144 of their direct flops on the matrix
    pipe — real outputs only, tile padding is waste, not work; everything else executes what it counts.  The algorithmic
    rate (direct-convolution flops over the same time; > 1 is Winograd's saving, not speed) is reported next to it."""
    gb = 8.98 + 1.43 * rois
    gflop = 424.4 + 86.5 + (69.3 + 14.1) * rois
    wino = 416.2 + 68.0 * rois                     # direct-form flops of the layers that run as F(4x4,3x3)
    executed = gflop - 0.75 * wino
    return {"rois_per_frame": round(rois, 2), "algorithmic_gb": round(gb, 2), "algorithmic_gflop": round(gflop, 1),
            "executed_gflop": round(executed, 1),
            "hbm_frac": round(gb / sec_per_frame / PEAK_HBM_GBS, 4),
            "mfma_frac": round(executed / 1e3 / sec_per_frame / PEAK_FP32_TFLOPS, 4),
            "algorithmic_mfma_frac": round(gflop / 1e3 / sec_per_frame / PEAK_FP32_TFLOPS, 4),
            "note": "algorithmic bytes/flops of SURVEY 8(d) per frame over the measured frame time; mfma_frac = flops the "
                    "matrix pipe executes for real outputs (Winograd layers: 36/144 of the direct form); the on-chip sampling "
                    "kernel moves less than the algorithmic bytes"}


# ----------------------------------------------------------------------------------------------------------------
# the record: ONE compact stdout line (the driver keeps only a few KB of output tail) + the full tables in a side file
# ----------------------------------------------------------------------------------------------------------------
MAX_LINE_BYTES = 3000


def write_full_record(line):
    """Everything the run measured (per-kernel / per-launch-shape tables, parity detail, clock samples) as JSON in
    gpurun_out/bench_full.json (UOC_BENCH_FULL overrides; a temp file if the tree is read-only).  Returns the path."""
    path = os.environ.get("UOC_BENCH_FULL") or os.path.join(ROOT, "gpurun_out", "bench_full.json")
    for cand in (path, os.path.join(tempfile.gettempdir(), "uoc_bench_full.json")):
        try:
            os.makedirs(os.path.dirname(cand), exist_ok=True)
            with open(cand, "w") as f:
                json.dump(line, f, indent=1)
            return os.path.relpath(cand, ROOT) if cand.startswith(ROOT + os.sep) else cand
        except OSError:
            continue
    return None


def _pick(d, keys):
    return {k: d[k] for k in keys if d and k in d} if d else None


def compact_line(full, full_path):
    """The stdout line: the contract fields + config + roofline / cpu_baseline / parity / latency in short form.  No
    per-shape tables, no prose notes: round 3's line was 22.7 KB and the driver's output tail cut its head off."""
    out = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = full["config"]
    if full.get("experiment"):
        out["experiment"] = full["experiment"][:120]
    roof = full.get("roofline")
    out["roofline"] = _pick(roof, ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "algorithmic_bytes", "avg_launch_us",
                                   "gpu_time_share", "algorithmic_tflops", "matrix_pipe_tflops", "matrix_pipe_frac"))
    cpu = full.get("cpu_baseline")
    out["cpu_baseline"] = _pick(cpu, ("value", "unit", "cores", "host_cores", "cpu_model", "kind", "sample"))
    if out["cpu_baseline"] and out["cpu_baseline"].get("sample"):
        out["cpu_baseline"]["sample"] = out["cpu_baseline"]["sample"][:110]
    par = full.get("parity")
    out["parity"] = _pick(par, ("frames", "embed_max_err", "stage1_exact", "mismatched_pixels", "mismatches_beyond_margin",
                                "escalated_frames", "unexplained_pixels",
                                "given_oracle_embeddings_mismatched_pixels", "given_oracle_embeddings_beyond_margin",
                                "given_oracle_embeddings_mismatched_pixels_vs_fixture_oracle"))
    for k in ("mismatched_pixels", "given_oracle_embeddings_mismatched_pixels", "given_oracle_embeddings_mismatched_pixels_vs_fixture_oracle"):
        v = (out["parity"] or {}).get(k)         # per-frame lists grow with --cpu-frames: count / max / first 8 beyond that
        if isinstance(v, list) and len(v) > 8:
            out["parity"][k] = {"frames": len(v), "sum": int(sum(v)), "max": int(max(v)), "first": v[:8]}
    lat = full.get("latency")
    out["latency"] = _pick(lat, ("ms_per_frame", "frames_per_s"))
    sus = full.get("sustained")
    out["sustained_frames_per_s"] = sus["frames_per_s"] if sus else None
    out["pcie_inclusive_frames_per_s"] = full.get("pcie_inclusive_frames_per_s")
    fr = full.get("frame_roofline")
    out["frame_roofline"] = _pick(fr, ("rois_per_frame", "hbm_frac", "mfma_frac", "algorithmic_mfma_frac"))
    out["per_rank"] = [_pick(r, ("frames", "compute_s", "gather_s", "host_cpu_s")) for r in (full.get("per_rank") or [])][:8]
    out["kernel_time_share"] = {k["kernel"]: k["gpu_time_share"] for k in (full.get("kernels") or [])[:6]}
    if full.get("kernels_pipe"):       # the same shares inside the shipped multi-stream schedule (transforms weigh more there)
        out["kernel_time_share_pipe"] = {k["kernel"]: k["gpu_time_share"] for k in full["kernels_pipe"][:6]}
    out["full"] = full_path
    size = lambda: len(json.dumps(out, separators=(",", ":")))
    # never again: drop / shorten the optional parts, most expendable first, RE-MEASURING after each step, rather than lose
    # the record to the driver's output tail
    steps = [lambda: out.pop("kernel_time_share_pipe", None), lambda: out.pop("kernel_time_share", None), lambda: out.pop("per_rank", None), lambda: out.pop("frame_roofline", None),
             lambda: out.__setitem__("config", _pick(out.get("config"), ("workload", "total_frames", "frames_per_gpu", "streams_per_gpu",
                                                                         "frames_per_launch")) or {}),
             lambda: out["config"].__setitem__("workload", str(out["config"].get("workload", ""))[:160]),
             lambda: out.__setitem__("parity", _pick(out.get("parity"), ("frames", "embed_max_err", "mismatches_beyond_margin", "escalated_frames"))),
             lambda: (out.get("cpu_baseline") or {}).pop("sample", None), lambda: (out.get("cpu_baseline") or {}).pop("cpu_model", None),
             lambda: out.pop("latency", None), lambda: out.pop("parity", None), lambda: out.pop("config", None) or out.__setitem__("config", {})]
    for step in steps:
        if size() <= MAX_LINE_BYTES:
            break
        step()
    return out


METRIC = "frames/sec at 640x480 RGB-D, two-stage clustering"
# where a run currently is (the `stage` of an error record) and whether this process already wrote its JSON line
STATE = {"stage": "init", "emitted": False, "json_fd": None, "rank": 0, "world": 1, "t0": time.time()}


def error_line(stage, err, n_gpus, **extra):
    """The ONE JSON line of a failed run: the contract's metric with value null, what failed and where."""
    rec = {"metric": METRIC, "value": None, "unit": "frames/s", "n_gpus": n_gpus, "error": str(err)[:600], "stage": stage,
           "higher_is_better": True, "elapsed_s": round(time.time() - STATE["t0"], 1)}
    rec.update(extra)
    return json.dumps(rec, separators=(",", ":"))


def _nccl_log_tail(limit=1500):
    """Tail of the NCCL_DEBUG=WARN side files of this run (multi-rank runs point NCCL_DEBUG_FILE into gpurun_out/)."""
    import glob
    pat = os.environ.get("UOC_NCCL_LOG_GLOB")
    if not pat:
        return None
    out = []
    for p in sorted(glob.glob(pat))[:16]:
        try:
            txt = open(p, errors="replace").read().strip()
        except OSError:
            continue
        if txt:
            out.append(f"{os.path.basename(p)}: {txt[-300:]}")
    return "\n".join(out)[-limit:] or None


def emit_error(stage, err):
    """Rank 0 (or a single process) writes the error record once, to the duplicate of the original stdout."""
    if STATE["emitted"] or STATE["rank"] != 0:
        return
    STATE["emitted"] = True
    line = error_line(stage, err, STATE["world"], nccl_log=_nccl_log_tail())
    fd = STATE["json_fd"] if STATE["json_fd"] is not None else 1
    try:
        os.write(fd, (line + "\n").encode())
    except OSError:
        pass


def _stage():
    """The stage an error record names: inside the timed region, 'gather' once this rank's frame block is done."""
    st, tm = STATE["stage"], STATE.get("timing") or {}
    return "gather" if st == "timed" and "compute_s" in tm and "gather_s" not in tm else st


def _on_sigterm(signum, frame):
    # torch.distributed.run terminates the surviving ranks when one rank dies: rank 0 still owes the driver its record
    emit_error(_stage(), f"terminated by signal {signum} (the launcher stops all ranks when one rank fails); "
                         f"this rank was in stage '{_stage()}'")
    os._exit(143)


def relaunch_under_torchrun(n):
    """`python bench.py --gpus N` without a launcher: spawn the N ranks ourselves (one process per GPU) and make sure ONE
    JSON line comes out whatever happens to them: rank 0's line is passed through; if the ranks exit non-zero (or exceed
    $UOC_BENCH_TIMEOUT seconds, default 3600) without one, the launcher writes the error record itself."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    limit = float(os.environ.get("UOC_BENCH_TIMEOUT", "3600"))
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, start_new_session=True)
    seen = []

    def pump():
        for raw in proc.stdout:
            txt = raw.decode(errors="replace")
            if txt.lstrip().startswith("{") and '"metric"' in txt:
                seen.append(txt)
            sys.stdout.write(txt)
            sys.stdout.flush()
    t = threading.Thread(target=pump, daemon=True)
    t.start()
    try:
        rc = proc.wait(timeout=limit)
        why = f"the ranks exited with code {rc}"
    except subprocess.TimeoutExpired:
        import signal
        os.killpg(proc.pid, signal.SIGTERM)
        try:
            proc.wait(timeout=10)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.wait()
        rc, why = 124, f"no result after {limit:.0f} s: the ranks were stopped"
    t.join(timeout=5)
    if rc != 0 and not seen:
        print(error_line("launch", why + " and rank 0 left no record", n, nccl_log=_nccl_log_tail()), flush=True)
    return rc if rc != 0 or seen else 1


def numa_pin(device_index, local_rank, local_world):
    """Pins this rank to the cores of its GPU's NUMA node (its share of them when several ranks sit on one node), so that the
    event-driven host loop, torch's copy threads and the frame-synthesis workers of a rank stay next to its GPU and the ranks
    do not wander over each other's cores.  Best effort: returns {'numa_node', 'cpus'} or None (no sysfs entry, no rights)."""
    try:
        props = torch.cuda.get_device_properties(device_index)
        bdf = f"{props.pci_domain_id:04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}.0"
        node = int(open(f"/sys/bus/pci/devices/{bdf}/numa_node").read())
        if node < 0:
            return None
        cpus = []
        for part in open(f"/sys/devices/system/node/node{node}/cpulist").read().strip().split(","):
            a, _, b = part.partition("-")
            cpus += list(range(int(a), int(b or a) + 1))
        allowed = sorted(set(cpus) & set(os.sched_getaffinity(0)))
        # ranks whose GPUs share this node split its cores evenly (the same computation on every rank)
        mates = []
        for i in range(local_world):
            try:
                p = torch.cuda.get_device_properties(i)
                n_i = int(open(f"/sys/bus/pci/devices/{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0/numa_node").read())
            except Exception:      # noqa: BLE001
                n_i = -1
            if n_i == node:
                mates.append(i)
        if device_index in mates and len(mates) > 1:
            share = max(2, len(allowed) // len(mates))
            k = mates.index(device_index)
            allowed = allowed[k * share:(k + 1) * share] or allowed
        if len(allowed) < 2:
            return None
        os.sched_setaffinity(0, allowed)
        return {"numa_node": node, "cpus": len(allowed)}
    except Exception:          # noqa: BLE001 - best effort
        return None


def stub_frame_fn(h, w):
    """CPU stand-in for the two-stage frame function (tests of the launcher / sharding / JSON plumbing only; selected
    by --stub, never on a GPU run): a deterministic label map that consumes the per-frame RNG like the real path."""
    def fn(g):
        first = np.random.randint(0, h * w)
        m = torch.full((h, w), g % 200, dtype=torch.int32)
        m.view(-1)[first] = 250
        return m
    fn.roi_counts = []
    return fn


def _fault(stage, rank, args):
    """Test hook of the CPU launcher tests (honoured only with --stub): UOC_BENCH_FAULT="<rank>:<stage>:<kind>" makes that rank
    raise / hang / die (SIGKILL) when it reaches that stage."""
    spec = os.environ.get("UOC_BENCH_FAULT", "")
    if not spec or not args.stub:
        return
    r, st, kind = spec.split(":")
    if int(r) != rank or st != stage:
        return
    if kind == "raise":
        raise RuntimeError(f"injected fault: rank {rank} raises in stage {stage}")
    if kind == "hang":
        time.sleep(10_000)
    if kind == "exit":
        os.kill(os.getpid(), 9)


def _watch_sigterm():
    """SIGTERM must produce the error record even while the main thread is blocked inside a collective / the rendezvous
    (a Python-level signal handler only runs between bytecodes): the C-level handler writes to a wake-up pipe and a daemon
    thread reading it emits the record and leaves."""
    import signal
    r, w = os.pipe()
    os.set_blocking(w, False)
    signal.set_wakeup_fd(w, warn_on_full_buffer=False)
    signal.signal(signal.SIGTERM, lambda *a: None)

    def waiter():
        os.read(r, 1)
        _on_sigterm(15, None)
    threading.Thread(target=waiter, daemon=True).start()


def main():
    try:
        return _main()
    except BaseException as e:      # noqa: BLE001 - every failure must leave the one JSON line behind
        if isinstance(e, SystemExit) and e.code in (0, None):
            raise
        import traceback
        traceback.print_exc()
        emit_error(_stage(), f"{type(e).__name__}: {e}")
        try:
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:           # noqa: BLE001
            pass
        return 1


def _main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64, help="frames per GPU (weak scaling)")
    ap.add_argument("--frames", type=int, default=0,
                    help="strong scaling: this many frames in total, sharded in contiguous blocks over the GPUs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline figure: PCIe-inclusive, latency, sustained, profiled passes "
                         "(roofline, kernel shares), CPU baseline + parity, and write the side file with the full record")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write the label map of the last timed frame to DIR/label_map.npy (float32)")
    ap.add_argument("--cpu-frames", type=int, default=3, help="with --full: frames for the CPU baseline + parity (0 = skip)")
    ap.add_argument("--profile-steps", type=int, default=4, help="with --full: launch sets in the profiled pass (0 = skip)")
    ap.add_argument("--sustained-seconds", type=float, default=10.0, help="with --full: sustained leg at N=1 (0 = skip)")
    ap.add_argument("--inflight", type=int, default=int(os.environ.get("UOC_FRAMES_IN_FLIGHT", "3")),
                    help="streams per GPU, each working on one launch set of --frames-per-launch frames (runner._run_block_pipelined)")
    ap.add_argument("--frames-per-launch", type=int, default=int(os.environ.get("UOC_FRAMES_PER_LAUNCH", "4")),
                    help="frames batched into one set of launches per stage (fcn.test_dataset.FrameGroupJob)")
    ap.add_argument("--skip-pcie", action="store_true", help="with --full: skip the PCIe-inclusive leg (profiling runs)")
    ap.add_argument("--skip-latency", action="store_true", help="with --full: skip the one-frame-at-a-time latency leg (profiling runs)")
    ap.add_argument("--cpu-baseline-only", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-out", default="", help=argparse.SUPPRESS)
    ap.add_argument("--split-precision", action="store_true",
                    help="EXPERIMENT, never the headline: plane GEMMs in split precision (bf16 x 3, fp32 accumulation); the line "
                         "then says dtype 'bf16x3' and carries an 'experiment' key")
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dist-timeout", type=float, default=float(os.environ.get("UOC_BENCH_DIST_TIMEOUT", "300")),
                    help="seconds the rendezvous and every collective may take before the run fails with an error record")
    args = ap.parse_args()
    if args.cpu_baseline_only > 0:
        print(json.dumps(cpu_baseline(args.cpu_baseline_only, args.cpu_out)), flush=True)
        return 0

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return relaunch_under_torchrun(args.gpus)

    # ONE JSON line on stdout: libraries write to fd 1 too (RCCL prints a "Librccl path" banner), so the process's fd 1 is
    # pointed at stderr for the whole run and the JSON line goes to a duplicate of the original stdout at the end
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    STATE.update(json_fd=json_fd, rank=rank, world=world, stage="init")
    if rank == 0 and world > 1:
        _watch_sigterm()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    stub = args.stub
    strong = args.frames > 0
    total = args.frames if strong else args.steps * world
    # host-side inputs first: big blocks are generated by forked workers, and forking is only clean before this process
    # has a HIP context or RCCL threads
    host = None if stub else host_frames(*_block(total, rank, world))
    if stub:
        device, backend, h, w = torch.device("cpu"), "gloo", 12, 16
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a ROCm device: the product path has no CPU fallback")
        # UOC_BENCH_ONE_DEVICE=1 + UOC_BENCH_BACKEND=gloo (tests only): every rank on GPU 0, label maps gathered through
        # gloo (staged through the host by runner.run_sharded) — the REAL frame function at world size > 1 on a box with
        # one GPU (RCCL refuses two ranks on one device); the driver's multi-GPU runs use neither knob
        dev_index = 0 if os.environ.get("UOC_BENCH_ONE_DEVICE") == "1" else local_rank
        torch.cuda.set_device(dev_index)
        device, backend, h, w = torch.device("cuda", dev_index), os.environ.get("UOC_BENCH_BACKEND", "nccl"), H, W
    use_dist = world > 1 or os.environ.get("UOC_BENCH_FORCE_DIST") == "1"   # FORCE: exercise the RCCL path on 1 GPU
    pinned = None
    if not stub and world > 1 and os.environ.get("UOC_BENCH_PIN", "1") != "0" and os.environ.get("UOC_BENCH_ONE_DEVICE") != "1":
        pinned = numa_pin(dev_index, local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    if use_dist:
        import datetime
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "nccl" and world > 1:
            # RCCL's warnings of a failing first multi-GPU run go to side files next to the full record
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            os.environ.setdefault("NCCL_DEBUG", "WARN")
            os.environ.setdefault("NCCL_DEBUG_FILE", os.path.join(ROOT, "gpurun_out", f"nccl_{os.environ['MASTER_PORT']}_%h_%p.log"))
            os.environ["UOC_NCCL_LOG_GLOB"] = os.path.join(ROOT, "gpurun_out", f"nccl_{os.environ['MASTER_PORT']}_*.log")
        _fault("init", rank, args)
        kw = {} if stub or backend != "nccl" else {"device_id": device}
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=args.dist_timeout), **kw)
    STATE["stage"] = "setup"
    _fault("setup", rank, args)

    from unseenobjectclustering_amd import runner
    sync = (lambda: None) if stub else torch.cuda.synchronize
    t_setup0 = time.perf_counter()
    if use_dist and not stub and "UOC_CONV_TUNE_CACHE" not in os.environ:
        # ONE tile choice per layer shape for the whole job: rank 0 tunes (its setup frames below) and writes the cache,
        # the other ranks wait at a barrier and load it at their first convolution — every rank then launches identical
        # kernels (the choices are bit-identical in their results either way; this makes the launch shapes identical too)
        os.environ["UOC_CONV_TUNE_CACHE"] = os.path.join(tempfile.gettempdir(), f"uoc_conv_tune_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}.txt")
        if rank == 0 and os.path.exists(os.environ["UOC_CONV_TUNE_CACHE"]):
            os.remove(os.environ["UOC_CONV_TUNE_CACHE"])

    lo, hi = runner.shard_range(total, rank, world)
    assert (lo, hi) == _block(total, rank, world)
    K = (total + world - 1) // world            # frames per GPU = steps
    if stub:
        frame_fn = stub_frame_fn(h, w)
        network = network_crop = samples = None
    else:
        from unseenobjectclustering_amd import _native, networks, synth
        from unseenobjectclustering_amd.fcn.config import cfg
        cfg.device = device
        if args.split_precision:
            cfg.TEST.SPLIT_PRECISION_GEMM = True        # read by SEGNET at construction
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
        network = networks.seg_resnet34_8s_embedding(2, 64, sd).eval()
        network_crop = networks.seg_resnet34_8s_embedding(2, 64, sd).eval()
        samples = [dict(image_color=torch.from_numpy(a).to(device), depth=torch.from_numpy(b).to(device)) for a, b in host]
        frame_fn = runner.two_stage_frame_fn(samples, network, network_crop, first_index=lo,     # global index -> resident sample
                                             frames_per_launch=args.frames_per_launch)

    rank_timing = STATE["timing"] = {}

    def run(nframes_total, gather):
        maps = runner.run_sharded(nframes_total, frame_fn, h, w, device, rank, world, gather, force_collective=use_dist,
                                  inflight=args.inflight, timing=rank_timing)
        return maps.cpu()           # label-map block lands on the host inside the timed region

    # setup (never timed, independent of --warmup): the native weight copies, the conv autotuner's choice for every layer
    # shape, and — because the stage-2 batch size (number of ROIs) differs per frame — the first-use work of every batch
    # size (kernel instantiations loading, a tile-height variant's attributes, a tuner lookup).
    # Rank 0 runs its first frames (= the tuning launches) before the others start theirs: they load its choices from the
    # cache file (UOC_CONV_TUNE_CACHE above).  The two barriers below pair up on every rank (also in --stub runs, so that
    # the CPU launcher test covers the ordering).
    if use_dist and rank != 0:
        dist.barrier()                            # rank 0 is tuning; its cache file is complete after its barrier
    if not stub:
        for g in range(lo, min(hi, lo + 2)):          # one frame at a time first: the tuner's timing launches run alone
            np.random.seed(runner.frame_rng_seed(g))
            frame_fn(g)
        sync()
    if use_dist and rank == 0:
        dist.barrier()
    if not stub:
        # ... then the same streams x frames-per-launch path the timed region uses, over (up to) 64 frames of the block
        runner.run_sharded(min(hi - lo, 64), frame_fn, h, w, device, 0, 1, False, inflight=args.inflight)
        del frame_fn.roi_counts[:]
        sync()
        print(f"[bench] rank {rank}: nets built, {hi - lo} frames resident, warming up", file=sys.stderr, flush=True)
    if args.warmup > 0:
        # W frames per GPU through the same code path (collective included).  In strong mode the warm-up shards
        # W*world frames, which are the first W of rank 0's block only when world == 1 — any frames do.
        # (two_stage_frame_fn indexes its resident samples modulo the block length, so any global index is valid)
        runner.run_sharded(min(args.warmup, K) * world, frame_fn, h, w, device, rank, world, use_dist,
                           force_collective=use_dist, inflight=args.inflight).cpu()
    sync()
    if use_dist:
        dist.barrier()
    STATE["stage"] = "timed"
    t0 = time.perf_counter()
    _fault("timed", rank, args)
    maps = run(total, use_dist)
    sync()
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    rank_timing["setup_s"] = t0 - t_setup0
    print(f"[bench] rank {rank}: timed region {dt:.3f}s (this rank: setup {rank_timing['setup_s']:.1f}s, compute "
          f"{rank_timing.get('compute_s', 0.0):.3f}s for {rank_timing.get('frames', 0)} frames, gather "
          f"{rank_timing.get('gather_s', 0.0):.3f}s)", file=sys.stderr, flush=True)
    if pinned is not None:
        rank_timing.update(pinned)          # numa_node / cpus this rank is pinned to
    per_rank = [rank_timing]
    if use_dist:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, {k: round(v, 4) if isinstance(v, float) else v for k, v in rank_timing.items()})
    objects = float(np.mean([int(m.max()) for m in maps[:total]]))
    counts = frame_fn.roi_counts[-(hi - lo):] if frame_fn.roi_counts else []
    rois = float(np.mean(counts)) if counts else 0.0
    if rank == 0 and args.dump_outputs:
        # what a caller of the timed path receives for its last step: the label map of the last frame (rank 0 holds the
        # gathered block), as float32
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "label_map.npy"), maps[total - 1].numpy().astype(np.float32))
    STATE["stage"] = "report"
    # every leg below the timed region runs only with --full: a plain run reports the headline figure alone
    solo = rank == 0 and world == 1 and not stub and args.full
    lead = rank == 0 and not stub and args.full       # rank 0 also fills roofline / cpu_baseline / parity of a multi-GPU run (after the gather)

    pcie = None
    if solo and not args.skip_pcie:
        # informative only (never `value`): the frames as a capture pipeline hands them over — RAW uint8 BGR + uint16
        # millimetre depth in pinned host memory (1.5 MB instead of 7.4 MB of float tensors per frame), uploaded inside
        # the timed region and turned into the network inputs on the device (uoc_prep_rgbd, tools/test_images.py:96-133).
        # The quantised inputs are not bit-identical to the resident float frames, so this leg is timed, not compared.
        from unseenobjectclustering_amd import io as uio
        cam = dict(synth.DEMO_CAMERA)
        mean = (synth.PIXEL_MEANS / 255.0).astype(np.float32)
        hs = []
        for a, b in host:
            bgr = np.clip(np.rint((a[0].transpose(1, 2, 0) + mean) * 255.0), 0, 255).astype(np.uint8)
            mm = np.clip(np.rint(b[0, 2] * 1000.0), 0, 65535).astype(np.uint16)
            d = uio.make_sample_raw(bgr, mm, cam)
            d["image_u8"], d["depth_u16"] = d["image_u8"].pin_memory(), d["depth_u16"].pin_memory()
            hs.append(d)
        fn2 = runner.two_stage_frame_fn(hs, network, network_crop, frames_per_launch=args.frames_per_launch)
        # untimed: the first use of the raw-sample path on EVERY stream (allocator pools of the uint8 / uint16 staging tensors, the
        # preparation kernel), two launch sets per stream like the main leg's warm-up
        runner.run_sharded(min(total, 2 * args.inflight * args.frames_per_launch), fn2, h, w, device, 0, 1, False, inflight=args.inflight)
        sync()
        t1 = time.perf_counter()
        runner.run_sharded(total, fn2, h, w, device, 0, 1, False, inflight=args.inflight).cpu()
        sync()
        pcie = round(total / (time.perf_counter() - t1), 3)

    latency = None
    if solo and not args.skip_latency:
        # BASELINE configs[3] read literally ("batch=1"): ONE frame at a time on one stream, host waiting for each result
        # (round 6: the ROI ordering runs on the device, so a frame has ONE mid-frame host wait — the ROI count — and the final read)
        # Untimed pass over the SAME frames first (round 6): a frame's stage-2 launches are shaped by its ROI count, and the first
        # one-frame-at-a-time use of a count pays one-time work (tuner lookups for that batch size, a tile variant's attributes,
        # workspace growth) that the two warm-up frames of round 5 did not cover — 8.05 instead of 7.78 ms (scripts/latency_state.py).
        nlat, reps = min(hi - lo, 12), 2
        for g in range(lo, lo + nlat):
            np.random.seed(runner.frame_rng_seed(g))
            frame_fn(g).cpu()
        sync()
        t1 = time.perf_counter()
        for _ in range(reps):
            for g in range(lo, lo + nlat):
                np.random.seed(runner.frame_rng_seed(g))
                frame_fn(g).to(torch.uint8).cpu()
        sync()
        el = (time.perf_counter() - t1) / reps
        latency = {"frames_per_launch": 1, "streams": 1, "frames": nlat, "repetitions": reps, "ms_per_frame": round(1e3 * el / nlat, 3),
                   "frames_per_s": round(nlat / el, 3)}
        del frame_fn.roi_counts[-(1 + reps) * nlat:]

    sustained = None
    if solo and args.sustained_seconds > 0:
        sampler = SmiSampler(local_rank)
        sampler.start()
        sync()
        t1 = time.perf_counter()
        done = 0
        while time.perf_counter() - t1 < args.sustained_seconds:
            runner.run_sharded(total, frame_fn, h, w, device, 0, 1, False, inflight=args.inflight).cpu()
            done += total
        sync()
        el = time.perf_counter() - t1
        smp = sampler.stop()
        sustained = {"seconds": round(el, 2), "frames": done, "frames_per_s": round(done / el, 3),
                     "sclk_mhz": [s.get("sclk_mhz") for s in smp], "power_w": [s.get("power_w") for s in smp]}

    # ---- profiled pass (HIP events around every launch; separate from the timed region) ----
    roof, kernels = None, []
    if lead and args.profile_steps > 0:
        # the launch shapes of the timed region (launch sets of --frames-per-launch frames), but one launch set at a time
        # on one stream: the HIP events around a launch then time that kernel alone
        nprof = min(hi - lo, args.profile_steps * max(1, args.frames_per_launch))
        _native.prof_enable(True)
        if args.frames_per_launch > 1:
            runner.run_sharded(nprof, frame_fn, h, w, device, 0, 1, False, inflight=1)
        else:
            for g in range(lo, lo + nprof):
                np.random.seed(runner.frame_rng_seed(g))
                frame_fn(g)
        sync()
        rep = _native.prof_report()
        _native.prof_enable(False)
        tot = sum(r["total_ms"] for r in rep) or 1.0
        for r in sorted(rep, key=lambda r: -r["total_ms"]):
            sec = r["total_ms"] / 1e3
            kernels.append({"kernel": r["kernel"], "launches_per_frame": r["launches"] / nprof,
                            "avg_us": round(1e3 * r["total_ms"] / r["launches"], 2),
                            "gpu_time_share": round(r["total_ms"] / tot, 4),
                            "tflops": round(r["flops"] / sec / 1e12, 2), "gbs": round(r["bytes"] / sec / 1e9, 1)})
        by_shape = []
        for r in rep:          # per-launch-shape rows of the convolution classes (tag = GEMM rows, Cin, Cout, dilation)
            for sh in r.get("shapes", []):
                if not r["kernel"].startswith(("wino", "conv")):
                    continue
                us = 1e3 * sh["total_ms"] / sh["launches"]
                factor = 0.25 if r["kernel"] == "wino4_gemm" else (16.0 / 36.0 if r["kernel"] == "wino_gemm" else 1.0)
                by_shape.append({"kernel": r["kernel"], "rows": sh["tag"][0], "cin": sh["tag"][1], "cout": sh["tag"][2],
                                 "dilation": sh["tag"][3], "launches": sh["launches"], "avg_us": round(us, 1),
                                 "algorithmic_tflops": round(sh["flops"] / sh["total_ms"] / 1e9, 1),
                                 "executed_tflops": round(factor * sh["flops"] / sh["total_ms"] / 1e9, 1),
                                 "algorithmic_gbs": round(sh["bytes"] / sh["total_ms"] / 1e6, 1)})
                if r["kernel"] == "wino4_gemm":   # every MFMA the kernel issues, partial 4x4 tiles included: 72 planes (two branches) of [rows x Cin] x [Cin x Cout]
                    by_shape[-1]["matrix_pipe_tflops"] = round(72 * 2.0 * sh["tag"][0] * sh["tag"][1] * sh["tag"][2] * sh["launches"] / sh["total_ms"] / 1e9, 1)
        by_shape.sort(key=lambda d: -d["avg_us"] * d["launches"])
        clustering_by_shape = []      # hc_iter: tag = [pixels, fields, virtual blocks, physical blocks per field]; fps: [pixels, fields, blocks per field, pixels per lane]
        for r in rep:
            if r["kernel"] in ("hc_iter", "fps_step"):
                for sh in r.get("shapes", []):
                    clustering_by_shape.append({"kernel": r["kernel"], "tag": sh["tag"], "launches": sh["launches"],
                                                "avg_us": round(1e3 * sh["total_ms"] / sh["launches"], 1),
                                                "tflops": round(sh["flops"] / sh["total_ms"] / 1e9, 1)})
        dom = max(rep, key=lambda r: r["total_ms"])
        sec = dom["total_ms"] / 1e3
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "traffic.json")   # PMC-derived HBM bytes per launch, if collected
        if os.path.exists(tpath):
            traffic = json.load(open(tpath)).get(dom["kernel"])
        if dom["kernel"].startswith(("conv", "wino_gemm", "wino4_gemm")) or dom["kernel"] in ("hc_iter", "assign"):   # MFMA-bound classes
            ach = dom["flops"] / sec / 1e12
            roof = {"kernel": dom["kernel"], "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_FP32_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(ach / PEAK_FP32_TFLOPS, 4), "traffic": traffic,
                    "algorithmic_bytes": round(dom["bytes"] / dom["launches"]),   # per launch, like `traffic` (PMC): the ratio is the re-read factor
                    "avg_launch_us": round(1e3 * dom["total_ms"] / dom["launches"], 2),
                    "frames_per_launch": max(1, args.frames_per_launch),
                    "by_shape": [d for d in by_shape if d["kernel"] == dom["kernel"]]}
            if dom["kernel"] == "wino4_gemm":
                # algorithmic = the direct 3x3 convolution's flops; Winograd F(4x4,3x3) issues 36/144 of
                # them to the matrix pipe (tile padding not counted: it is wasted work, not achieved work)
                roof["algorithmic_tflops"] = roof["achieved"]
                roof["algorithmic_frac"] = roof["frac"]
                roof["achieved"] = round(ach * 0.25, 2)
                roof["frac"] = round(ach * 0.25 / PEAK_FP32_TFLOPS, 4)
                pipe = sum(72 * 2.0 * d["rows"] * d["cin"] * d["cout"] * d["launches"] for d in roof["by_shape"]) / sec / 1e12
                roof["matrix_pipe_tflops"] = round(pipe, 2)
                roof["matrix_pipe_frac"] = round(pipe / PEAK_FP32_TFLOPS, 4)
                roof["note"] = ("Winograd F(4x4,3x3): achieved = MFMA flops executed for real outputs (36/144 of the direct "
                                "conv's); matrix_pipe_* = every MFMA issued, the padded rows of partial 4x4 tiles included (7 % "
                                "at 60x80, 31 % on the 7x7 / 14x14 phase images of the 28x28 crop features); algorithmic_* = "
                                "SURVEY 8(d) direct-conv flops over the same time")
            if dom["kernel"] == "wino_gemm":
                # the prof class counts the ALGORITHMIC (direct 3x3) flops; Winograd F(2x2,3x3) issues 16/36 of them
                # to the matrix pipe.  `achieved` / `frac` are the flops the pipe really executes (a fraction of a
                # roofline cannot exceed 1); the algorithmic rate is reported next to them.
                roof["algorithmic_tflops"] = roof["achieved"]
                roof["algorithmic_frac"] = roof["frac"]
                roof["achieved"] = round(ach * 16.0 / 36.0, 2)
                roof["frac"] = round(ach * 16.0 / 36.0 / PEAK_FP32_TFLOPS, 4)
                roof["note"] = ("Winograd F(2x2,3x3): achieved = MFMA flops executed (16/36 of the direct conv's); "
                                "algorithmic_* = SURVEY 8(d) direct-conv flops over the same time")
        else:
            ach = dom["bytes"] / sec / 1e9
            roof = {"kernel": dom["kernel"], "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS,
                    "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": traffic,
                    "algorithmic_bytes": round(dom["bytes"] / dom["launches"]),
                    "avg_launch_us": round(1e3 * dom["total_ms"] / dom["launches"], 2)}

    if roof is not None:
        roof["gpu_time_share"] = round(dom["total_ms"] / tot, 4)
        if roof.get("traffic") is not None:
            # not measured in THIS run: the PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate runs, gfx950 corrections)
            # of scripts/profile_round.sh, committed as profiles/traffic.json next to their tables (profiles/r0N_pmc_traffic.md)
            roof["traffic_source"] = "profiles/traffic.json"

    # ---- the same HIP-event timing inside the SHIPPED schedule (streams x launch sets): a kernel's duration next to the other
    # streams' kernels.  The bandwidth-bound Winograd transforms take 2-3x their solo time there, so their share of the
    # frame is larger than the solo table says.
    kernels_pipe = None
    if lead and args.profile_steps > 0 and args.inflight > 1:
        npipe = min(hi - lo, 2 * args.inflight * max(1, args.frames_per_launch))
        _native.prof_enable(True)
        runner.run_sharded(npipe, frame_fn, h, w, device, 0, 1, False, inflight=args.inflight)
        sync()
        rep2 = _native.prof_report()
        _native.prof_enable(False)
        del frame_fn.roi_counts[-npipe:]
        tot2 = sum(r["total_ms"] for r in rep2) or 1.0
        kernels_pipe = [{"kernel": r["kernel"], "avg_us": round(1e3 * r["total_ms"] / r["launches"], 2),
                         "gpu_time_share": round(r["total_ms"] / tot2, 4), "ms_per_frame": round(r["total_ms"] / npipe, 4)}
                        for r in sorted(rep2, key=lambda r: -r["total_ms"])]

    cpu = parity = None
    if lead and args.cpu_frames > 0:
        with tempfile.TemporaryDirectory() as td:
            out_path = os.path.join(td, "cpu_maps.npz")
            cpu = cpu_baseline_subprocess(min(args.cpu_frames, total), out_path)
            if os.path.exists(out_path):
                parity = parity_report(maps.numpy(), out_path, network, network_crop, device)

    if rank == 0 and os.environ.get("UOC_BENCH_DUMP"):     # tests: the label-map block of the timed region
        np.save(os.environ["UOC_BENCH_DUMP"], maps.numpy())
    if rank == 0:
        workload = (f"configs[3] frames: full two-stage (crop-and-refine) segmentation of single 640x480 RGB-D frames; "
                    f"throughput schedule {args.inflight} streams x {args.frames_per_launch}-frame launch sets "
                    f"(one frame at a time: `latency`)")
        if world > 1 or strong:
            workload += (f"; configs[4]: {total} frames sharded over {world} GPU(s) in contiguous blocks + "
                         f"RCCL all_gather of the uint8 label maps" if use_dist else f"; {total} frames on one GPU")
        line = {
            "metric": METRIC,
            "value": round(total / dt, 3), "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / K, 3), "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "bf16x3" if args.split_precision else "f32", "data": "synthetic" + (" (stub frame function, CPU plumbing test)" if stub else ""),
            "config": {"workload": workload, "frame": "640x480", "seeds": 100, "iters": 10, "crop": 224,
                       "total_frames": total, "frames_per_gpu": K, "collective": bool(use_dist),
                       "frames_in_flight_per_gpu": args.inflight * args.frames_per_launch,
                       "streams_per_gpu": args.inflight, "frames_per_launch": args.frames_per_launch,
                       "mean_final_objects": round(objects, 2), "mean_rois": round(rois, 2)},
            "per_rank": [{k: round(v, 4) if isinstance(v, float) else v for k, v in (r or {}).items()} for r in per_rank],
            "pcie_inclusive_frames_per_s": pcie, "latency": latency, "sustained": sustained,
            "roofline": roof, "frame_roofline": frame_roofline(rois, dt / K) if not stub else None,
            "cpu_baseline": cpu, "parity": parity, "kernels": kernels, "kernels_pipe": kernels_pipe, "conv_by_shape": by_shape if lead and args.profile_steps > 0 else None,
            "clustering_by_shape": clustering_by_shape if lead and args.profile_steps > 0 else None,
        }
        if args.split_precision and line.get("roofline"):
            line["roofline"]["note"] = ("EXPERIMENT: the plane GEMM issues six bf16 MFMA products per fp32 product on the bf16 pipe; `achieved` / "
                                        "`frac` are still computed against the fp32 peak and are NOT a roofline fraction in this mode")
        if args.split_precision:
            line["experiment"] = ("split-precision plane GEMMs (csrc/wino4_split.hip): every fp32 operand as three bf16 terms, six bf16 "
                                  "MFMA products, fp32 accumulation; NOT the shipped default, NOT comparable as `value`")
    else:
        line = None
    if use_dist:
        dist.destroy_process_group()
    if line is not None:
        full_path = write_full_record(line) if args.full else None
        out = compact_line(line, full_path)
        # last thing on stdout (RCCL writes a "Librccl path" banner to stdout while the process group is alive)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out, separators=(",", ":")) + "\n").encode())
    os.close(json_fd)
    return 0


if __name__ == "__main__":
    _rc = main()
    if _rc:                 # a plain fall-through on success: profilers attached to the process finalise more reliably
        sys.exit(_rc)       # than through SystemExit -> Py_Exit
