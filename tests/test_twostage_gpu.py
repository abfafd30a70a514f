"""GPU parity of the two-stage glue kernels and of test_sample end to end (through the C ABI)
against golden vectors captured from the reference's own functions.  Integer outputs
(filtered maps, ROI boxes, mask crops, refined maps) are bit-exact; resampled crops 1e-5."""
import os

import numpy as np
import pytest
import torch

from oracle import mean_shift_oracle as O
from tests.golden.cases import (GLUE_CASES, E2E_CASES, RNG_SEED, glue_inputs, crop_cluster_labels,
                                e2e_stub_features)
from unseenobjectclustering_amd import synth
from unseenobjectclustering_amd.fcn import test_dataset as TD
from unseenobjectclustering_amd.fcn.config import cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "glue.npz"))


@pytest.mark.parametrize("name", list(GLUE_CASES))
def test_glue_matches_reference_golden(golden, device, name):
    cfg.device = device
    c = GLUE_CASES[name]
    img, lab, depth, gt = glue_inputs(c)
    imgd, depthd = img.to(device), depth.to(device)
    filt = TD.filter_labels_depth(lab, depthd, 0.8)
    assert filt.dtype == lab.dtype and filt.device == lab.device
    assert np.array_equal(filt.numpy().astype(np.uint8), golden[name + "/filtered"])

    rgb_c, mask_c, rois, depth_c = TD.crop_rois(imgd, filt.clone(), depthd)
    K = rgb_c.shape[0]
    assert rgb_c.shape == (K, 3, 224, 224) and depth_c.shape == (K, 3, 224, 224) and mask_c.shape == (K, 224, 224)
    assert np.array_equal(rois.cpu().numpy().astype(np.int32).reshape(-1, 4), golden[name + "/rois"].reshape(-1, 4))
    assert np.array_equal(np.packbits(mask_c.cpu().numpy().astype(np.uint8), axis=None), golden[name + "/mask_crops"])
    if K == 0:
        return
    pos = golden[name + "/crop_pos"]
    assert np.abs(rgb_c.reshape(K, -1)[:, pos].cpu().numpy() - golden[name + "/rgb_crops_s"]).max() < 1e-5
    assert np.abs(depth_c.reshape(K, -1)[:, pos].cpu().numpy() - golden[name + "/depth_crops_s"]).max() < 1e-5
    assert np.abs(rgb_c.double().sum(dim=(1, 2, 3)).cpu().numpy() - golden[name + "/rgb_crops_sum"]).max() < 1e-2

    labels_c = crop_cluster_labels(c, gt, rois.cpu()).to(device)
    refined, labels_c2 = TD.match_label_crop(filt, labels_c, mask_c, rois, depth_c)
    assert refined.shape == filt.shape and refined.dtype == torch.float32
    assert np.array_equal(refined.cpu().numpy().astype(np.uint8), golden[name + "/refined"])
    assert np.array_equal(labels_c2.cpu().numpy().astype(np.int8), golden[name + "/labels_crop_out"])


@pytest.mark.parametrize("name", list(E2E_CASES))
def test_test_sample_matches_reference_golden(golden_dir, device, name):
    """test_sample with stub networks that return fixed embedding fields: exercises the device
    pipeline, the RNG coupling (1 + K draws) and the ROI batching against the reference's result."""
    cfg.device = device
    g = np.load(os.path.join(golden_dir, "e2e.npz"))
    c = E2E_CASES[name]
    fr = synth.rgbd_frame(c["seed"], 480, 640, c["objects"])
    sample = dict(image_color=torch.from_numpy(fr["image_color"]), depth=torch.from_numpy(fr["depth"]))
    net = lambda img, label, depth: e2e_stub_features(c["seed"], 480, 640, c["objects"] + 2).to(device)
    net_crop = lambda rgb, label, depth: torch.cat(
        [e2e_stub_features(1000 + 10 * c["seed"] + k, 224, 224, 2 + k % 3) for k in range(rgb.shape[0])]).to(device)
    np.random.seed(RNG_SEED)
    out_label, refined = TD.test_sample(sample, net, net_crop)
    assert out_label.device.type == "cpu" and out_label.dtype == torch.float32 and out_label.shape == (1, 480, 640)
    assert refined.device.type == "cpu" and refined.dtype == torch.float32 and refined.shape == (1, 480, 640)
    assert O.labels_equal_up_to_permutation(out_label.numpy(), g[name + "/out_label"])
    assert np.array_equal(out_label.numpy().astype(np.uint8), g[name + "/out_label"])
    assert O.labels_equal_up_to_permutation(refined.numpy(), g[name + "/refined"])
    assert np.array_equal(refined.numpy().astype(np.uint8), g[name + "/refined"])


def test_no_objects_returns_none(device):
    cfg.device = device
    fr = synth.rgbd_frame(50, 120, 160, 0)
    sample = dict(image_color=torch.from_numpy(fr["image_color"]), depth=torch.from_numpy(fr["depth"]))
    one = torch.zeros(1, 64, 120, 160, device=device)
    one[:, 0] = 1.0
    out_label, refined = TD.test_sample(sample, lambda i, l, d: one, lambda i, l, d: one)
    assert refined is None and float(out_label.abs().max()) == 0.0


def test_test_segnet_loop_writes_mat_files(device, tmp_path):
    """test_segnet (test_dataset.py:271-381): loader loop, per-sample .mat with labels / labels_refined /
    filename (:337-340); dataset name 'osd' selects the 0.8 depth filter (:303-305)."""
    import scipy.io
    cfg.device = device

    class Loader(list):
        class dataset:
            name = "osd_object_test"

    samples = Loader()
    for s in (61, 62):
        fr = synth.rgbd_frame(s, 120, 160, 2)
        samples.append(dict(image_color=torch.from_numpy(fr["image_color"]), depth=torch.from_numpy(fr["depth"]),
                            label=torch.zeros(1, 120, 160), filename="frame%d" % s))

    class Net:
        def __init__(self, seed):
            self.seed = seed

        def eval(self):
            return self

        def __call__(self, img, label, depth):
            B, _, h, w = img.shape
            return torch.cat([e2e_stub_features(self.seed + k, h, w, 3) for k in range(B)]).to(device)

    np.random.seed(3)
    res = TD.test_segnet(samples, Net(70), str(tmp_path), Net(80))
    assert len(res) == 2
    for i in range(2):
        m = scipy.io.loadmat(os.path.join(str(tmp_path), "%06d.mat" % i))
        assert m["labels"].shape == (120, 160) and m["labels_refined"].shape == (120, 160)
        assert np.array_equal(m["labels"], res[i]["labels"])


def test_many_rois_vs_oracle(device):
    """12 objects -> 12 ROIs: more crops than one cooperative farthest-point launch holds (8), so stage 2 runs as
    several launches; label ids up to 12 + the two-way splits of stage 2.  Against the CPU oracle's test_sample."""
    from oracle import glue_oracle as G
    cfg.device = device
    H, W = 240, 320
    lab = np.zeros((H, W), np.int64)
    k = 0
    for by in range(3):
        for bx in range(4):
            k += 1
            lab[20 + by * 70: 20 + by * 70 + 40 + 2 * k, 15 + bx * 78: 15 + bx * 78 + 30 + 3 * bx] = k
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((k + 1, 64)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = centres[lab.reshape(-1)] + np.float32(0.05) * rng.standard_normal((H * W, 64), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    feat = torch.from_numpy(X.astype(np.float32)).view(H, W, 64).permute(2, 0, 1)[None].contiguous()
    fr = synth.rgbd_frame(91, H, W, 2, hole_fraction=0.0)
    img, dep = torch.from_numpy(fr["image_color"]), torch.from_numpy(fr["depth"])
    dep[:, 2] = 1.0 + torch.arange(W, dtype=torch.float32)[None, None, :] / W       # distinct mean depth per ROI
    s1 = lambda i, l, d: feat
    s2 = lambda i, l, d: torch.cat([e2e_stub_features(2000 + j, 224, 224, 2 + j % 2) for j in range(i.shape[0])])
    want_label, want_refined = G.test_sample(img, dep, s1, s2, np.random.RandomState(RNG_SEED))
    assert len(np.unique(want_label.numpy())) == 13
    np.random.seed(RNG_SEED)
    out_label, refined = TD.test_sample(dict(image_color=img, depth=dep), lambda i, l, d: s1(i, l, d).to(device),
                                        lambda i, l, d: s2(i, l, d).to(device))
    assert np.array_equal(out_label.numpy(), want_label.numpy())
    assert np.array_equal(refined.numpy(), want_refined.numpy())
    assert int(refined.max()) >= 12


def test_bench_json_contract(device):
    """bench.py --full prints ONE JSON line with the driver's keys plus the roofline / cpu_baseline objects."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--cpu-frames", "1",
                          "--profile-steps", "1"], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    # the driver keeps only a few KB of output tail (stdout AND stderr): round 3's 22.7 KB line was cut and the record lost
    assert len(lines[0]) < 3000, len(lines[0])
    assert len(out.stderr) < 3000, "stderr shares the driver's output tail with the JSON line"
    d = json.loads(lines[0])
    full = json.load(open(os.path.join(root, d["full"])))
    assert full["value"] == d["value"] and full["conv_by_shape"] and full["kernels"] and full["clustering_by_shape"]
    assert d["latency"]["frames_per_s"] > 1 and d["sustained_frames_per_s"] > 1 and d["pcie_inclusive_frames_per_s"] > 1
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "frames/s" and d["value"] > 1 and abs(d["value"] * d["ms_per_step"] - 1000.0) < 1.0
    assert "workload" in d["config"] and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    f = full["frame_roofline"]
    assert d["frame_roofline"]["hbm_frac"] == f["hbm_frac"]
    assert 0 < f["hbm_frac"] < 1 and 0 < f["mfma_frac"] < 1 and f["rois_per_frame"] >= 1
    assert abs(f["algorithmic_gb"] - (8.98 + 1.43 * f["rois_per_frame"])) < 0.02
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c


def test_batch_of_two_and_no_crop_network(device):
    """test_sample on a batch of 2 (test_dataset.py:247-261: every item is clustered and depth-filtered, only item
    0 is refined) and with network_crop=None (returns (out_label, None))."""
    from oracle import glue_oracle as G
    cfg.device = device
    frs = [synth.rgbd_frame(s, 120, 160, 3) for s in (81, 82)]
    img = torch.from_numpy(np.concatenate([f["image_color"] for f in frs]))
    dep = torch.from_numpy(np.concatenate([f["depth"] for f in frs]))
    s1 = lambda i, l, d: torch.cat([e2e_stub_features(300 + k, 120, 160, 4) for k in range(i.shape[0])])
    s2 = lambda i, l, d: torch.cat([e2e_stub_features(400 + k, 224, 224, 2) for k in range(i.shape[0])])
    want_label, want_refined = G.test_sample(img, dep, s1, s2, np.random.RandomState(RNG_SEED))
    np.random.seed(RNG_SEED)
    out_label, refined = TD.test_sample(dict(image_color=img, depth=dep), lambda i, l, d: s1(i, l, d).to(device),
                                        lambda i, l, d: s2(i, l, d).to(device))
    assert out_label.shape == (2, 120, 160) and refined.shape == (2, 120, 160) and float(refined[1].abs().max()) == 0.0
    assert np.array_equal(out_label.numpy(), want_label.numpy())
    assert np.array_equal(refined.numpy(), want_refined.numpy())
    np.random.seed(RNG_SEED)
    out2, none = TD.test_sample(dict(image_color=img, depth=dep), lambda i, l, d: s1(i, l, d).to(device), None)
    assert none is None and np.array_equal(out2.numpy(), want_label.numpy())


def _order_case(rng, K, S, nan_rate, tie_rate):
    """Random crop clusterings of K ROIs with mean depths that tie and that are NaN (every kept pixel at z = 0)."""
    SS = S * S
    labels = torch.from_numpy(rng.randint(0, 4, size=(K, SS)).astype(np.int32))
    mask = torch.from_numpy((rng.rand(K, S, S) < 0.7).astype(np.float32))
    zval = rng.choice(np.round(rng.rand(max(2, K // 3)) + 0.5, 2), size=K) if tie_rate else rng.rand(K) + 0.5
    depth = torch.zeros(K, 3, S, S)
    for k in range(K):
        depth[k, 2] = 0.0 if rng.rand() < nan_rate else float(zval[k])
    t = TD._native.RoiTable()
    t.K = K
    for k in range(K):
        x0, y0 = rng.randint(0, 40), rng.randint(0, 30)
        t.box[k][0], t.box[k][1], t.box[k][2], t.box[k][3] = x0, y0, x0 + rng.randint(3, 24), y0 + rng.randint(3, 18)
        t.label[k] = k + 1
    return labels, mask, depth, t


@pytest.mark.parametrize("with_depth", [True, False])
def test_device_roi_order_is_pythons_sorted(device, with_depth):
    """uoc_roi_match (round 6: ROI paint order + renumbering on the device) against the host path it replaces — the
    statistics read back, Python's own sorted(key=0-dim tensors, reverse=True), uoc_roi_paste — on random cases with
    tied keys and NaN keys (lib/fcn/test_dataset.py:129-163; NaN: torch.mean of an empty selection, :135).  K < 64 covers
    CPython's short-list algorithm (count_run + binary insertion) that the kernel restates for NaN keys; K >= 64
    without NaN the rank sort; K >= 64 WITH NaN must raise the status flag instead of guessing."""
    cfg.device = device
    rng = np.random.RandomState(11)
    old = cfg.TRAIN.SYN_CROP_SIZE
    cfg.TRAIN.SYN_CROP_SIZE = 8
    H, W = 64, 72
    try:
        cases = [(K, nan, tie) for K in (1, 2, 3, 5, 8, 13, 31, 63) for nan in (0.0, 0.3, 0.9) for tie in (0, 1)]
        cases += [(64, 0.0, 1), (100, 0.0, 0), (127, 0.0, 1)]
        for K, nan_rate, tie in cases:
            for rep in range(3 if K < 64 else 1):
                labels, mask, depth, t = _order_case(rng, K, 8, nan_rate if with_depth else 0.0, tie)
                table = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(device)
                lab_d, mask_d = labels.to(device), mask.to(device)
                dep_d = depth.to(device) if with_depth else None
                want, keep_w = TD._match_host_order(lab_d, mask_d, dep_d, table, K, H, W, device)
                got, keep_g = TD._match_device(lab_d, mask_d, dep_d, table, K, H, W, device, want_keep=True)
                assert not TD._take_order_flag(TD._status_word(device)), (K, nan_rate, tie)
                assert torch.equal(keep_w.cpu(), keep_g.cpu())
                assert torch.equal(want.cpu(), got.cpu()), (K, nan_rate, tie, rep)
        if with_depth:
            labels, mask, depth, t = _order_case(rng, 70, 8, 0.5, 0)
            table = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(device)
            TD._match_device(labels.to(device), mask.to(device), depth.to(device), table, 70, H, W, device)
            assert TD._take_order_flag(TD._status_word(device)), "NaN keys with >= 64 ROIs must be flagged for the host path"
            assert not TD._take_order_flag(TD._status_word(device)), "the flag is cleared by reading it"
            # ... and match_label_crop (the reference-surface entry) takes that path by itself
            rois = torch.tensor([[t.box[k][i] for i in range(4)] for k in range(70)], dtype=torch.float32)
            init = torch.zeros(1, H, W)
            got, _ = TD.match_label_crop(init, labels.view(70, 8, 8).float().to(device), mask.to(device), rois, depth.to(device))
            want, _ = TD._match_host_order(labels.to(device), mask.to(device), depth.to(device), table, 70, H, W, device)
            assert torch.equal(got[0].to(torch.int32).cpu().view(-1), want.cpu())
    finally:
        cfg.TRAIN.SYN_CROP_SIZE = old
