"""The whole network (csrc/net.hip: BatchNorm fold, layer table, stride-to-dilation switch, buffer rotation, shortcut, the
five modes) against the fp64 reference, under a bar taken from the CPU alone, and the tuner's promise that it never changes
an embedding.

The bar of every case is  GPU error vs fp64 <= MARGIN x yardstick, the yardstick being what a float32 evaluation of the same
network costs on the very case (tests/network_reference.py; stored in tests/golden/network_yardsticks.json because the
emulation takes 5 to 25 s per case, and held to a recomputation by tests/test_network_reference_host.py).  MARGIN is the
project's 4 (tests/test_conv_tiles_gpu.py, conv_reference._accumulate: the matrix core rounds after every product where the
yardstick rounds once per four, which is a factor of two, and a maximum over 1e4 .. 1e5 outputs of an equally long sum in
another order draws from the same distribution).  Nothing here is taken from the GPU.  Measured ratios:
profiles/network_error.md (scripts/network_error_report.py).

The network runs through its raw entry with the output filled with NaN before every call (tests/network_gpu.py).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conv_reference as CR
from tests import network_gpu as NG
from tests import network_reference as NR
from tests.backbone_layers import backbone_layers

pytestmark = pytest.mark.gpu
MARGIN = 4.0
DIRECT_BN = {0: 128, 1: 128, 2: 64, 3: 64}     # the direct kernel's tile families (csrc/conv.hip kCfgs)


@functools.lru_cache(maxsize=None)
def native_net(device, mode, hostile=False):
    return NG.RawNet(device, NR.state_dict(mode, hostile), mode)


@functools.lru_cache(maxsize=None)
def gpu_embedding(device, name):
    """The case's embeddings [B,64|128,H,W] on the CPU."""
    c = NR.CASES[name]
    _, img, depth, _ = NR.case_reference(name)
    return NG.nchw(native_net(device, c["mode"], c["hostile"]).forward(img, depth), c["H"], c["W"])


def measure(device, name, net=None):
    """-> (yardstick, GPU error, max | |embedding| - 1 | outside the pixels the reference itself makes zero), the errors
    against fp64 in max norm.  net: another network for the case's inputs (the report's split-precision row)."""
    c = NR.CASES[name]
    _, img, depth, ref = NR.case_reference(name)
    got = gpu_embedding(device, name) if net is None else NG.nchw(net.forward(img, depth), c["H"], c["W"])
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} outputs are not finite"
    norm = got.double().norm(dim=1)
    norm[ref.norm(dim=1) == 0] = 1.0
    return NR.stored_yardstick(name), CR.max_err(got, ref), (norm - 1).abs().max().item()


def check_case(device, name):
    yard, err, norm_err = measure(device, name)
    print(f"network {name}: yardstick {yard:.3e} GPU error {err:.3e} ratio {err / yard:.2f}, |norm - 1| {norm_err:.2e}")
    assert norm_err < 1e-5, norm_err
    assert err <= MARGIN * yard, f"{name}: GPU error {err:.3e} > {MARGIN} x yardstick {yard:.3e}"


@pytest.mark.parametrize("name", list(NR.CASES))
def test_network_vs_fp64(device, name):
    """Shapes x modes (8x8: the 1/8 map is one pixel, every dilated tap but the centre is outside, every Winograd tile is
    partial), the hostile BatchNorm weights, and a batch of three."""
    check_case(device, name)


def test_case_table_is_the_stated_one():
    names = set(NR.CASES)
    assert {f"RGBD_ADD {s} B={b}" for s, b in (("8x8", 1), ("16x8", 1), ("9x15", 2), ("37x53", 2), ("77x93", 1), ("37x53", 3))} <= names
    assert {f"{m} {s} B=2" for m in ("COLOR", "DEPTH", "RGBD_CAT", "RGBD_EARLY") for s in ("9x15", "37x53")} <= names
    assert {f"{m} 37x53 B=2 hostile BN" for m in ("RGBD_ADD", "RGBD_CAT")} <= names
    assert len(names) == 16


@pytest.mark.parametrize("shape", [(37, 53, (41, 42, 43)), (224, 224, (61, 62, 63, 64, 65))], ids=["37x53 B=3", "224x224 B=5"])
def test_frame_in_a_batch_equals_frame_alone(device, shape):
    """Bit for bit: no summation order depends on a frame's launch-set mates, whatever tile the batch size picks."""
    H, W, seeds = shape
    net = native_net(device, "RGBD_ADD")
    img, depth = NR.frames(seeds, H, W)
    batch = net.forward(img, depth)
    assert torch.isfinite(batch).all()
    assert not torch.equal(batch[0], batch[1])                   # different frames
    for i in range(len(seeds)):
        alone = net.forward(img[i:i + 1], depth[i:i + 1])
        same = torch.equal(batch[i], alone[0])
        assert same, f"{H}x{W}: frame {i} of {len(seeds)} differs from the frame alone in {int((batch[i] != alone[0]).sum())} " \
            f"values, max |diff| {(batch[i] - alone[0]).abs().max().item():.3e}"


# ---- the tuner never changes an embedding -----------------------------------------------------------------------------------
TUNER_ENV = ("UOC_CONV_AUTOTUNE", "UOC_CONV_TUNE_CACHE", "UOC_CONV_VERBOSE")


def direct_layer_keys():
    """The tuner's key (G, B, H, W, Cin, Cout, K, stride, dil) of every layer of the child's two runs that the direct kernel
    runs and the tuner therefore sees: the strided 3x3, the three shortcuts and fc."""
    keys = []
    for H, W, seeds in NG.TUNER_SHAPES:
        for (h, w, cin, cout, K, s, d) in backbone_layers(H, W):
            if not NR.runs_winograd(cin, cout, K, s):
                keys.append((2, len(seeds), h, w, cin, cout, K, s, d))
    assert len(keys) == 10 and len(set(keys)) == 10
    return keys


def cache_line(key, family):
    return " ".join(str(v) for v in key + (family, 1)) + "\n"


def run_variant(tmp_path, tag, env_changes):
    """One fresh child under the variant's environment -> (the bytes of its two embedding files, its tuning reports on
    stderr).  Any failure of the child fails the test here, so nothing further starts."""
    out = tmp_path / tag
    out.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in TUNER_ENV}
    env.update(env_changes)
    env["UOC_CONV_VERBOSE"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(NG.__file__), str(out)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"variant {tag}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    files = sorted(os.listdir(out))
    assert files == sorted(f"embed_{H}x{W}.npy" for H, W, _ in NG.TUNER_SHAPES), files
    tuned = [l for l in r.stderr.splitlines() if l.startswith("[uoc] conv ")]
    return tuple((out / f).read_bytes() for f in files), tuned


def test_tuner_never_changes_an_embedding(tmp_path):
    """Static model, tuner, a cache being written, the cache being read, every direct-kernel family forced through a
    hand-written cache, and a cache with inadmissible, truncated and out-of-range lines in front: the same bytes."""
    keys = direct_layer_keys()
    base, tuned = run_variant(tmp_path, "a_static", {"UOC_CONV_AUTOTUNE": "0"})
    assert tuned == []
    assert np.isfinite(np.load(tmp_path / "a_static" / "embed_37x53.npy")).all()

    def same(tag, got):
        for (H, W, _), a, b in zip(NG.TUNER_SHAPES, base, got):
            assert a == b, f"variant {tag}: the {H}x{W} embeddings differ from the static model's"

    got, tuned = run_variant(tmp_path, "b_default", {})
    assert len(tuned) == len(keys), tuned                         # the tuner did run, once per direct layer shape
    same("b_default", got)

    cache = tmp_path / "tune_cache.txt"
    got, tuned = run_variant(tmp_path, "c_cache_written", {"UOC_CONV_TUNE_CACHE": str(cache)})
    same("c_cache_written", got)
    written = cache.read_text()
    lines = [tuple(int(v) for v in l.split()) for l in written.splitlines()]
    assert len(tuned) == len(keys) and sorted(l[:9] for l in lines) == sorted(keys), written
    assert all(len(l) == 11 and l[5] % DIRECT_BN[l[9]] == 0 for l in lines), written

    got, tuned = run_variant(tmp_path, "d_cache_read", {"UOC_CONV_TUNE_CACHE": str(cache)})
    same("d_cache_read", got)
    assert tuned == [] and cache.read_text() == written          # every choice came from the file, which did not grow

    for family, bn in DIRECT_BN.items():
        forced = [k for k in keys if k[5] % bn == 0]
        assert forced
        path = tmp_path / f"family{family}.txt"
        path.write_text("".join(cache_line(k, family) for k in forced))
        got, tuned = run_variant(tmp_path, f"e_family{family}", {"UOC_CONV_TUNE_CACHE": str(path)})
        same(f"e_family{family}", got)
        assert len(tuned) == len(keys) - len(forced), (family, tuned)      # the forced layers were taken from the file

    # (f) lines the loader must drop, in front of the valid ones: a family whose BN = 128 does not divide Cout = 64 (the fc
    # layers), non-positive dimensions, families out of range, a line cut short.  launch_tile refuses such a pair, choose()
    # falls back to the static choice and the loader drops the line, so the worst outcome is an error code before a launch.
    fc = [k for k in keys if k[5] == 64]
    assert len(fc) == 2
    bad = [cache_line(k, f) for k in fc for f in (0, 1)]
    bad += [cache_line(keys[0][:2] + (0,) + keys[0][3:], 2), cache_line((2, -2) + keys[1][2:], 3),
            cache_line(keys[2][:5] + (0,) + keys[2][6:], 2), cache_line(keys[3], 4), cache_line(keys[4], -1),
            cache_line(keys[5], 1 << 20), " ".join(str(v) for v in keys[6][:5]) + "\n"]
    path = tmp_path / "hostile_cache.txt"
    path.write_text("".join(bad) + written)
    got, tuned = run_variant(tmp_path, "f_bad_lines", {"UOC_CONV_TUNE_CACHE": str(path)})
    same("f_bad_lines", got)
    assert tuned == [] and path.read_text() == "".join(bad) + written      # the valid lines behind the bad ones all counted
