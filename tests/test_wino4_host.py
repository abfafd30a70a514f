"""CPU check of the Winograd F(4x4,3x3) arithmetic the HIP kernels share (csrc/wino4_math.h is host + device code):
tests/csrc/wino4_host_test.cpp drives the weight / input / output transform bodies with plain loops and compares with
a direct dilated 3x3 convolution in double (partial tiles, every dilation the backbone uses, ragged sizes)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host_program(tmp_path, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / name)
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", exe,
                    os.path.join(ROOT, "tests", "csrc", name + ".cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_wino4_transforms_on_the_host(tmp_path):
    out = run_host_program(tmp_path, "wino4_host_test")
    assert out.count(" ok") == 6, out


def test_wino4_skipping_plan_on_the_host(tmp_path):
    """The plan with which partial tiles skip frequency planes, at 1/8 maps down to one pixel (inputs of 8x8 .. 16x8, image
    smaller than the dilation, empty phases): the tiles with work are the tile origins with an output inside, each once and in
    its class (11 maps x dilation 1, 2, 4 x batch 1, 3), and five convolutions under that plan match the direct sum."""
    out = run_host_program(tmp_path, "wino4_plan_host_test")
    assert out.count(" ok\n") == 66 + 5 and "FAIL" not in out, out
