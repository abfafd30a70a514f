"""CPU check of the skipping plan of the Winograd F(4x4,3x3) path (csrc/wino4_math.h is host + device code):
tests/csrc/wino4_skip_host_test.cpp checks the class-major tile order (decode is a bijection, class counts, each plane's row
range), runs the transform bodies over NaN-filled V and M with a GEMM restricted to each plane's range and compares every
stored output bit for bit with the dense plan, and counts the plane GEMM's work items against the cost model's count."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wino4_skipping_plan_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "wino4_skip_host_test")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", exe,
                    os.path.join(ROOT, "tests", "csrc", "wino4_skip_host_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 10 and "FAIL" not in r.stdout, r.stdout
