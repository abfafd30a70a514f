"""Writes tests/golden/network_yardsticks.json: the float32 yardstick (tests/network_reference.py) of every case of
tests/test_network_fp64_gpu.py.  CPU only; the emulation takes 5 to 25 s per case, which is why the results are stored:
tests/test_network_reference_host.py recomputes the two smallest cases and holds the file to them within 1 %.

    python tests/golden/make_network_yardsticks.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import network_reference as NR  # noqa: E402


def main():
    out = {}
    for name in NR.CASES:
        out[name] = NR.case_yardstick(name)
        print(f"{name}: {out[name]:.6e}", flush=True)
    with open(NR.YARDSTICK_FILE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
