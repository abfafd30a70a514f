"""Writes profiles/network_error.md: per case of tests/test_network_fp64_gpu.py the float32 yardstick the test takes its
tolerance from, the GPU network's error (both against the fp64 reference, max norm) and their ratio; the split-precision
network's error on one case next to them, recorded and not asserted.  Needs a GPU.

    python scripts/network_error_report.py [--out profiles/network_error.md]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import network_gpu as NG  # noqa: E402
from tests import network_reference as NR  # noqa: E402
from tests import test_network_fp64_gpu as T  # noqa: E402

SPLIT_CASE = "RGBD_ADD 37x53 B=2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_error.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    rows = [(name, "fp32", *T.measure(dev, name)) for name in NR.CASES]
    split = NG.RawNet(dev, NR.state_dict("RGBD_ADD"), "RGBD_ADD")
    split.set_split_precision(True)
    rows.append((SPLIT_CASE, "split precision (bf16x3 plane GEMMs), not asserted", *T.measure(dev, SPLIT_CASE, net=split)))
    split.close()
    worst = max(rows[:-1], key=lambda r: r[3] / r[2])
    with open(args.out, "w") as f:
        f.write("# The embedding network: GPU error against the float32 yardsticks\n\n")
        f.write("Written by `scripts/network_error_report.py` on " + torch.cuda.get_device_name(0) + ".  Errors are max norms over the\n"
                "unit-norm embeddings against the fp64 reference of the case (the oracle in double); the yardstick is the error of a\n"
                "float32 CPU evaluation of the same network (`tests/network_reference.py`, stored in\n"
                "`tests/golden/network_yardsticks.json`); `tests/test_network_fp64_gpu.py` allows the network " + f"{T.MARGIN:g}" + " x the yardstick.\n"
                "Weights: `synthetic_state_dict(3)`, hostile BN: `network_reference.hostile_bn`; frames: `synth.rgbd_frame`.\n\n")
        f.write("| case | arithmetic | yardstick | GPU error | ratio | max abs(norm - 1) |\n|---|---|---|---|---|---|\n")
        for name, kind, yard, err, norm_err in rows:
            f.write(f"| {name} | {kind} | {yard:.3e} | {err:.3e} | {err / yard:.2f} | {norm_err:.1e} |\n")
        f.write(f"\nLargest ratio of the asserted rows: {worst[3] / worst[2]:.2f} ({worst[0]}).\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
