"""Prints the table of profiles/ms_euclidean_error.md: per hill-climbing case of tests/test_ms_euclidean_stages_gpu.py the
deviation from float64 of the kernel and of the CPU yardsticks (the direct-difference torch float32 restatement, the
16-pixel-tile fp32 norm expansion in six channel orders, float64 one ulp off), and the kernel's ratio to the largest of them
(the test allows K_CLIMB).  Batches are summarised by their worst
field.  Needs a GPU.

    python scripts/ms_euclidean_error.py [--out table.md]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import ms_euclidean_cases as EC  # noqa: E402
from tests import test_ms_euclidean_stages_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["| case | fields | kernel | direct | tiles | ulp | kernel / max(direct, tiles, ulp) |", "|---|---|---|---|---|---|---|"]
    worst = (0.0, "")
    for name, fn in T.climb_cases().items():
        rows = fn(dev)
        ratios = [T.ratio(err, devs) for _, err, devs, _ in rows]
        k = max(range(len(rows)), key=lambda i: ratios[i])
        _, err, devs, _ = rows[k]
        lines.append("| %s | %d | %.2e | %.2e | %.2e | %.2e | %.2f |" % ((name, len(rows), err) + devs + (ratios[k],)))
        worst = max(worst, (ratios[k], name))
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("largest ratio %.2f (%s); K in force %g" % (worst[0], worst[1], EC.K_CLIMB))
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
