"""Writes profiles/conv_tiles_error.md: per case of tests/test_conv_tiles_gpu.py the float32 yardstick the test takes its
tolerance from, the GPU kernels' error (both against the fp64 reference, max norm) and their ratio.  Needs a GPU.

    python scripts/conv_tile_report.py [--out profiles/conv_tiles_error.md]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_conv_tiles_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_tiles_error.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for algo in (T.DIRECT, T.WINO):
        for c in T.CASES[algo]:
            yard, err = T.measure(dev, c["name"], algo)
            tiles = len(T.run_case(dev, c["name"], algo)[0])
            rows.append((c["name"], f"{T.ALGO_NAME[algo]}, {tiles} tiles bit-identical", yard, err))
    for hw in [(8, 8), (9, 11), (37, 53), (64, 64)]:
        rows.append((f"stem {hw[0]}x{hw[1]}", "direct, stem tile", *T.measure_stem(dev, hw[0], hw[1], 3)))
    for hw in [(9, 11), (37, 53)]:
        rows.append((f"stem {hw[0]}x{hw[1]} early fusion", "direct, stem tile, two passes", *T.measure_stem(dev, hw[0], hw[1], 6)))
    for shape in T.HEAD_SHAPES:
        for mode in T.HEAD_MODES:
            yard, err, _ = T.measure_head(dev, shape, mode)
            rows.append(("head %dx%d -> %dx%d" % shape, f"head, {mode}", yard, err))
    split = []
    for c in T.CASES[T.SPLIT]:
        got, fp32 = T.run_case(dev, c["name"], T.SPLIT), T.run_case(dev, c["name"], T.WINO)
        split.append((c["name"], len(got[0]), T.CR.max_err(got[1], fp32[1]), T.case_data(c["name"])["scale"]))
    with open(args.out, "w") as f:
        f.write("# Convolution tiles, stem and head: GPU error against the float32 yardsticks\n\n")
        f.write("Written by `scripts/conv_tile_report.py` on " + torch.cuda.get_device_name(0) + ".  Errors are max norms against the fp64\n"
                "reference of the case; the yardstick is the error of a float32 CPU evaluation of the same operation\n"
                "(`tests/conv_reference.py`); `tests/test_conv_tiles_gpu.py` allows the kernels " + f"{T.MARGIN:g}" + " x the yardstick.\n\n")
        f.write("| case | algorithm | yardstick | GPU error | ratio |\n|---|---|---|---|---|\n")
        for name, algo, yard, err in rows:
            f.write(f"| {name} | {algo} | {yard:.3e} | {err:.3e} | {err / yard:.2f} |\n")
        f.write("\nThe GEMM kernels sit near ratio 2 because the yardstick rounds once per step of four products while the matrix core\n"
                "rounds after every product: a variant of `conv_reference._accumulate` with one rounding per product (q = 0..3 in turn)\n"
                "gives, on the CPU, the direct kernel's GPU error above to all four digits on D1-D5 and D7.  Four times the roundings is\n"
                "twice the error; no case needed a wider margin.\n")
        f.write("\nSplit-precision plane GEMM against the fp32 Winograd result of the same case (bar: 2e-5 of the output scale):\n\n")
        f.write("| case | tiles bit-identical | max difference | output scale | difference / scale |\n|---|---|---|---|---|\n")
        for name, n, err, scale in split:
            f.write(f"| {name} | {n} | {err:.3e} | {scale:.3f} | {err / scale:.2e} |\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
