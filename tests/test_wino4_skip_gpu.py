"""The skipping plan of the Winograd F(4x4,3x3) path against the dense plan (csrc/wino4.hip, csrc/wino4_math.h).

UOC_CONV_WINOGRAD4 orders the tiles by class and runs every frequency plane over the tiles that read it for a stored output
only; UOC_CONV_WINOGRAD4_DENSE runs the same three kernels with every plane over every tile.  No stored bit may differ.  The
entry owns its scratch, so the test poisons it through the entry itself: a dense-plan call on an all-NaN input of the same
shape leaves every (plane, tile) row of V and M NaN, whichever plan runs next; a row the skipping plan read without having
written it would show as a NaN (or as a difference) in the output.

The tolerance against torch's fp32 conv2d on the CPU is the one test_backbone_gpu.test_winograd_conv_vs_torch_cpu uses."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unseenobjectclustering_amd import _native

pytestmark = pytest.mark.gpu

SKIP, DENSE = _native.CONV_WINOGRAD4, _native.CONV_WINOGRAD4_DENSE
EINVAL = -22

# (G, B, H, W, dil, Cin, Cout, residual + ReLU, every tile of the list as well)
CASES = [
    (1, 1, 7, 7, 1, 32, 64, False, True),       # one tile per class; ranges of 1-4 rows
    (2, 2, 28, 28, 4, 64, 64, True, False),     # 7x7 phases
    (1, 3, 28, 28, 2, 32, 128, False, False),   # 14x14 phases, two invalid rows
    (1, 1, 15, 20, 1, 64, 64, False, False),    # row-partial only
    (1, 1, 8, 8, 1, 32, 64, False, False),      # nothing skipped
    (1, 1, 29, 31, 4, 32, 64, False, False),    # ragged phases
    (1, 1, 33, 5, 4, 32, 64, False, False),     # ragged phases, empty tiles
    (1, 1, 3, 5, 4, 32, 64, False, False),      # image smaller than the dilation
    (1, 7, 28, 28, 4, 64, 64, False, True),     # ranges of 448 / 224 / 224 / 112 rows: unaligned lo, partial m-tiles
]


def tile_list(algo):
    L = _native.lib()
    n = L.uoc_conv2d_tile_list(algo, None, 0)
    assert n > 0, n
    buf = (ctypes.c_int32 * (2 * n))()
    assert L.uoc_conv2d_tile_list(algo, buf, n) == n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


def conv(device, xd, wd, bd, rd, dil, relu, algo, pair=None):
    """One call of the entry on NHWC device tensors -> (rc, out [G,B,H,W,Cout] on the device)."""
    G, B, H, W, Cin = xd.shape
    Cout = wd.shape[2]
    out = torch.full((G, B, H, W, Cout), 7.0, device=device)
    L = _native.lib()
    args = (_native.ptr(xd), _native.ptr(wd), _native.ptr(bd), _native.ptr(rd), _native.ptr(out), G, B, H, W, Cin, Cout, 3, 1, dil,
            dil, int(relu), algo, _native.stream_ptr(device))
    rc = L.uoc_conv2d_nhwc_algo(*args) if pair is None else L.uoc_conv2d_nhwc_tile(*args, pair[0], pair[1])
    return rc, out


def poisoned_run(device, xd, wd, bd, rd, dil, relu, algo, pair=None):
    """Fill the entry's V and M with NaN (dense plan, all-NaN input: every row of every plane), then the real call."""
    rc, _ = conv(device, torch.full_like(xd, float("nan")), wd, bd, rd, dil, relu, DENSE)
    assert rc == 0, rc
    rc, out = conv(device, xd, wd, bd, rd, dil, relu, algo, pair)
    _native.check(rc, f"conv algo {algo} tile {pair}")
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "G%dB%d_%dx%d_d%d_%d-%d" % c[:7])
def test_skipping_plan_equals_dense_plan(device, case):
    G, B, H, W, dil, Cin, Cout, resrelu, every_tile = case
    g = torch.Generator().manual_seed(1000 * H + 10 * W + dil)
    x = torch.randn(G, B, Cin, H, W, generator=g)
    w = torch.randn(G, Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(G, Cout, generator=g)
    res = torch.randn(G, B, Cout, H, W, generator=g) if resrelu else None
    ref = torch.stack([F.conv2d(x[i], w[i], b[i], padding=dil, dilation=dil) for i in range(G)])
    if resrelu:
        ref = F.relu(ref + res)
    xd = x.permute(0, 1, 3, 4, 2).contiguous().to(device)
    wd = w.permute(0, 3, 4, 1, 2).reshape(G, 9, Cout, Cin).contiguous().to(device)
    bd = b.to(device)
    rd = res.permute(0, 1, 3, 4, 2).contiguous().to(device) if resrelu else None

    dense = poisoned_run(device, xd, wd, bd, rd, dil, resrelu, DENSE)
    err = (dense.cpu().permute(0, 1, 4, 2, 3) - ref).abs().max().item()
    print(f"dense plan: max abs error against fp32 conv2d {err:.3e} (scale {ref.abs().max().item():.2f})")
    assert torch.isfinite(dense).all()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err

    got = poisoned_run(device, xd, wd, bd, rd, dil, resrelu, SKIP)
    assert torch.isfinite(got).all(), "the skipping plan read a row it had not written"
    assert torch.equal(got, dense)
    err = (got.cpu().permute(0, 1, 4, 2, 3) - ref).abs().max().item()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err

    if every_tile:
        ran = 0
        for pair in tile_list(SKIP):
            if Cout % pair[0]:
                rc, _ = conv(device, xd, wd, bd, rd, dil, resrelu, SKIP, pair)
                assert rc == EINVAL, (pair, rc)
                continue
            for algo in (SKIP, DENSE):
                got = poisoned_run(device, xd, wd, bd, rd, dil, resrelu, algo, pair)
                assert torch.isfinite(got).all(), (algo, pair)
                assert torch.equal(got, dense), (algo, pair)
            ran += 1
        assert ran >= 4, ran


def test_dense_algorithm_shares_list_and_model():
    """The dense algorithm names the same instantiations; the static model answers for either plan with a listed pair."""
    L = _native.lib()
    assert tile_list(DENSE) == tile_list(SKIP)
    cfg, bm = ctypes.c_int32(), ctypes.c_int32()
    for algo in (SKIP, DENSE):
        for (G, B, H, W, dil, Cin, Cout, _, _) in CASES:
            assert L.uoc_conv2d_tile_choice(G, B, H, W, Cin, Cout, 3, 1, dil, algo, ctypes.byref(cfg), ctypes.byref(bm), None) == 0
            assert (cfg.value, bm.value) in tile_list(algo) and Cout % cfg.value == 0
