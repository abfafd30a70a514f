"""Every tile instantiation of the convolution kernels, and the stem, the pooling and the head kernels on their own.

The direct kernel (csrc/conv.hip), the Winograd plane GEMM (csrc/wino4.hip) and its split-precision variant
(csrc/wino4_split.hip) are families of template instantiations chosen at run time.  uoc_conv2d_tile_list names them,
uoc_conv2d_nhwc_tile runs exactly one.  Per algorithm: all instantiations that admit a case are bit-identical, one of them is
within a tolerance of the fp64 reference, and every instantiation of the list ran.

Tolerances come from the CPU alone (tests/conv_reference.py), never from the kernel: 4 x the error, against fp64 and on the
very case, of a float32 evaluation of the same operation — the sequential yardstick in the kernel's K order or torch's own
float32 kernel, whichever is larger, for the direct kernel and the stem; the float32 F(4x4,3x3) emulation for Winograd; the
float32 head for the head.  The 4 is the margin for an equally long summation in another order (two float32 sums of the same
terms in different orders draw their maximum error over 1e4 .. 1e5 outputs from the same distribution).  Measured ratios
GPU error / yardstick: profiles/conv_tiles_error.md (scripts/conv_tile_report.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_reference as CR
from tests.backbone_layers import backbone_layers
from unseenobjectclustering_amd import _native

pytestmark = pytest.mark.gpu
EINVAL = -22
MARGIN = 4.0
DIRECT, WINO, SPLIT = _native.CONV_DIRECT, _native.CONV_WINOGRAD4, _native.CONV_WINOGRAD4_BF16X3
ALGO_NAME = {DIRECT: "direct", WINO: "winograd4", SPLIT: "winograd4 bf16x3"}
DIRECT_BN = {0: 128, 1: 128, 2: 64, 3: 64}


def tile_list(algo):
    L = _native.lib()
    n = L.uoc_conv2d_tile_list(algo, None, 0)
    assert n > 0, n
    buf = (ctypes.c_int32 * (2 * n))()
    assert L.uoc_conv2d_tile_list(algo, buf, n) == n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


def admits(algo, pair, case):
    """Cout % BN == 0: the one condition under which a listed tile does not serve a case of this file."""
    bn = DIRECT_BN[pair[0]] if algo == DIRECT else pair[0]
    return case["Cout"] % bn == 0


def pair_loop(case):
    """The plane GEMM's static rule: the pair loop runs on an even number, four or more, of 32-channel chunks."""
    cpt = case["Cin"] // 32
    return cpt % 2 == 0 and cpt >= 4


def _c(name, seed, G, B, H, W, Cin, Cout, K=3, stride=1, dil=1, res=False, relu=False, bias=True):
    return dict(name=name, seed=seed, G=G, B=B, H=H, W=W, Cin=Cin, Cout=Cout, K=K, stride=stride, dil=dil,
                pad=dil if K == 3 else 0, res=res, relu=relu, bias=bias)


DIRECT_BMS = (64, 80, 96, 128, 160, 192)
DIRECT_CASES = [
    _c("D1", 1, 2, 2, 9, 7, 32, 128, res=True, relu=True),          # M = 126: one partial m-tile; one K-chunk per tap
    _c("D2", 2, 1, 1, 16, 24, 96, 256, dil=2, bias=False),          # M = 384: exact multiple of 64, 96, 128, 192; odd chunk count
    _c("D3", 3, 1, 3, 31, 27, 64, 128, stride=2),                   # strided, ragged
    _c("D4", 4, 2, 2, 33, 17, 64, 128, K=1, stride=2),              # the shortcut
    _c("D5", 5, 1, 1, 15, 20, 128, 64, dil=4),                      # most taps outside the image; Cout = 64: families 2 and 3 only
] + [_c(f"D6({bm})", 60 + i, 1, 1, 1, 2 * bm + 1, 32, 128) for i, bm in enumerate(DIRECT_BMS)] + [   # M = 2 bm + 1; every vertical tap outside
    _c("D7", 7, 1, 1, 60, 80, 512, 64, K=1),                        # the fc shape; long K
]
WINO_BMS = (96, 128, 160, 192)
WINO_CASES = [
    _c("W1", 11, 2, 2, 13, 9, 64, 128, dil=2),                      # NT = 32: one partial m-tile
    _c("W2", 12, 1, 3, 28, 28, 128, 256, dil=4, res=True, relu=True),   # NT = 192: exact for BM 96 and 192, ragged for 128 and 160
    _c("W3", 13, 2, 1, 61, 83, 128, 256, dil=2, res=True, relu=True),   # NT = 352, >= 288 items on <= 256 blocks: the ring prefetches across items
] + [_c(f"W4({bm})", 140 + i, 1, 1, 4, 4 * bm + 4, 32, 128) for i, bm in enumerate(WINO_BMS)] + [   # NT = bm + 1; one K-chunk
    _c("W5", 15, 1, 2, 20, 24, 96, 64, bias=False),                 # three chunks: odd, no pair loop
    _c("W6", 16, 1, 2, 20, 24, 160, 128),                           # five chunks
    _c("W7", 17, 1, 2, 20, 24, 192, 128, dil=2),                    # six chunks: pair loop with an odd number of pairs
]
SPLIT_CASES = [c for c in WINO_CASES if c["name"] in ("W1", "W2", "W3", "W7")]
CASES = {DIRECT: DIRECT_CASES, WINO: WINO_CASES, SPLIT: SPLIT_CASES}
BY_NAME = {c["name"]: c for c in DIRECT_CASES + WINO_CASES}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs of a case and its CPU results, computed once: the fp64 reference and the float32 yardstick errors."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randn(c["G"], c["B"], c["Cin"], c["H"], c["W"], generator=g)
    w = torch.randn(c["G"], c["Cout"], c["Cin"], c["K"], c["K"], generator=g) / np.sqrt(c["Cin"] * c["K"] * c["K"])
    b = torch.randn(c["G"], c["Cout"], generator=g) if c["bias"] else None
    ref = CR.conv(x, w, b, None, c["stride"], c["pad"], c["dil"], False)
    res = torch.randn(ref.shape, generator=g) if c["res"] else None
    args = (x, w, b, res, c["stride"], c["pad"], c["dil"], c["relu"])
    ref = CR.conv(*args)
    d = dict(x=x, w=w, b=b, res=res, ref=ref, scale=max(1.0, ref.abs().max().item()))
    if name.startswith("D"):
        d["yard"] = max(CR.max_err(CR.conv_seq_fp32(*args), ref), CR.max_err(CR.conv(*args, dtype=torch.float32), ref))
    else:
        d["yard"] = CR.max_err(CR.conv_wino4(x, w, b, res, c["dil"], c["relu"]), ref)
    assert 0 < d["yard"] < 1e-4 * d["scale"], d["yard"]
    return d


@functools.lru_cache(maxsize=None)
def device_inputs(name, device):
    c, d = BY_NAME[name], case_data(name)
    K = c["K"]
    xd = d["x"].permute(0, 1, 3, 4, 2).contiguous().to(device)                                              # [G][B][H][W][Cin]
    wd = d["w"].permute(0, 3, 4, 1, 2).reshape(c["G"], K * K, c["Cout"], c["Cin"]).contiguous().to(device)    # [G][tap][Cout][Cin]
    bd = d["b"].to(device) if d["b"] is not None else None
    rd = d["res"].permute(0, 1, 3, 4, 2).contiguous().to(device) if d["res"] is not None else None
    return xd, wd, bd, rd


def run_tile(device, name, algo, pair, expect_rc=0):
    """One instantiation on one case -> the output [G,B,Ho,Wo,Cout] on the device (pre-filled with NaN: an output the kernel
    does not write cannot pass), or None after the expected error code."""
    c, d = BY_NAME[name], case_data(name)
    xd, wd, bd, rd = device_inputs(name, device)
    G, B, Cout, Ho, Wo = d["ref"].shape
    out = torch.full((G, B, Ho, Wo, Cout), float("nan"), device=device)
    L = _native.lib()
    rc = L.uoc_conv2d_nhwc_tile(_native.ptr(xd), _native.ptr(wd), _native.ptr(bd), _native.ptr(rd), _native.ptr(out),
                                G, B, c["H"], c["W"], c["Cin"], Cout, c["K"], c["stride"], c["dil"], c["pad"], int(c["relu"]),
                                algo, _native.stream_ptr(device), pair[0], pair[1])
    if expect_rc:
        assert rc == expect_rc, (name, pair, rc)
        return None
    _native.check(rc, f"uoc_conv2d_nhwc_tile {name} {pair}")
    return out


@functools.lru_cache(maxsize=None)
def run_case(device, name, algo):
    """Every listed instantiation of `algo` on the case: those that admit it must agree bit for bit (a), the others return
    UOC_EINVAL.  -> (pairs that ran, the common output on the CPU as [G,B,Cout,Ho,Wo])."""
    c = BY_NAME[name]
    ran, first = [], None
    for pair in tile_list(algo):
        if not admits(algo, pair, c):
            run_tile(device, name, algo, pair, expect_rc=EINVAL)
            continue
        out = run_tile(device, name, algo, pair)
        if first is None:
            first = out
        else:
            assert torch.equal(out, first), f"{ALGO_NAME[algo]} {name}: tile {pair} differs from tile {ran[0]} in " \
                f"{int((out != first).sum())} outputs, max |diff| {(out - first).abs().max().item():.3e}"
        ran.append(pair)
    assert ran, name
    return tuple(ran), first.cpu().permute(0, 1, 4, 2, 3)


def measure(device, name, algo):
    """-> (yardstick, GPU error) of a case, both against fp64 in max norm (the report's columns)."""
    d = case_data(name)
    _, got = run_case(device, name, algo)
    return d["yard"], CR.max_err(got, d["ref"])


def check_case(device, name, algo):
    yard, err = measure(device, name, algo)
    print(f"{ALGO_NAME[algo]} {name}: yardstick {yard:.3e} GPU error {err:.3e} ratio {err / yard:.2f}")
    assert err <= MARGIN * yard, f"{name}: GPU error {err:.3e} > {MARGIN} x yardstick {yard:.3e}"


def check_coverage(device, algo):
    """(c) every listed pair ran at least 4 cases, (d) the set of pairs run equals the list; the plane GEMM's pairs met both
    settings of the pair loop."""
    tiles = tile_list(algo)
    assert len(set(tiles)) == len(tiles)
    count = {p: 0 for p in tiles}
    loops = {p: set() for p in tiles}
    for c in CASES[algo]:
        for p in run_case(device, c["name"], algo)[0]:
            count[p] += 1
            loops[p].add(pair_loop(c))
    assert set(p for p, n in count.items() if n) == set(tiles)
    assert min(count.values()) >= 4, count
    if algo == WINO:
        assert all(s == {True, False} for s in loops.values()), loops


@pytest.mark.parametrize("name", [c["name"] for c in DIRECT_CASES])
def test_direct_tiles_agree_and_match_fp64(device, name):
    check_case(device, name, DIRECT)


def test_direct_every_tile_ran(device):
    tiles = tile_list(DIRECT)
    assert len(tiles) == 14 and set(bm for _, bm in tiles) == set(DIRECT_BMS)
    check_coverage(device, DIRECT)


@pytest.mark.parametrize("name", [c["name"] for c in WINO_CASES])
def test_winograd_tiles_agree_and_match_fp64(device, name):
    check_case(device, name, WINO)


def test_winograd_every_tile_ran(device):
    tiles = tile_list(WINO)
    assert len(tiles) == 8 and set(bm for _, bm in tiles) == set(WINO_BMS)      # each with and without the pair loop: 16
    check_coverage(device, WINO)


@pytest.mark.parametrize("name", [c["name"] for c in SPLIT_CASES])
def test_split_precision_tiles_agree_and_match_fp32_winograd(device, name):
    """Bit-identical across the split-precision GEMM's own tiles, and within 2e-5 of the output scale of the fp32 Winograd
    result (the bar of test_split_precision_plane_gemm_vs_fp32: the dropped terms are <= 2^-24 relative per product)."""
    _, got = run_case(device, name, SPLIT)
    _, fp32 = run_case(device, name, WINO)
    err = CR.max_err(got, fp32)
    print(f"bf16x3 {name}: |bf16x3 - fp32| {err:.3e}, scale {case_data(name)['scale']:.3f}")
    assert err < 2e-5 * case_data(name)["scale"], err


def test_split_precision_every_tile_ran(device):
    assert len(tile_list(SPLIT)) == 6
    check_coverage(device, SPLIT)


def test_unlisted_tiles_are_refused(device):
    """(e): a pair that is not in the list returns UOC_EINVAL, and so does an unknown algorithm."""
    for algo, name, bad in ((DIRECT, "D1", [(0, 64), (0, 80), (1, 128), (3, 160), (2, 100), (4, 96), (-1, 96), (0, 0), (128, 96)]),
                            (WINO, "W1", [(128, 64), (128, 80), (64, 100), (32, 96), (0, 96), (3, 96), (256, 128)]),
                            (SPLIT, "W1", [(128, 160), (128, 192), (64, 64), (0, 128)])):
        listed = set(tile_list(algo))
        for pair in bad:
            assert pair not in listed
            run_tile(device, name, algo, pair, expect_rc=EINVAL)
    run_tile(device, "D1", 3, (0, 96), expect_rc=EINVAL)
    assert _native.lib().uoc_conv2d_tile_list(3, None, 0) == EINVAL


def test_network_shapes_choose_listed_tiles(device):
    """Whatever the static model — or, for the direct kernel, the tuner, which may take any family at the height the model gives
    it — picks for a layer of the backbone at 480x640 (B = 1, 4) and 224x224 (B = 1..12) is in the lists, all of which ran."""
    L = _native.lib()
    lists = {a: set(tile_list(a)) for a in (DIRECT, WINO, SPLIT)}
    seen = {a: set() for a in lists}
    cfg, bm, fam = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_int32 * 4)()
    shapes = [(480, 640, B) for B in (1, 4)] + [(224, 224, B) for B in range(1, 13)]
    for H, W, B in shapes:
        for G in (1, 2):
            for (h, w, cin, cout, K, s, d) in backbone_layers(H, W):
                wino = K == 3 and s == 1 and cin >= 64          # the network's static rule (csrc/net.hip finalize_layer)
                for algo in ((WINO, SPLIT) if wino else (DIRECT,)):
                    rc = L.uoc_conv2d_tile_choice(G, B, h, w, cin, cout, K, s, d, algo, ctypes.byref(cfg), ctypes.byref(bm), fam)
                    _native.check(rc, "uoc_conv2d_tile_choice")
                    picks = {(cfg.value, bm.value)}
                    if algo == DIRECT:
                        assert fam[cfg.value] == bm.value
                        assert [f > 0 for f in fam] == [cout % DIRECT_BN[i] == 0 for i in range(4)]
                        picks |= {(i, fam[i]) for i in range(4) if fam[i]}
                    assert picks <= lists[algo], (H, W, B, G, h, w, cin, cout, K, s, d, picks)
                    seen[algo] |= picks
    assert len(seen[DIRECT]) >= 8 and len(seen[WINO]) >= 4, seen      # the shapes do spread over the lists
    assert L.uoc_conv2d_tile_choice(1, 1, 20, 24, 128, 192, 3, 1, 1, WINO, ctypes.byref(cfg), ctypes.byref(bm), None) == EINVAL


# ---- the stem -------------------------------------------------------------------------------------------------------------
def _stem(device, x, w, b, res, relu):
    """uoc_net_stem: x [G,B,3,H,W] (CPU), w [G,64,3,7,7], b [G,64] | None (host), res [G,B,H1,W1,64] on the device | None."""
    G, B, _, H, W = x.shape
    H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = x.contiguous().to(device)
    wh = w.contiguous().float()
    bh = b.contiguous().float() if b is not None else None
    out = torch.full((G, B, H1, W1, 64), float("nan"), device=device)
    _native.call("uoc_net_stem", device, xd, wh, bh, res, G, B, H, W, int(relu), out)
    return out


@functools.lru_cache(maxsize=None)
def stem_data(H, W, cin):
    g = torch.Generator().manual_seed(1000 + 7 * H + W + cin)
    x = torch.randn(2, 2, cin, H, W, generator=g)
    w = torch.randn(2, 64, cin, 7, 7, generator=g) / np.sqrt(cin * 49)
    b = torch.randn(2, 64, generator=g)
    ref = CR.conv(x, w, b, None, 2, 3, 1, True)
    if cin == 3:
        seq = CR.conv_seq_fp32(x, w, b, None, 2, 3, 1, True, stem=True)
    else:       # early fusion as the network runs it: the XYZ half without bias or ReLU, then the image half on top of it
        part = CR.conv_seq_fp32(x[:, :, 3:], w[:, :, 3:], None, None, 2, 3, 1, False, stem=True)
        seq = CR.conv_seq_fp32(x[:, :, :3], w[:, :, :3], b, part, 2, 3, 1, True, stem=True)
    yard = max(CR.max_err(seq, ref), CR.max_err(CR.conv(x, w, b, None, 2, 3, 1, True, dtype=torch.float32), ref))
    assert 0 < yard < 1e-4 * max(1.0, ref.abs().max().item())
    return x, w, b, ref, yard


def measure_stem(device, H, W, cin):
    x, w, b, ref, yard = stem_data(H, W, cin)
    if cin == 3:
        out = _stem(device, x, w, b, None, True)
    else:
        part = _stem(device, x[:, :, 3:], w[:, :, 3:], None, None, False)
        out = _stem(device, x[:, :, :3], w[:, :, :3], b, part, True)
    return yard, CR.max_err(out.cpu().permute(0, 1, 4, 2, 3), ref)


@pytest.mark.parametrize("hw", [(8, 8), (9, 11), (37, 53), (64, 64)])
def test_stem_vs_fp64(device, hw):
    yard, err = measure_stem(device, hw[0], hw[1], 3)
    print(f"stem {hw}: yardstick {yard:.3e} GPU error {err:.3e} ratio {err / yard:.2f}")
    assert err <= MARGIN * yard, (err, yard)


@pytest.mark.parametrize("hw", [(9, 11), (37, 53)])
def test_stem_early_fusion_two_passes_vs_fp64(device, hw):
    """Pass one: the XYZ half of the six-channel weights, NULL bias, no ReLU; pass two: the image half with the bias, pass one as
    its residual, ReLU — against the fp64 six-channel convolution."""
    yard, err = measure_stem(device, hw[0], hw[1], 6)
    print(f"early-fusion stem {hw}: yardstick {yard:.3e} GPU error {err:.3e} ratio {err / yard:.2f}")
    assert err <= MARGIN * yard, (err, yard)


# ---- max pooling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("hw", [(4, 4), (5, 7), (1, 9), (32, 40)])
def test_maxpool_equals_torch(device, hw, negative):
    """Bit-equal to F.max_pool2d(x, 3, 2, 1) on the same float32 data.  With every value negative, a border padded with zero
    instead of skipped would win every border window."""
    H, W = hw
    g = torch.Generator().manual_seed(2000 + 50 * H + W)
    x = torch.randn(3, 64, H, W, generator=g)
    if negative:
        x = -x.abs() - 0.5
    want = F.max_pool2d(x, 3, 2, 1)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert want.shape == (3, 64, Ho, Wo)
    xd = x.permute(0, 2, 3, 1).contiguous().to(device)
    out = torch.full((3, Ho, Wo, 64), float("nan"), device=device)
    _native.call("uoc_maxpool3x3s2_nhwc", device, xd, out, 3, H, W, 64)
    assert torch.equal(out.cpu().permute(0, 3, 1, 2), want)


# ---- the head ---------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 1, 8, 8), (2, 3, 9, 17), (8, 8, 64, 64), (10, 12, 77, 93), (28, 28, 224, 224)]
HEAD_MODES = ("single", "add", "cat")


def _head(device, fa, fb, H, W, cat):
    """uoc_head: fa, fb [B,64,h,w] (CPU; fb may be None) -> [B,64 or 128,H,W] on the CPU."""
    B, _, h, w = fa.shape
    fad = fa.permute(0, 2, 3, 1).contiguous().to(device)
    fbd = fb.permute(0, 2, 3, 1).contiguous().to(device) if fb is not None else None
    out = torch.full((B, 2 if cat else 1, H * W, 64), float("nan"), device=device)
    _native.call("uoc_head", device, fad, fbd, out, B, h, w, H, W, int(cat))
    return out.cpu().permute(0, 1, 3, 2).reshape(B, -1, H, W)


@functools.lru_cache(maxsize=None)
def head_data(shape, mode):
    h, w, H, W = shape
    g = torch.Generator().manual_seed(3000 + 100 * h + w + HEAD_MODES.index(mode))
    fa = torch.randn(2, 64, h, w, generator=g)
    fb = torch.randn(2, 64, h, w, generator=g) if mode != "single" else None
    ref = CR.head(fa, fb, H, W, mode == "cat")
    yard = CR.max_err(CR.head(fa, fb, H, W, mode == "cat", dtype=torch.float32), ref)
    assert 0 < yard < 1e-5
    return fa, fb, ref, yard


def measure_head(device, shape, mode):
    fa, fb, ref, yard = head_data(shape, mode)
    got = _head(device, fa, fb, shape[2], shape[3], mode == "cat")
    return yard, CR.max_err(got, ref), (got.double().norm(dim=1) - 1).abs().max().item()


@pytest.mark.parametrize("mode", HEAD_MODES)
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_vs_fp64(device, shape, mode):
    yard, err, norm_err = measure_head(device, shape, mode)
    print(f"head {shape} {mode}: yardstick {yard:.3e} GPU error {err:.3e} ratio {err / yard:.2f}, |norm - 1| {norm_err:.2e}")
    assert norm_err < 1e-5
    assert err <= MARGIN * yard, (err, yard)


@pytest.mark.parametrize("mode", HEAD_MODES)
def test_head_all_zero_pixel_is_zero_not_nan(device, mode):
    """Every channel of every source of output pixel (0, 0) is zero (its only source with a non-zero weight is (0, 0)): the
    embedding there is 0, as F.normalize gives, and every other pixel is still unit-norm."""
    g = torch.Generator().manual_seed(3999)
    fa = torch.randn(2, 64, 2, 3, generator=g)
    fb = torch.randn(2, 64, 2, 3, generator=g) if mode != "single" else None
    fa[:, :, 0, 0] = 0
    if fb is not None:
        fb[:, :, 0, 0] = 0
    got = _head(device, fa, fb, 9, 17, mode == "cat")
    assert torch.isfinite(got).all()
    assert (got[:, :, 0, 0] == 0).all()
    norms = got.double().norm(dim=1)
    norms[:, 0, 0] = 1
    assert (norms - 1).abs().max().item() < 1e-5
    ref = CR.head(fa, fb, 9, 17, mode == "cat")
    assert (ref[:, :, 0, 0] == 0).all() and CR.max_err(got, ref) < 1e-5
