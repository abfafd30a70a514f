"""The CPU references of tests/conv_reference.py check each other (no GPU): the Winograd algebra against the direct sum, the
float32 yardsticks against float64, the head against the oracle's network."""
import numpy as np
import torch

from oracle import backbone_oracle as BO
from tests import conv_reference as CR
from unseenobjectclustering_amd import synth


def _case(seed, G, B, H, W, Cin, Cout, K=3, bias=True, use_res=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(G, B, Cin, H, W, generator=g)
    w = torch.randn(G, Cout, Cin, K, K, generator=g) / np.sqrt(Cin * K * K)
    b = torch.randn(G, Cout, generator=g) if bias else None
    return x, w, b, g, use_res


def test_winograd_algebra_in_float64_equals_the_direct_sum():
    """Ragged and dilated shapes (partial tiles in every phase, phases of different size, a phase narrower than a tile)."""
    for seed, (G, B, H, W, Cin, Cout, dil) in enumerate([(2, 2, 13, 9, 32, 64, 2), (1, 1, 15, 20, 64, 64, 4), (1, 2, 7, 10, 32, 64, 1),
                                                         (1, 1, 4, 21, 32, 64, 1), (1, 1, 5, 3, 32, 64, 3)]):
        x, w, b, g, _ = _case(100 + seed, G, B, H, W, Cin, Cout)
        res = torch.randn(G, B, Cout, H, W, generator=g)
        want = CR.conv(x, w, b, res, 1, dil, dil, True)
        got = CR.conv_wino4(x, w, b, res, dil, True, dtype=np.float64)
        assert got.dtype == torch.float64 and CR.max_err(got, want) < 1e-10, (H, W, dil)


def test_conv_yardsticks_differ_from_float64_by_rounding_only():
    x, w, b, g, _ = _case(7, 2, 2, 11, 9, 64, 64)
    res = torch.randn(2, 2, 64, 11, 9, generator=g)
    want = CR.conv(x, w, b, res, 1, 2, 2, True)
    scale = max(1.0, want.abs().max().item())
    for name, got in (("sequential", CR.conv_seq_fp32(x, w, b, res, 1, 2, 2, True)), ("winograd", CR.conv_wino4(x, w, b, res, 2, True)),
                      ("torch", CR.conv(x, w, b, res, 1, 2, 2, True, dtype=torch.float32))):
        assert got.dtype == torch.float32
        assert 0 < CR.max_err(got, want) < 1e-4 * scale, name
    # strided, and the 1x1 shortcut
    x, w, b, _, _ = _case(8, 1, 2, 13, 10, 32, 64)
    want = CR.conv(x, w, b, None, 2, 1, 1, False)
    assert 0 < CR.max_err(CR.conv_seq_fp32(x, w, b, None, 2, 1, 1, False), want) < 1e-4 * max(1.0, want.abs().max().item())
    x, w, b, _, _ = _case(9, 1, 1, 9, 7, 96, 64, K=1, bias=False)
    want = CR.conv(x, w, None, None, 2, 0, 1, False)
    assert 0 < CR.max_err(CR.conv_seq_fp32(x, w, None, None, 2, 0, 1, False), want) < 1e-4 * max(1.0, want.abs().max().item())
    # the stem's order: 7x7 stride 2 pad 3 over 3 channels, one chunk per kernel row
    x, w, b, _, _ = _case(10, 2, 1, 9, 11, 3, 64, K=7)
    want = CR.conv(x, w, b, None, 2, 3, 1, True)
    assert 0 < CR.max_err(CR.conv_seq_fp32(x, w, b, None, 2, 3, 1, True, stem=True), want) < 1e-4 * max(1.0, want.abs().max().item())


def test_head_yardstick_differs_from_float64():
    g = torch.Generator().manual_seed(11)
    fa, fb = torch.randn(2, 64, 2, 3, generator=g), torch.randn(2, 64, 2, 3, generator=g)
    for cat in (False, True):                 # 2x3 -> 9x17: source coordinates oy / 8 and ox / 8
        want = CR.head(fa, fb, 9, 17, cat)
        got = CR.head(fa, fb, 9, 17, cat, dtype=torch.float32)
        assert want.shape == (2, 128 if cat else 64, 9, 17) and got.dtype == torch.float32
        assert 0 < CR.max_err(got, want) < 1e-5
        assert (want.norm(dim=1) - 1).abs().max().item() < 1e-12


def test_head_reference_equals_the_oracle():
    """The oracle upsamples each branch's 1/8-resolution features and adds; the head reference adds and upsamples.  In float64,
    on the features of the oracle's own two backbones, both give the same embeddings."""
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.synthetic_state_dict(3).items()}
    fr = synth.rgbd_frame(5, 40, 56, 2)
    img, dep = torch.from_numpy(fr["image_color"]).double(), torch.from_numpy(fr["depth"]).double()
    with torch.no_grad():
        fa, _ = BO.resnet34_8s(sd, "fcn.resnet34_8s.", img)
        fb, _ = BO.resnet34_8s(sd, "fcn_depth.resnet34_8s.", dep)
    assert fa.shape[2:] == (5, 7)
    for mode, cat in (("RGBD_ADD", False), ("RGBD_CAT", True)):
        want = BO.segnet_forward(sd, img, dep, mode)
        assert CR.max_err(CR.head(fa, fb, 40, 56, cat), want) < 1e-12, mode
    assert CR.max_err(CR.head(fa, None, 40, 56), BO.segnet_forward(sd, img, None, "COLOR")) < 1e-12
