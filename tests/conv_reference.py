"""CPU references of the backbone's kernels (test infrastructure, never product code): fp64 references of the convolution
and of the head, and the fp32 yardsticks the GPU tests take their tolerances from.

A yardstick is a plain float32 evaluation of the same operation in the kernel's documented summation order; its distance from
the fp64 reference on a case is what float32 costs there, and the GPU tests allow the kernels a small multiple of it
(tests/test_conv_tiles_gpu.py).  Tensors are NCHW with the groups in front: x [G,B,Cin,H,W], w [G,Cout,Cin,K,K], b [G,Cout]
or None, res [G,B,Cout,Ho,Wo] or None.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

BK = 32     # channels per K-chunk of both GEMM kernels (csrc/conv.hip, csrc/wino4.hip)


def _finish(y, b, res, relu):
    """+ bias, + residual, ReLU, in this order (the order of both kernels' epilogues), in y's dtype."""
    if b is not None:
        y = y + b.to(y.dtype)[:, None, :, None, None]
    if res is not None:
        y = y + res.to(y.dtype)
    return F.relu(y) if relu else y


def conv(x, w, b=None, res=None, stride=1, pad=0, dil=1, relu=False, dtype=torch.float64):
    """F.conv2d per group in `dtype` (float64: the reference; float32: torch's own CPU kernel, the second yardstick)."""
    y = torch.stack([F.conv2d(x[g].to(dtype), w[g].to(dtype), None, stride=stride, padding=pad, dilation=dil)
                     for g in range(x.shape[0])])
    return _finish(y, b, res, relu)


def _accumulate(acc, A, Wc):
    """One 32-wide K-chunk on the matrix cores: eight steps of four products (lane group q supplies k = 16h + 4q + e to step
    (h, e)), each step's four products summed and added to the float32 accumulator with one rounding.
    acc [..., M, N] float32, A [..., M, 32], Wc [..., N, 32] float32.
    (The yardstick is deliberately the tighter reading of "four products per step".  On the MI355X the GPU's error is about
    twice this one, profiles/conv_tiles_error.md: a variant of this function that rounds after every product, q = 0..3 in
    turn, reproduces the direct kernel's measured maximum error to all four printed digits on every case, so the matrix
    core evidently rounds four times per step, and four times the roundings is twice the error.)"""
    for h in range(2):
        for e in range(4):
            ks = [16 * h + 4 * q + e for q in range(4)]
            part = A[..., ks].astype(np.float64) @ np.swapaxes(Wc[..., ks], -1, -2).astype(np.float64)
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def conv_seq_fp32(x, w, b=None, res=None, stride=1, pad=0, dil=1, relu=False, stem=False):
    """Sequential float32 yardstick of the direct kernel: float32 accumulators, four products per step, K order = cin slice
    outer, tap inner (csrc/conv.hip).  stem: the 7x7 kernel's order instead, one chunk per kernel row, k = 4 kw + channel."""
    G, B, Cin, H, W = x.shape
    Cout, K = w.shape[1], w.shape[3]
    Ho = (H + 2 * pad - dil * (K - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (K - 1) - 1) // stride + 1
    xs = np.pad(x.numpy().astype(np.float32), ((0, 0), (0, 0), (0, 0), (pad, pad), (pad, pad)))
    ws = w.numpy().astype(np.float32)
    out = np.empty((G, B, Cout, Ho, Wo), np.float32)

    def window(g, kh, kw, c0, c1):        # [B*Ho*Wo, c1 - c0]
        v = xs[g, :, c0:c1, kh * dil: kh * dil + (Ho - 1) * stride + 1: stride, kw * dil: kw * dil + (Wo - 1) * stride + 1: stride]
        return v.transpose(0, 2, 3, 1).reshape(B * Ho * Wo, c1 - c0)

    for g in range(G):
        acc = np.zeros((B * Ho * Wo, Cout), np.float32)
        if stem:
            for kh in range(K):
                A = np.zeros((B * Ho * Wo, BK), np.float32)
                Wc = np.zeros((Cout, BK), np.float32)
                for kw in range(K):
                    A[:, 4 * kw: 4 * kw + Cin] = window(g, kh, kw, 0, Cin)
                    Wc[:, 4 * kw: 4 * kw + Cin] = ws[g, :, :, kh, kw]
                acc = _accumulate(acc, A, Wc)
        else:
            for c0 in range(0, Cin, BK):
                for kh in range(K):
                    for kw in range(K):
                        acc = _accumulate(acc, window(g, kh, kw, c0, c0 + BK), ws[g, :, c0:c0 + BK, kh, kw])
        out[g] = acc.reshape(B, Ho, Wo, Cout).transpose(0, 3, 1, 2)
    return _finish(torch.from_numpy(out), b, res, relu)


# F(4x4, 3x3) with the interpolation points 0, 1, -1, 2, -1/2 (and infinity): the matrices of csrc/wino4_math.h
W4_BT = [[1, 1.5, -2, -1.5, 1, 0], [0, -1, -2.5, -0.5, 1, 0], [0, 1, 0.5, -2.5, 1, 0],
         [0, -0.5, -1, 0.5, 1, 0], [0, 2, -1, -2, 1, 0], [0, 1, 1.5, -2, -1.5, 1]]
W4_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -0.5, 0], [0, 1, 1, 4, 0.25, 0], [0, 1, -1, 8, -0.125, 1]]
W4_G = [[1, 0, 0], [-1 / 3, -1 / 3, -1 / 3], [1 / 3, -1 / 3, 1 / 3], [1 / 15, 2 / 15, 4 / 15], [-16 / 15, 8 / 15, -4 / 15], [0, 0, 1]]


def conv_wino4(x, w, b=None, res=None, dil=1, relu=False, dtype=np.float32):
    """The 3x3 stride-1 pad = dil convolution as Winograd F(4x4,3x3), dilation by phase decomposition (csrc/wino4.hip).
    float32: the emulation of the kernels — U = G g G^T in double, rounded once; input transform, the 36 plane products
    (cin chunks of 32 in order, four products per step) and output transform in float32.  float64: the same algebra in
    double, which must equal the direct sum up to fp64 rounding."""
    G, B, Cin, H, W = x.shape
    Cout = w.shape[1]
    f32 = dtype == np.float32
    Gm, BT, AT = np.array(W4_G, np.float64), np.array(W4_BT, dtype), np.array(W4_AT, dtype)
    U = np.einsum("ia,gocab,jb->gijoc", Gm, w.numpy().astype(np.float64), Gm).astype(dtype)        # [G,6,6,Cout,Cin]
    xs = x.numpy().astype(dtype)
    out = np.zeros((G, B, Cout, H, W), dtype)
    for py in range(dil):
        for px in range(dil):
            sub = xs[:, :, :, py::dil, px::dil]                       # one phase: a plain 3x3 pad-1 convolution
            h, wd = sub.shape[3], sub.shape[4]
            if h == 0 or wd == 0:
                continue
            TH, TW = (h + 3) // 4, (wd + 3) // 4
            sp = np.pad(sub, ((0, 0), (0, 0), (0, 0), (1, 4 * TH + 1 - h), (1, 4 * TW + 1 - wd)))
            d = np.lib.stride_tricks.sliding_window_view(sp, (6, 6), axis=(3, 4))[:, :, :, ::4, ::4]   # [G,B,Cin,TH,TW,6,6]
            V = np.einsum("ia,gbctuae,je->gijbtuc", BT, d, BT, optimize=True).astype(dtype)         # [G,6,6,B,TH,TW,Cin]
            V = V.reshape(G, 36, B * TH * TW, Cin)
            Up = U.reshape(G, 36, Cout, Cin)
            if f32:
                M = np.zeros((G, 36, B * TH * TW, Cout), np.float32)
                for c0 in range(0, Cin, BK):
                    M = _accumulate(M, V[..., c0:c0 + BK], Up[..., c0:c0 + BK])
            else:
                M = V @ np.swapaxes(Up, -1, -2)
            M = M.reshape(G, 6, 6, B, TH, TW, Cout)
            Y = np.einsum("ai,gijbtuo,ej->gbotaue", AT, M, AT, optimize=True).astype(dtype)         # [G,B,Cout,TH,4,TW,4]
            Y = Y.reshape(G, B, Cout, 4 * TH, 4 * TW)[:, :, :, :h, :wd]
            out[:, :, :, py::dil, px::dil] = Y
    return _finish(torch.from_numpy(out), b, res, relu)


def head(fa, fb, H, W, cat=False, dtype=torch.float64):
    """The network's head (lib/networks/resnet_dilated.py:325, SEG.py:106-114): bilinear upsampling with align_corners=True of
    the branch sum — or with `cat` of each branch, concatenated — and L2 normalisation over the channels.
    fa, fb [B,64,h,w] (fb may be None) -> [B,64 or 128,H,W] in `dtype` (float64: the reference, float32: the yardstick)."""
    a = fa.to(dtype)
    if cat:
        up = torch.cat([F.interpolate(t.to(dtype), size=(H, W), mode="bilinear", align_corners=True) for t in (fa, fb)], 1)
    else:
        if fb is not None:
            a = a + fb.to(dtype)
        up = F.interpolate(a, size=(H, W), mode="bilinear", align_corners=True)
    return F.normalize(up, p=2, dim=1)


def max_err(a, b):
    return (a.double() - b.double()).abs().max().item()
