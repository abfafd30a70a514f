"""CPU references of the whole embedding network (test infrastructure, never product code): the fp64 reference, and the
float32 yardstick the GPU test takes its tolerance from (tests/test_network_fp64_gpu.py).

reference() is the oracle (oracle/backbone_oracle.py, dtype-generic) on the state dict and the inputs cast to double.
yardstick() is what float32 costs on the case: the distance from that reference of a float32 evaluation, the larger of
  * the network run the way the library runs it (csrc/net.hip), layer by layer: BatchNorm folded in double and rounded to
    float32 once, the Winograd layers through the float32 F(4x4,3x3) emulation of tests/conv_reference.py, every other
    convolution through torch's float32 kernel, the early-fusion stem in two passes, the float32 head;
  * the plain float32 oracle.
The same "whichever is larger" rule as case_data of tests/test_conv_tiles_gpu.py.  The layer-wise evaluation also runs in
float64 (fold kept in double, Winograd algebra in double): it must then equal the reference up to fp64 rounding, which shows
that it has the network's structure and fold (tests/test_network_reference_host.py).

Tensors are NCHW: img, depth [B,3,H,W]; the result is [B,64,H,W], or [B,128,H,W] for RGBD_CAT.
"""
from __future__ import annotations

import contextlib
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import backbone_oracle as BO
from tests import conv_reference as CR
from unseenobjectclustering_amd import synth

MODES = ("RGBD_ADD", "COLOR", "DEPTH", "RGBD_EARLY", "RGBD_CAT")
BRANCH = ("fcn", "fcn_depth")          # group g of the library reads branch g (csrc/net.hip kBranch)
FOLD_EPS = 1e-5                        # BatchNorm2d's eps, the constant of finalize_layer
WINO_MIN_CIN = 64                      # the network's documented Winograd threshold (csrc/net.hip wino_min_cin)
HOSTILE_VARS = (0.0, 1e-8, 1e-6, 1e-4, 1e2)


def groups(mode):
    return 2 if mode in ("RGBD_ADD", "RGBD_CAT") else 1


def runs_winograd(cin, cout, k, stride):
    """The static rule, written down from finalize_layer and wino4_eligible (csrc/net.hip, csrc/wino4.hip): a 3x3 stride-1
    convolution (pad = dilation, so the output has the input's size) with Cin >= 64, Cin a multiple of 32 and Cout = 64 times
    a power of two.  In ResNet34 that is every 3x3 layer but layer2.0.conv1, which has stride 2."""
    n64 = cout // 64
    pair_ok = cin % 32 == 0 and cout % 64 == 0 and n64 > 0 and n64 & (n64 - 1) == 0
    return k == 3 and stride == 1 and cin >= WINO_MIN_CIN and pair_ok


def as_tensors(sd):
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in as_tensors(sd).items()}


@contextlib.contextmanager
def oracle_eps(eps):
    """The oracle with another BatchNorm eps, for the experiment that shows what a test can see; restored on exit."""
    saved = BO.BN_EPS
    BO.BN_EPS = eps
    try:
        yield
    finally:
        BO.BN_EPS = saved


def reference(sd, img, depth, mode, eps=None):
    """The fp64 reference [B,64|128,H,W]: the oracle in double.  eps: the BN_EPS experiment (default: the oracle's own)."""
    with oracle_eps(BO.BN_EPS if eps is None else eps):
        return BO.segnet_forward(to_double(sd), img.double(), depth.double(), mode)


def _fold(sd, G, conv, bn, dtype):
    """finalize_layer: per group w * scale and shift = beta - mean * scale (+ conv bias), scale = gamma / sqrt(var + 1e-5),
    all in double, then ONE rounding to `dtype`.  -> w [G,Cout,Cin,K,K], b [G,Cout]."""
    ws, bs = [], []
    for g in range(G):
        base = f"{BRANCH[g]}.resnet34_8s."
        w = sd[base + conv + ".weight"].double()
        scale, shift = torch.ones(w.shape[0], dtype=torch.float64), torch.zeros(w.shape[0], dtype=torch.float64)
        if bn:
            ga, be, mu, va = (sd[base + bn + s].double() for s in (".weight", ".bias", ".running_mean", ".running_var"))
            scale = ga * (1.0 / torch.sqrt(va + FOLD_EPS))
            shift = be - mu * scale
        if base + conv + ".bias" in sd:
            shift = shift + sd[base + conv + ".bias"].double()
        ws.append((w * scale[:, None, None, None]).to(dtype))
        bs.append(shift.to(dtype))
    return torch.stack(ws), torch.stack(bs)


def layerwise(sd, img, depth, mode, dtype=torch.float32):
    """The network as uoc_net_forward runs it (csrc/net.hip), on the CPU in `dtype` (float32: the emulation; float64: the
    same structure in double).  Activations are [G,B,C,H,W], the groups being the backbones evaluated side by side."""
    sd = as_tensors(sd)
    G = groups(mode)
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    H, W = img.shape[2:]

    def conv(x, name, bn, k, stride, dil, relu, res=None):
        w, b = _fold(sd, G, name, bn, dtype)
        if runs_winograd(w.shape[2], w.shape[1], k, stride):
            return CR.conv_wino4(x, w, b, res, dil, relu, dtype=np_dtype)
        return CR.conv(x, w, b, res, stride, dil if k == 3 else 0, dil, relu, dtype=dtype)

    # the stem: 7x7 stride 2 pad 3 + BN + ReLU
    w, b = _fold(sd, G, "conv1", "bn1", dtype)
    if mode == "RGBD_EARLY":     # two passes: the XYZ half without bias or ReLU, then the image half on top of it
        part = CR.conv(depth[None].to(dtype), w[:, :, 3:], None, None, 2, 3, 1, False, dtype=dtype)
        x = CR.conv(img[None].to(dtype), w[:, :, :3], b, part, 2, 3, 1, True, dtype=dtype)
    else:
        first = depth if mode == "DEPTH" else img
        x = torch.stack([first, depth]) if G == 2 else first[None]
        x = CR.conv(x.to(dtype), w, b, None, 2, 3, 1, True, dtype=dtype)
    x = torch.stack([F.max_pool2d(x[g], 3, 2, 1) for g in range(G)])

    inpl, cur_stride, cur_dil = 64, 4, 1
    for li, (nb, planes) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512)), start=1):
        stride = 1 if li == 1 else 2
        down = stride != 1 or inpl != planes
        if down:
            if cur_stride == 8:          # the stride-to-dilation switch
                cur_dil, stride = cur_dil * stride, 1
            else:
                cur_stride *= stride
        for bi in range(nb):
            p = f"layer{li}.{bi}."
            s = stride if bi == 0 else 1
            tmp = conv(x, p + "conv1", p + "bn1", 3, s, cur_dil, True)
            res = x
            if bi == 0 and down:
                res = conv(x, p + "downsample.0", p + "downsample.1", 1, s, 1, False)
            x = conv(tmp, p + "conv2", p + "bn2", 3, 1, cur_dil, True, res=res)
        inpl = planes
    x = conv(x, "fc", "", 1, 1, 1, False)
    return CR.head(x[0], x[1] if G == 2 else None, H, W, cat=mode == "RGBD_CAT", dtype=dtype)


def yardstick(sd, img, depth, mode, ref=None):
    """max |float32 evaluation - fp64 reference|, the larger of the layer-wise emulation's and the plain float32 oracle's."""
    if ref is None:
        ref = reference(sd, img, depth, mode)
    sd = as_tensors(sd)
    emulation = CR.max_err(layerwise(sd, img, depth, mode, torch.float32), ref)
    plain = CR.max_err(BO.segnet_forward(sd, img.float(), depth.float(), mode), ref)
    return max(emulation, plain)


def hostile_bn(sd, seed):
    """A copy of a synthetic state dict whose BatchNorms stress the fold.  In every BN about every seventh channel gets
    running_var from {0, 1e-8, 1e-6, 1e-4, 1e2}, gamma = g0 * sqrt(var + 1e-5) (g0 the old gamma, the sign of a third of
    them flipped) and running_mean up to +-3; one more channel per BN gets gamma = 0.  The folded scale of those channels
    stays g0 = O(1), so activations stay finite, while a wrong or missing eps changes them by orders of magnitude
    (var = 0: eps = 1e-3 instead of 1e-5 divides the scale by 10; no eps divides by zero)."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    rng = np.random.default_rng(32452843 * seed + 13)
    for key in sorted(k for k in out if k.endswith(".running_var")):
        pfx = key[:-len("running_var")]
        C = out[key].shape[0]
        idx = np.arange(int(rng.integers(7)), C, 7)
        var = rng.choice(np.array(HOSTILE_VARS, np.float32), size=len(idx)).astype(np.float32)
        sign = np.where(rng.random(len(idx)) < 1.0 / 3.0, -1.0, 1.0)
        g0 = out[pfx + "weight"][idx].astype(np.float64)
        out[key][idx] = var
        out[pfx + "weight"][idx] = (sign * g0 * np.sqrt(var.astype(np.float64) + FOLD_EPS)).astype(np.float32)
        out[pfx + "running_mean"][idx] = rng.uniform(-3.0, 3.0, size=len(idx)).astype(np.float32)
        out[pfx + "weight"][(idx[len(idx) // 2] + 3) % C] = 0.0
    return out


# ---- the cases of tests/test_network_fp64_gpu.py --------------------------------------------------------------------------
WSEED = 3


def _case(mode, H, W, frames=(31,), hostile=False):
    name = f"{mode} {H}x{W} B={len(frames)}" + (" hostile BN" if hostile else "")
    return dict(name=name, mode=mode, H=H, W=W, frames=tuple(frames), hostile=hostile)


CASE_LIST = (
    [_case("RGBD_ADD", 8, 8), _case("RGBD_ADD", 16, 8), _case("RGBD_ADD", 9, 15, (31, 32)), _case("RGBD_ADD", 37, 53, (31, 32)),
     _case("RGBD_ADD", 77, 93)]
    + [_case(m, h, w, (31, 32)) for m in ("COLOR", "DEPTH", "RGBD_CAT", "RGBD_EARLY") for h, w in ((9, 15), (37, 53))]
    + [_case("RGBD_ADD", 37, 53, (31, 32), hostile=True), _case("RGBD_CAT", 37, 53, (31, 32), hostile=True)]
    + [_case("RGBD_ADD", 37, 53, (41, 42, 43))]
)
CASES = {c["name"]: c for c in CASE_LIST}
assert len(CASES) == len(CASE_LIST)
HOSTILE_CASES = tuple(c["name"] for c in CASE_LIST if c["hostile"])
EPS_SLIP = 1e-3        # the BN_EPS experiment of the host test


@functools.lru_cache(maxsize=None)
def state_dict(mode, hostile=False):
    """The case's weights as numpy arrays: synthetic_state_dict(3) with the mode's branches and stem; hostile: hostile_bn."""
    branches = BRANCH if groups(mode) == 2 else BRANCH[:1]
    sd = synth.synthetic_state_dict(WSEED, branches=branches, in_channels=6 if mode == "RGBD_EARLY" else 3)
    return hostile_bn(sd, WSEED) if hostile else sd


@functools.lru_cache(maxsize=None)
def frames(seeds, H, W):
    """(img, depth) [B,3,H,W] float32: one synth.rgbd_frame per seed."""
    fr = [synth.rgbd_frame(s, H, W, 3) for s in seeds]
    return (torch.from_numpy(np.concatenate([f["image_color"] for f in fr])),
            torch.from_numpy(np.concatenate([f["depth"] for f in fr])))


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(state dict, img, depth, fp64 reference) of a case, computed once per session and never modified."""
    c = CASES[name]
    sd = state_dict(c["mode"], c["hostile"])
    img, depth = frames(c["frames"], c["H"], c["W"])
    return sd, img, depth, reference(sd, img, depth, c["mode"])


@functools.lru_cache(maxsize=None)
def case_yardstick(name):
    """The case's yardstick, computed (5 to 25 s, most of it in conv_reference._accumulate)."""
    sd, img, depth, ref = case_reference(name)
    return yardstick(sd, img, depth, CASES[name]["mode"], ref)


YARDSTICK_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "network_yardsticks.json")


@functools.lru_cache(maxsize=None)
def _stored():
    with open(YARDSTICK_FILE) as f:
        return json.load(f)


def stored_yardstick(name):
    """The case's yardstick as tests/golden/make_network_yardsticks.py wrote it (CPU results only; the host test holds the
    file to a recomputation)."""
    return float(_stored()[name])
