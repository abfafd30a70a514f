"""The clustering stages of csrc/meanshift.hip through the C ABI's metric entry points (uoc_ms_*_ex), one call per stage, on
numpy or device inputs: what tests/test_ms_cosine_gpu.py and tests/test_ms_euclidean_stages_gpu.py drive.  metric is
_native.METRIC_COSINE or _native.METRIC_EUCLIDEAN; with the cosine code every _ex call is the plain entry point (the plain
ones forward to it)."""
import numpy as np
import torch

from tests.golden.cases import KAPPA
from unseenobjectclustering_amd import _native
from unseenobjectclustering_amd.utils import mean_shift as MS

COSINE, EUCLIDEAN = _native.METRIC_COSINE, _native.METRIC_EUCLIDEAN


def to_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def hill_climb_raw(X, Z0, iters, n=None, metric=COSINE, ws=None):
    """uoc_ms_hill_climb_ex on device tensors X [B, >= n, 64] (n rows are read), Z0 [B, m, 64] -> the new seeds."""
    L = _native.lib()
    batch, m = X.shape[0], Z0.shape[1]
    n = X.shape[1] if n is None else n
    assert batch == 1 or n == X.shape[1]
    ws = MS._workspace(X.device, L.uoc_ms_workspace_bytes(batch, n, m)) if ws is None else ws
    Z = Z0.clone()
    _native.call("uoc_ms_hill_climb_ex", X.device, X, batch, n, Z, m, KAPPA, iters, metric, ws, ws.numel())
    torch.cuda.synchronize(X.device)
    return Z


def select_raw(device, X, m, first=None, init=None, num_init=0, metric=COSINE, ws=None):
    """uoc_ms_select_seeds_ex on X [B, n, 64], with or without given rows -> (indices [B, m], seeds [B, m, 64]) numpy."""
    L = _native.lib()
    Xd = to_dev(X, device)
    B, n = X.shape[0], X.shape[1]
    seeds = torch.full((B, m, 64), 9.0, device=device) if init is None else to_dev(init, device)
    idx = torch.full((B, m), -7, dtype=torch.int32, device=device)
    firstd = None if first is None else torch.tensor(first, dtype=torch.int32, device=device)
    ws = MS._workspace(device, L.uoc_ms_workspace_bytes(B, n, m)) if ws is None else ws
    _native.call("uoc_ms_select_seeds_ex", device, Xd, B, n, m, 0 if init is None else num_init, firstd, seeds, idx, metric, ws, ws.numel())
    _native.call("uoc_ms_check", device)
    return idx.cpu().numpy(), seeds.cpu().numpy()


def both_sampling_kernels(fn):
    """fn() with the on-chip persistent kernel, then with the one-launch-per-step kernel; the setting is restored."""
    L = _native.lib()
    try:
        for on in (1, 0):
            L.uoc_ms_set_persistent_fps(on)
            fn("on-chip" if on else "streaming")
    finally:
        L.uoc_ms_set_persistent_fps(1)


def components_raw(device, Z, eps, metric=COSINE):
    """uoc_ms_seed_components_ex on Z [B, m, 64] -> (labels [B, m], num_unique [B]) numpy."""
    Zd = to_dev(Z, device)
    B, m = Z.shape[0], Z.shape[1]
    out = torch.full((B, m), -7, dtype=torch.int32, device=device)
    nu = torch.full((B,), -7, dtype=torch.int32, device=device)
    _native.call("uoc_ms_seed_components_ex", device, Zd, B, m, float(eps), metric, out, nu)
    return out.cpu().numpy(), nu.cpu().numpy()


def assign_raw(device, X, Z, sl, nu, metric=COSINE, ws=None, cws=None):
    """uoc_ms_assign_ex and (cosine: the only metric it is built for) uoc_ms_confidence on X [B, n, 64], Z [B, m, 64], seed
    labels [B, m], num_unique [B] -> ((labels, closest) of the assignment, (labels, closest) of the confidence call or None),
    numpy [B, n].
    ws / cws: the scratch of the two calls, of (at least) the size functions' values; the callers' own when given."""
    L = _native.lib()
    Xd, Zd = to_dev(X, device), to_dev(Z, device)
    sld, nud = to_dev(np.asarray(sl, np.int32), device), to_dev(np.asarray(nu, np.int32), device)
    B, n, m = X.shape[0], X.shape[1], Z.shape[1]
    la, ca, lc, cc = (torch.full((B, n), -7, dtype=torch.int32, device=device) for _ in range(4))
    ws = MS._workspace(device, L.uoc_ms_workspace_bytes(B, n, m)) if ws is None else ws
    _native.call("uoc_ms_assign_ex", device, Xd, B, n, Zd, sld, nud, m, metric, la, ca, ws, ws.numel())
    if metric != COSINE:
        return (la.cpu().numpy(), ca.cpu().numpy()), None
    margin = torch.empty((B, n), device=device)
    nws = L.uoc_ms_confidence_workspace_bytes(B, n, m, 1)
    cws = torch.empty(nws, dtype=torch.uint8, device=device) if cws is None else cws
    _native.call("uoc_ms_confidence", device, Xd, 1, B, n, Zd, sld, nud, m, 0, lc, margin, None, cc, None, cws, nws)
    return (la.cpu().numpy(), ca.cpu().numpy()), (lc.cpu().numpy(), cc.cpu().numpy())
