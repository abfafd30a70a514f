"""Which way every surface faces: per-pixel normals and object faces, on the device (uoc_normals, include/uoc_hip.h;
DESIGN.md §21).

    fitted = support.fit_plane(refined, xyz)                   # the support plane of §13, on the GPU
    res = estimate(xyz, refined, fitted)                       # step 2, window 2, 16 azimuth bins over a full turn
    res.n[b], res.info[b]                                      # [H,W,3] integer normals towards the camera; packed info
    classes(res), azimuth(res)                                 # UP / SIDE / OBLIQUE / DOWN per pixel; the bin of a SIDE pixel
    face_table(res, 0)[a]                                      # pixels, with_normal, up, side, ..., peak, hist of id a
    side_directions(res, fitted, 0, a)                         # approach directions for a side grasp, fullest face first
    opposed(res, 0, a, k, 8)                                   # the SIDE pixels facing along / against closing direction k

The depth sensor delivers whole millimetres, so a normal from box-summed integer differences of the organised cloud is
exact arithmetic on the data as measured: q = rint(16000 p), differences over `step` pixels that stay on one id and jump
at most `jump`, summed over a (2 window + 1)^2 box, a cross product in int64.  With a plane the normal is classed against
it (up within `up_deg` of the plane normal, side within `side_deg` of the plane) and a side pixel falls in one of `angles`
azimuth bins in the plane's own axes; per id the counts and the azimuth histogram.  Integer arithmetic in HIP kernels:
defined exactly, independent of launch order and batch.  `estimate` neither copies to the host nor synchronises.  No CPU
fallback."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native, placement

NUM_IDS = 128
FACE_WORDS = _native.NORMALS_FACE_WORDS
UP, SIDE, OBLIQUE, DOWN = _native.NORMAL_UP, _native.NORMAL_SIDE, _native.NORMAL_OBLIQUE, _native.NORMAL_DOWN
FACE_FIELDS = ("pixels", "with_normal", "up", "side", "oblique", "down", "grazing", "peak")
_PLANE_WORDS = ctypes.sizeof(_native.UocPlane) // 4


class NormalsResult(_native.Fields):
    """Device tensors.  n [B,H,W,3] int32: the integer normal n', zero without one; info [B,H,W] int32 = class | grazing
    << 3 | bin << 8 | nX << 16 | nY << 24, zero without a normal; unit [B,3,H,W] float32 (NaN without a normal) or None;
    faces [B,128,40] int32: FACE_FIELDS and the azimuth histogram [32] per id.  dirs: the direction table [A,2] (host,
    numpy).  packed: n and info as the kernel wrote them, [B,H,W,4]."""


def direction_table(angles):
    """The azimuth bins [A,2] int32: (rint(cos(2 pi k / A) S), rint(sin(2 pi k / A) S)), S = 16384, in float64."""
    A = int(angles)
    if not 1 <= A <= _native.NORMALS_MAX_DIRS:
        raise ValueError(f"angles = {angles} outside 1..{_native.NORMALS_MAX_DIRS}")
    k = np.arange(A, dtype=np.float64)
    S = float(_native.PLACE_SCALE)
    return np.stack([np.rint(np.cos(2 * np.pi * k / A) * S), np.rint(np.sin(2 * np.pi * k / A) * S)], axis=1).astype(np.int32)


def thresholds(up_deg, side_deg):
    """(c_up, s_side) = (rint(cos(up_deg) 2^28), rint(sin(side_deg) 2^28)) in float64."""
    up, side = float(up_deg), float(side_deg)
    if not (up >= 0 and side >= 0 and up + side < 90):
        raise ValueError(f"up_deg = {up_deg} and side_deg = {side_deg}: both must be >= 0 and their sum below 90")
    return (int(np.rint(np.cos(np.deg2rad(np.float64(up))) * 2.0 ** 28)),
            int(np.rint(np.sin(np.deg2rad(np.float64(side))) * 2.0 ** 28)))


def normals_records(xyz, labels, planes, step, window, jump_mm, min_pairs, dirs, c_up, s_side, unit=False):
    """The raw uoc_normals call: (packed [B,H,W,4] int32, unit [B,3,H,W] float32 or None, faces [B,128,40] int32) on the
    device, no synchronisation.  xyz float32 [B,3,H,W] contiguous; labels int32 [B,H,W] contiguous or None; planes int32
    [B,21] contiguous or None, all on one GPU; dirs: [A,2] integers in -16384..16384."""
    B, _, H, W = (int(v) for v in xyz.shape)
    dev = xyz.device
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.int64))
    if d.ndim != 2 or d.shape[1] != 2:
        raise ValueError(f"dirs has shape {d.shape}, not [A,2]")
    A = int(d.shape[0])
    if not 1 <= A <= _native.NORMALS_MAX_DIRS:
        raise ValueError(f"{A} directions outside 1..{_native.NORMALS_MAX_DIRS}")
    if np.abs(d).max() > _native.PLACE_SCALE:
        raise ValueError(f"dirs has a component outside -{_native.PLACE_SCALE}..{_native.PLACE_SCALE}")
    ws = _native.workspace("uoc_normals_workspace_bytes", dev, B, H, W, who="normals", hint=f"B={B} H={H} W={W}")
    packed = torch.empty((B, H, W, 4), dtype=torch.int32, device=dev)
    un = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if unit else None
    faces = torch.empty((B, NUM_IDS, FACE_WORDS), dtype=torch.int32, device=dev)
    _native.call("uoc_normals", dev, xyz, labels, planes, B, H, W, int(step), int(window), int(jump_mm), int(min_pairs),
                 _native.host_words(d, 2), A, int(c_up), int(s_side), packed, un, faces, ws, ws.numel())
    return packed, un, faces


def estimate(xyz, labels=None, fitted=None, step=2, window=2, jump=0.030, min_pairs=None, angles=16, up_deg=20.0,
             side_deg=20.0, unit=False) -> NormalsResult:
    """xyz: device tensor [B,3,H,W] or [3,H,W] float metres (sample['depth']); labels: [B,H,W] or [H,W] of int32 / int64 /
    float ids, or None (one surface).  fitted: the result of support.fit_plane on the same frames (its device records are
    read in place), a tuple (normal, d, centroid, u, v) as placement.pack_planes takes it, or None (no classes).  step in
    1..8 pixels, window in 0..4, jump in metres, used in whole millimetres (1..1000); min_pairs in 1..(2 window + 1)^2,
    None: half the window, at least 1; angles: azimuth bins over a full turn, 1..32; up_deg, side_deg >= 0 with a sum
    below 90; unit: also the fp32 unit normals.  Returns a NormalsResult."""
    r, s = int(step), int(window)
    if not 1 <= r <= 8:
        raise ValueError(f"step = {step} outside 1..8")
    if not 0 <= s <= 4:
        raise ValueError(f"window = {window} outside 0..4")
    jump_mm = int(round(float(jump) * 1000))
    if not 1 <= jump_mm <= 1000:
        raise ValueError(f"jump = {jump} m is {jump_mm} mm, outside 1..1000 mm")
    mp = max(1, s // 2) if min_pairs is None else int(min_pairs)
    if not 1 <= mp <= (2 * s + 1) ** 2:
        raise ValueError(f"min_pairs = {min_pairs} outside 1..{(2 * s + 1) ** 2}")
    dirs = direction_table(angles)
    c_up, s_side = thresholds(up_deg, side_deg)
    if not _native.on_gpu(xyz):
        raise _native.NativeError("normals: xyz must be a tensor on the GPU (there is no CPU fallback)")
    if xyz.dim() == 3:
        xyz = xyz[None]
    if xyz.dim() != 4 or xyz.shape[1] != 3:
        raise _native.NativeError(f"normals: xyz {tuple(xyz.shape)} is not [B,3,H,W]")
    B = int(xyz.shape[0])
    dev = xyz.device
    lab = None
    if labels is not None:
        if not _native.on_gpu(labels) or labels.device != dev:
            raise _native.NativeError("normals: labels must be a tensor on the GPU of xyz (there is no CPU fallback)")
        if labels.dim() == 2:
            labels = labels[None]
        if labels.dim() != 3 or labels.shape[0] != B or tuple(labels.shape[1:]) != tuple(xyz.shape[2:]):
            raise _native.NativeError(f"normals: labels {tuple(labels.shape)} and xyz {tuple(xyz.shape)} do not match "
                                      "([B,H,W] and [B,3,H,W])")
        lab = _native.as_labels(labels)
    planes = None
    if fitted is not None:
        if isinstance(fitted, (tuple, list)):
            planes = torch.from_numpy(placement.pack_planes(*fitted, frames=B)).to(dev)
        else:
            planes = getattr(fitted, "records", None)
            if planes is None:
                raise _native.NativeError("normals: fitted is neither a fit_plane result nor (normal, d, centroid, u, v)")
        if not _native.on_gpu(planes) or planes.device != dev or planes.dtype != torch.int32 or tuple(planes.shape) != (B, _PLANE_WORDS):
            raise _native.NativeError(f"normals: the plane records do not match the {B} frames on {dev}")
        planes = planes.contiguous()
    packed, un, faces = normals_records(xyz.to(torch.float32).contiguous(), lab, planes, r, s, jump_mm, mp, dirs, c_up, s_side,
                                        unit)
    return NormalsResult(n=packed[..., :3], info=packed[..., 3], unit=un, faces=faces, dirs=dirs, packed=packed, planes=planes,
                         step=r, window=s, jump_mm=jump_mm, min_pairs=mp, angles=len(dirs), c_up=c_up, s_side=s_side)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def classes(result):
    """[B,H,W] int32 on the device: 0 (no normal, or no plane), UP, SIDE, OBLIQUE or DOWN."""
    return result.info & 7


def grazing(result):
    """[B,H,W] bool on the device: the pixels whose normal does not face the camera."""
    return (result.info >> 3 & 1) != 0


def azimuth(result):
    """[B,H,W] int32 on the device: the azimuth bin of a SIDE pixel, -1 elsewhere."""
    return torch.where(classes(result) == SIDE, result.info >> 8 & 31, torch.full_like(result.info, -1))


def face_table(result, b):
    """Frame b's faces on the host: a dict of FACE_FIELDS -> int array [128] and `hist` -> [128,A]."""
    t = result.faces[b].cpu().numpy().astype(np.int64)
    out = {name: t[:, k] for k, name in enumerate(FACE_FIELDS)}
    out["hist"] = t[:, len(FACE_FIELDS):len(FACE_FIELDS) + result.angles]
    return out


def _plane_axes(fitted, b):
    """(u, v) of frame b, float64 on the host, from a fit_plane result, device records or the pack_planes tuple."""
    if isinstance(fitted, (tuple, list)):
        rec = placement.pack_planes(*fitted)
        return placement.plane_axes(rec, b if len(rec) > 1 else 0)[2:]
    return placement.plane_axes(getattr(fitted, "records", fitted), b)[2:]


def side_directions(result, fitted, b, a, min_share=0.2):
    """The camera-space unit vectors cos(2 pi k / A) u + sin(2 pi k / A) v of the azimuth bins k that hold at least
    `min_share` of id a's SIDE pixels in frame b, fullest first (ties: the lower bin): the directions its side faces look
    in, which a side grasp approaches against.  A list of (k, share, vector [3] float64); empty without SIDE pixels."""
    row = result.faces[b, int(a)].cpu().numpy().astype(np.int64)
    side, hist = int(row[3]), row[len(FACE_FIELDS):len(FACE_FIELDS) + result.angles]
    if side == 0:
        return []
    u, v = _plane_axes(fitted, b)
    out = []
    for k in sorted(range(result.angles), key=lambda k: (-int(hist[k]), k)):
        if hist[k] < min_share * side or hist[k] == 0:
            break
        t = 2 * np.pi * k / result.angles
        d = np.cos(t) * u + np.sin(t) * v
        out.append((k, float(hist[k]) / side, d / np.linalg.norm(d)))
    return out


def opposed(result, b, a, k, A_half):
    """The antipodal support of closing direction k of a grasp.candidates(angles=A_half) result on id a of frame b: the
    numbers of SIDE pixels in the two full-turn bins that face along (k) and against (k + A_half) the closing direction,
    as (along, against).  Needs result.angles == 2 A_half, so that the grasp's direction pi k / A_half is bin k."""
    A_half, k = int(A_half), int(k)
    if result.angles != 2 * A_half:
        raise ValueError(f"opposed: the normals have {result.angles} bins, not 2 x {A_half}")
    if not 0 <= k < A_half:
        raise ValueError(f"opposed: k = {k} outside 0..{A_half - 1}")
    row = result.faces[b, int(a)].cpu().numpy().astype(np.int64)
    return int(row[len(FACE_FIELDS) + k]), int(row[len(FACE_FIELDS) + k + A_half])
