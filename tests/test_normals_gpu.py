"""uoc_normals on the GPU against tests/normals_reference.py: n, info and faces bit for bit, over the shapes, parameters and
engineered frames of DESIGN.md §21; batch independence, repeatability, the wrapper's label handling, every rejection with
the outputs left untouched, the unit normals against the float64 formula, the helpers and the demo pair end to end."""
import ctypes
import faulthandler
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import normals_reference as R
from tests import support_reference as S13
from unseenobjectclustering_amd import _native, normals, support

pytestmark = pytest.mark.gpu

DEFAULTS = dict(r=2, s=2, jump_mm=30, mp=None, A=16, angles=(20, 20))


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def boxes(H, W, seed, holes=0.05):
    return R.boxes_scene(H, W, seed, holes=holes)


def ref_kwargs(r, s, jump_mm, mp, A, angles):
    c_up, s_side = R.thresholds(*angles)
    return dict(step=r, window=s, jump_mm=jump_mm, min_pairs=mp, dirs=R.direction_table(A), c_up=c_up, s_side=s_side)


def run(device, xyz, labels=None, planes=None, unit=False, **kw):
    """xyz [B,3,H,W], labels [B,H,W] or None (numpy); planes: a list of plane dicts / None per frame, or None.  Returns
    (n, info, faces) as numpy and the unit tensor."""
    p = dict(DEFAULTS, **kw)
    X = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(device)
    L = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(device)
    P = None if planes is None else torch.from_numpy(np.stack([R.plane_record(q) for q in planes])).to(device)
    mp = R.default_min_pairs(p["s"]) if p["mp"] is None else p["mp"]
    c_up, s_side = R.thresholds(*p["angles"])
    packed, un, faces = normals.normals_records(X, L, P, p["r"], p["s"], p["jump_mm"], mp, R.direction_table(p["A"]), c_up, s_side, unit)
    packed = packed.cpu().numpy()
    return packed[..., :3], packed[..., 3], faces.cpu().numpy(), un


def check(got, want, what):
    n, info, faces = got[:3]
    assert np.array_equal(n, want["n"]), (what, "n", int((n != want["n"]).any(axis=-1).sum()))
    assert np.array_equal(info, want["info"]), (what, "info", int((info != want["info"]).sum()))
    assert np.array_equal(faces, want["faces"]), (what, "faces", np.argwhere(faces != want["faces"])[:8].tolist())


def against_reference(device, xyz, labels, planes, what, **kw):
    got = run(device, xyz, labels, planes, **kw)
    want = R.estimate_batch(xyz, labels, planes, **ref_kwargs(**dict(DEFAULTS, **kw)))
    check(got, want, what)
    return got, want


# ---- shapes and parameters ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(r=8, s=4, jump_mm=1000, mp=40, A=32, angles=(45, 44))], ids=["default", "largest"])
def test_full_frames(device, kw):
    lab, xyz = boxes(480, 640, 1)
    (n, info, faces, _), want = against_reference(device, xyz[None], lab[None], [R.table_plane()], "480x640", **kw)
    assert (info != 0).sum() > 100000 and (faces[0, 1:6, 1] > 0).all() and (kw or (faces[0, 1:6, 3] > 0).all())


@pytest.mark.parametrize("H,W", [(224, 224), (61, 83), (24, 32)])
@pytest.mark.parametrize("r,s", [(1, 0), (2, 2), (4, 4), (8, 4)])
def test_shapes_and_stencils(device, H, W, r, s):
    lab, xyz = boxes(H, W, 2, 0.0 if (r, s) == (4, 4) else 0.05)          # every pair of a full window needs a scene without holes
    full = (2 * s + 1) ** 2
    sets = {(1, 0): dict(jump_mm=1, mp=1, A=1, angles=(0, 0)), (2, 2): dict(jump_mm=30, mp=None, A=5, angles=(45, 44)),
            (4, 4): dict(jump_mm=1000, mp=full, A=16, angles=(89, 0)), (8, 4): dict(jump_mm=30, mp=1, A=32, angles=(20, 20))}
    kw = dict(sets[(r, s)], r=r, s=s)
    got, _ = against_reference(device, xyz[None], lab[None], [R.table_plane()], (H, W, r, s), **kw)
    assert (got[1] != 0).any() or (H, W) == (24, 32)           # 24x32 has no surface that fills the largest windows
    if (H, W) == (61, 83):                                   # the same stencil without labels, and without a plane
        bare, _ = against_reference(device, xyz[None], None, [R.table_plane()], (H, W, r, s, "no labels"), **kw)
        assert bare[2][0, 1:, 0].sum() == 0 and bare[2][0, 0, 0] == H * W
        flat, _ = against_reference(device, xyz[None], lab[None], None, (H, W, r, s, "no plane"), **kw)
        assert (flat[1] & 7).max() == 0 and np.array_equal(flat[0], got[0])          # the normals do not depend on the plane


@pytest.mark.parametrize("H,W", [(3, 1), (1, 1), (1, 40), (5, 70), (33, 17)])
def test_images_smaller_than_the_halo(device, H, W):
    lab, xyz = R.boxes_scene(H, W, 4, nobj=2, holes=0.0, mirror=False)
    xyz = R.frontal(H, W) if H * W < 50 else xyz
    for r, s in ((1, 0), (2, 2), (4, 4), (8, 4)):
        for mp in (1, (2 * s + 1) ** 2):
            against_reference(device, xyz[None], lab[None], [R.table_plane()], (H, W, r, s, mp), r=r, s=s, mp=mp, jump_mm=1000)


@pytest.mark.parametrize("jump_mm", [1, 30, 1000])
@pytest.mark.parametrize("A,angles", [(1, (20, 20)), (5, (0, 0)), (16, (45, 44)), (32, (89, 0))])
def test_jumps_bins_and_thresholds(device, jump_mm, A, angles):
    lab, xyz = boxes(61, 83, 3)
    got, _ = against_reference(device, xyz[None], lab[None], [R.table_plane()], (jump_mm, A, angles), jump_mm=jump_mm, A=A, angles=angles)
    assert ((got[1] >> 8 & 31) < A).all()


# ---- engineered frames ---------------------------------------------------------------------------------------------------
def test_bad_points_and_labels(device):
    lab, xyz = R.case_nasty()
    got, want = against_reference(device, xyz[None], lab[None], [R.table_plane()], "nasty")
    assert got[2][0, 50, 0] == 1 and got[2][0, 127, 1] > 0 and got[2][0, 0, 0] == ((lab < 1) | (lab > 127)).sum()
    bad = ~(np.isfinite(xyz).all(axis=0) & (xyz[2] > 0))
    assert bad.sum() > 50 and (got[1][0][bad] == 0).all() and (got[0][0][bad] == 0).all()
    lab, xyz = R.case_all_ids()
    got, _ = against_reference(device, xyz[None], lab[None], [R.table_plane()], "127 ids", s=1)
    assert (got[2][0, 1:, 0] > 0).all()


def test_the_edges_of_the_ranges(device):
    xyz = R.case_range()
    for r, s in ((1, 0), (1, 1), (2, 1)):
        (n, info, faces, _), want = against_reference(device, xyz[None], None, None, ("range", r, s), r=r, s=s, mp=1, jump_mm=1000)
    o = R.estimate(xyz, step=1, window=0, min_pairs=1, jump_mm=1000, parts=True)
    assert o["nX"][9, 5] == 1 and o["nX"][9, 9] == 0                  # a component of 16383 makes a pair, 16384 does not
    got = run(device, xyz[None], None, None, r=1, s=0, mp=1, jump_mm=1000)
    assert (got[1][0, 9, 5] >> 16 & 255) == 1 and got[1][0, 9, 9] == 0


def test_collinear_mirrored_equality_and_tie(device):
    got, _ = against_reference(device, R.case_collinear()[None], None, None, "collinear", r=1, s=1, jump_mm=1000)
    assert not got[0].any() and not got[1].any() and got[2][0, 0, :2].tolist() == [120, 0]
    got, _ = against_reference(device, R.case_mirrored()[None], None, None, "mirrored", r=1, s=0, mp=1)
    assert (got[1] != 0).sum() == 140 and ((got[1] >> 3 & 1) == (got[1] != 0)).all() and got[2][0, 0, 6] == 140
    plane = R.plane_dict(*R.frontal_plane_tuple())
    got, _ = against_reference(device, R.frontal(12, 16)[None], None, [plane], "equality", r=1, s=1, angles=(0, 0))
    assert ((got[1] & 7)[got[1] != 0] == R.UP).all() and got[2][0, 0, 2] == got[2][0, 0, 1] > 0
    xyz, plane = R.case_tie()
    got, _ = against_reference(device, xyz[None], None, [plane], "tie", r=1, s=1, A=4)
    assert ((got[1] & 7)[got[1] != 0] == R.SIDE).all() and (got[1] >> 8 & 31).max() == 0 and got[2][0, 0, 7] == 0
    got, _ = against_reference(device, xyz[None], None, [plane], "no tie", r=1, s=1, A=8)
    assert ((got[1] >> 8 & 31)[got[1] != 0] == 1).all() and got[2][0, 0, 7] == 1


def test_the_shift_at_the_largest_stencil(device):
    xyz = S13._grid_plane(40, 48)
    got, want = against_reference(device, xyz[None], None, None, "shift", r=8, s=4, jump_mm=1000)
    full = (got[1] >> 16 & 255) == 81
    assert full.any() and (np.abs(got[0][full]).max(axis=-1) >= 1 << 29).all()


# ---- batches, repeatability, labels -----------------------------------------------------------------------------------------
def test_a_frame_does_not_depend_on_its_mates(device):
    scenes = [boxes(61, 83, k) for k in (1, 2, 3)]
    lab, xyz = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    planes = [R.table_plane(), None, R.plane_dict(*R.frontal_plane_tuple())]
    got, want = against_reference(device, xyz, lab, planes, "batch")
    assert (got[1][1] & 7).max() == 0 and (got[1][0] & 7).max() > 0              # the frame without a plane among frames with one
    for b in range(3):
        alone = run(device, xyz[b:b + 1], lab[b:b + 1], planes[b:b + 1])
        for k in range(3):
            assert np.array_equal(alone[k][0], got[k][b]), (b, k)
    other = run(device, xyz[::-1].copy(), lab[::-1].copy(), planes[::-1])
    for k in range(3):
        assert np.array_equal(other[k][::-1], got[k]), k
    rejected = dict(planes[0], found=0)
    got0 = run(device, xyz[:1], lab[:1], [rejected])
    assert np.array_equal(got0[1], run(device, xyz[:1], lab[:1], None)[1])


def test_two_runs_agree(device):
    lab, xyz = boxes(224, 224, 5)
    a = run(device, xyz[None].repeat(4, 0), lab[None].repeat(4, 0), [R.table_plane()] * 4, unit=True)
    b = run(device, xyz[None].repeat(4, 0), lab[None].repeat(4, 0), [R.table_plane()] * 4, unit=True)
    for k in range(3):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k][0], a[k][3])
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


def test_estimate_takes_labels_of_any_type_and_layout(device):
    lab, xyz = boxes(61, 83, 1)
    want = R.estimate(xyz, lab, R.table_plane())
    X = torch.from_numpy(xyz).to(device)
    tup = tuple(R.table_plane()[k] for k in ("normal", "d", "centroid", "u", "v"))
    strided = torch.from_numpy(np.ascontiguousarray(lab.T)).to(device).T
    assert not strided.is_contiguous()
    for L in (torch.from_numpy(lab).to(device), torch.from_numpy(lab.astype(np.int64)).to(device), torch.from_numpy(lab.astype(np.float32)).to(device),
              strided, strided.long()[None]):
        res = normals.estimate(X if L.dim() == 2 else X[None], L, tup)
        check((res.n[0].cpu().numpy(), res.info[0].cpu().numpy(), res.faces[0].cpu().numpy()), want, str(L.dtype))
    wide = torch.from_numpy(np.concatenate([xyz, xyz], axis=2)).to(device)[:, :, :83]      # a non-contiguous cloud
    res = normals.estimate(wide.double(), strided, tup)
    check((res.n[0].cpu().numpy(), res.info[0].cpu().numpy(), res.faces[0].cpu().numpy()), want, "strided xyz")
    assert res.unit is None and res.angles == 16 and res.min_pairs == 1 and np.array_equal(res.dirs, R.direction_table(16))
    with pytest.raises(_native.NativeError):
        normals.estimate(X, torch.from_numpy(lab[:, :-1].copy()).to(device))
    with pytest.raises(_native.NativeError):
        normals.estimate(X, torch.from_numpy(lab), tup)
    with pytest.raises(_native.NativeError):
        normals.estimate(X, None, object())


def test_estimate_reads_a_fitted_plane_in_place(device):
    lab, xyz = boxes(224, 224, 5)
    X, L = torch.from_numpy(xyz).to(device), torch.from_numpy(lab).to(device)
    fitted = support.fit_plane(L, X)
    res = normals.estimate(X, L, fitted, angles=8, up_deg=15.0, side_deg=25.0)
    assert res.planes.data_ptr() == fitted.records.data_ptr() and int(fitted.found[0]) == 1
    kw = ref_kwargs(2, 2, 30, None, 8, (15.0, 25.0))
    want = R.estimate(xyz, lab, fitted.records[0].cpu().numpy(), **kw)
    check((res.n[0].cpu().numpy(), res.info[0].cpu().numpy(), res.faces[0].cpu().numpy()), want, "fitted")
    assert np.bincount((res.info[0].cpu().numpy() & 7).ravel(), minlength=5)[[R.UP, R.SIDE]].min() > 500


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def test_a_rejected_call_writes_nothing(device):
    H, W, B = 24, 32, 2
    lab, xyz = boxes(H, W, 1)
    X = torch.from_numpy(np.stack([xyz, xyz])).to(device)
    L = torch.from_numpy(np.stack([lab, lab])).to(device)
    P = torch.from_numpy(np.stack([R.plane_record(R.table_plane())] * 2)).to(device)
    lib = _native.lib()
    nws = lib.uoc_normals_workspace_bytes(B, H, W)
    assert nws >= B * 128 * 40 * 4
    packed = torch.full((B, H, W, 4), -7, dtype=torch.int32, device=device)
    unit = torch.full((B, 3, H, W), -7.0, device=device)
    faces = torch.full((B, 128, 40), -7, dtype=torch.int32, device=device)
    ws = torch.full((nws + 16,), 0x5A, dtype=torch.uint8, device=device)
    dirs = (ctypes.c_int32 * 64)(*([16384, 0] * 32))
    bad_dirs = (ctypes.c_int32 * 64)(*([16385, 0] * 32))

    def call(**over):
        a = dict(xyz=_native.ptr(X), labels=_native.ptr(L), planes=_native.ptr(P), B=B, H=H, W=W, step=2, window=2, jump_mm=30, min_pairs=1,
                 dirs=ctypes.cast(dirs, ctypes.c_void_p), A=16, c_up=1 << 27, s_side=1 << 26, n=_native.ptr(packed), unit=_native.ptr(unit),
                 faces=_native.ptr(faces), ws=_native.ptr(ws), ws_bytes=nws)
        a.update(over)
        with torch.cuda.device(device):
            return lib.uoc_normals(a["xyz"], a["labels"], a["planes"], a["B"], a["H"], a["W"], a["step"], a["window"], a["jump_mm"],
                                   a["min_pairs"], a["dirs"], a["A"], a["c_up"], a["s_side"], a["n"], a["unit"], a["faces"], a["ws"],
                                   a["ws_bytes"], _native.stream_ptr(device))

    odd_ws = ctypes.c_void_p(ws.data_ptr() + 4)
    odd_n = ctypes.c_void_p(packed.data_ptr() + 4)
    rejected = [dict(xyz=None), dict(n=None), dict(faces=None), dict(dirs=None), dict(ws=None), dict(B=0), dict(B=65536), dict(H=0), dict(W=-1),
                dict(step=0), dict(step=9), dict(window=-1), dict(window=5), dict(jump_mm=0), dict(jump_mm=1001), dict(min_pairs=0),
                dict(min_pairs=26), dict(A=0), dict(A=33), dict(c_up=-1), dict(c_up=(1 << 28) + 1), dict(s_side=-1), dict(s_side=1 << 27),
                dict(dirs=ctypes.cast(bad_dirs, ctypes.c_void_p)), dict(ws_bytes=nws - 1), dict(ws_bytes=0), dict(ws=odd_ws), dict(n=odd_n)]
    for over in rejected:
        assert call(**over) == -22, over
        assert lib.uoc_last_error().decode().startswith("uoc_normals:"), over
    torch.cuda.synchronize(device)
    assert (packed == -7).all() and (unit == -7.0).all() and (faces == -7).all() and (ws == 0x5A).all()
    assert call() == 0                                          # and the same buffers take the accepted call
    torch.cuda.synchronize(device)
    want = R.estimate_batch(np.stack([xyz, xyz]), np.stack([lab, lab]), [R.table_plane()] * 2, min_pairs=1,
                            dirs=np.array([[16384, 0]] * 16), c_up=1 << 27, s_side=1 << 26)
    check((packed[..., :3].cpu().numpy(), packed[..., 3].cpu().numpy(), faces.cpu().numpy()), want, "after the rejections")
    assert (ws[nws:] == 0x5A).all()                              # nothing past the stated size
    assert call(labels=None, planes=None, unit=None) == 0
    torch.cuda.synchronize(device)
    assert (packed[..., 3] & 7).max() == 0 and (faces[:, 1:, 0] == 0).all()


# ---- the unit normals ---------------------------------------------------------------------------------------------------------
def test_unit_normals_match_the_float64_formula(device):
    for (H, W, seed), kw in (((224, 224, 5), dict()), ((61, 83, 2), dict(r=8, s=4, jump_mm=1000))):
        lab, xyz = boxes(H, W, seed)
        n, info, faces, un = run(device, xyz[None], lab[None], [R.table_plane()], unit=True, **kw)
        want = R.estimate(xyz, lab, R.table_plane(), **ref_kwargs(**dict(DEFAULTS, **kw)))
        got = un[0].cpu().numpy()
        has = info[0] != 0
        assert has.sum() > 1000 and np.isnan(got[:, ~has]).all() and np.isnan(want["unit"][:, ~has]).all()
        err = np.abs(got[:, has].astype(np.float64) - want["unit"][:, has]).max()
        print("unit normals", (H, W), "max abs error", err)
        assert err <= 2.0 ** -22                     # one rounding to fp32 of a value in [-1, 1]: at most 2^-25
        plain = run(device, xyz[None], lab[None], [R.table_plane()], **kw)
        assert plain[3] is None and np.array_equal(plain[0], n) and np.array_equal(plain[2], faces)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def test_helpers(device):
    lab, xyz = boxes(480, 640, 1)
    X, L = torch.from_numpy(xyz).to(device), torch.from_numpy(lab).to(device)
    plane = R.table_plane()
    tup = tuple(plane[k] for k in ("normal", "d", "centroid", "u", "v"))
    res = normals.estimate(X, L, tup)
    want = R.estimate(xyz, lab, plane, parts=True)
    assert np.array_equal(normals.classes(res)[0].cpu().numpy(), want["cls"])
    assert np.array_equal(normals.grazing(res)[0].cpu().numpy(), want["grazing"])
    assert np.array_equal(normals.azimuth(res)[0].cpu().numpy(), np.where(want["cls"] == R.SIDE, want["bin"], -1))
    table = normals.face_table(res, 0)
    for k, name in enumerate(R.FACE_FIELDS):
        assert np.array_equal(table[name], want["faces"][:, k]), name
    assert table["hist"].shape == (128, 16) and np.array_equal(table["hist"], want["faces"][:, 8:24])
    n_plane = plane["normal"].astype(np.float64)
    seen = 0
    for a in range(1, 6):
        dirs = normals.side_directions(res, tup, 0, a)
        hist, side = want["faces"][a, 8:24], want["faces"][a, 3]
        assert [d[0] for d in dirs] == [k for k in sorted(range(16), key=lambda k: (-hist[k], k)) if hist[k] >= 0.2 * side]
        assert dirs and dirs[0][0] == want["faces"][a, 7]
        for k, share, vec in dirs:
            assert abs(np.linalg.norm(vec) - 1) < 1e-6 and abs(vec @ n_plane) < 1e-3 and abs(share - hist[k] / side) < 1e-12
            mean = want["unit"][:, (lab == a) & (want["cls"] == R.SIDE) & (want["bin"] == k)].mean(axis=1)
            assert mean @ vec / np.linalg.norm(mean) > np.cos(np.deg2rad(25.0))          # the bin's pixels do face that way
        if len(dirs) >= 2 and (dirs[0][0] - dirs[1][0]) % 16 in (4, 12):
            assert abs(dirs[0][2] @ dirs[1][2]) < 1e-3                                    # two faces a quarter turn apart
            seen += 1
        for k in range(8):
            assert normals.opposed(res, 0, a, k, 8) == (hist[k], hist[k + 8])
    assert seen >= 1
    assert normals.side_directions(res, tup, 0, 100) == []
    with pytest.raises(ValueError):
        normals.opposed(res, 0, 1, 0, 16)
    with pytest.raises(ValueError):
        normals.opposed(res, 0, 1, 8, 8)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _demo(golden_dir):
    from unseenobjectclustering_amd import io as uio, networks, synth
    d = os.path.join(golden_dir, "demo")
    cam = json.load(open(os.path.join(d, "camera_params.json")))
    sample = uio.read_sample(os.path.join(d, "000002-color.png"), os.path.join(d, "000002-depth.png"), cam)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


def test_segment_objects_with_normals_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    plain = O.segment_objects(sample, net, net_crop)
    np.random.seed(3)
    out = O.segment_objects(sample, net, net_crop, normals=True, normals_args=dict(angles=8, unit=True))
    assert len(plain) == 3 and len(out) == 5 and hasattr(out[3], "normal")       # implies the plane
    assert torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])
    res = out[4]
    final = out[1] if out[1] is not None else out[0]
    lab = final[0].numpy().astype(np.int32)
    xyz = sample["depth"][0].numpy()
    want = R.estimate(xyz, lab, out[3].records[0].cpu().numpy(), **ref_kwargs(2, 2, 30, None, 8, (20.0, 20.0)))
    check((res.n[0].cpu().numpy(), res.info[0].cpu().numpy(), res.faces[0].cpu().numpy()), want, "demo")
    assert res.unit is not None and (res.info != 0).sum() > 10000 and int(out[3].found[0]) == 1
    np.random.seed(3)
    both = O.segment_objects(sample, net, net_crop, relations=True, normals=True)
    assert len(both) == 6 and hasattr(both[4], "layer") and both[5].angles == 16
