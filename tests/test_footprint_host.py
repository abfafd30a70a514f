"""The numpy restatement of uoc_footprint (tests/footprint_reference.py): its span and run form against the all-offsets
form, the properties of the mask, the window, a hand-counted grid, the key orders on constructed ties, the conversions of
footprint.rect and its conservative claim, the engineered grids against what they are used for; the UOC_EINVAL paths of
uoc_footprint through ctypes (validation comes before any device work, the pointers are never dereferenced) and the
Python wrapper's range checks.  No GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import footprint_reference as R
from unseenobjectclustering_amd import _native, footprint

EINVAL = -22
HALF_EXTENTS = [(0, 0), (255, 255), (16384, 0), (0, 16384), (11585, 11585), (256, 0), (4024, 952), (1000, 1), (12000, 11000), (8192, 8192)]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ("fits", "count", "best"))


@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_span_and_run_form_equals_all_offsets_form(G):
    for seed in (1, 2):
        st, ow, d2 = R.random_grid(G, seed, noise=0.05)
        P = R.present_id(ow, st)
        for A, rects, ub in ((16, [R.record(640, 200), R.record(300, 300, ignore=P, mode=R.NEAREST, ai=3, aj=-2)], 1),
                             (5, [R.record(0, 0), R.record(1200, 0, ignore=P), R.record(0, 700)], 0),
                             (32, [R.record(513, 129, mode=R.NEAREST, ai=G, aj=G)], seed % 2)):
            dirs = R.direction_table(A)
            fast, slow = R.footprint(st, ow, d2, dirs, rects, ub), R.footprint_literal(st, ow, d2, dirs, rects, ub)
            assert same(fast, slow), (G, seed, A)
            assert fast["fits"].shape == (len(rects), G, G) and not fast["count"][:, A:].any()
    st, ow, d2 = R.random_grid(G, 3)
    dirs = R.direction_table(4)
    with_frame = R.footprint(st, ow, d2, dirs, [R.record(0, 0)], 0, R.flat_frame(1))
    assert same(with_frame, R.footprint(st, ow, d2, dirs, [R.record(0, 0)], 0)) and with_frame["best"][0, 0] == 1
    for found in (0, 2):
        none = R.footprint(st, ow, d2, dirs, [R.record(0, 0)], 0, R.flat_frame(found))
        assert not none["fits"].any() and not none["count"].any() and none["best"][0].tolist() == list(R.NO_POSE)


def test_mask_rows_are_contiguous_and_the_mask_is_symmetric():
    for A in (1, 5, 16, 32):
        dirs = R.direction_table(A)
        for HL, HW in HALF_EXTENTS:
            for k in range(A):
                offs = R.mask_offsets(dirs, k, HL, HW)
                s = set(offs)
                assert (0, 0) in s and all((-di, -dj) in s for di, dj in s), (A, k, HL, HW)
                spans = R.mask_spans(dirs, k, HL, HW)
                assert sum(hi - lo + 1 for lo, hi in spans.values()) == len(offs), (A, k, HL, HW)       # no gap in a row
                got = footprint.mask_offsets(dirs, k, HL, HW)
                assert got.dtype == np.int32 and [tuple(x) for x in got.tolist()] == offs


def test_window_r_plus_one_equals_window_66():
    assert [R.radius(*h) for h in HALF_EXTENTS[:5]] == [0, 2, 64, 64, 64]
    for A in (1, 5, 16, 32):
        dirs = R.direction_table(A)
        for HL, HW in HALF_EXTENTS:
            assert R.radius(HL, HW) <= 64
            for k in range(A):
                assert R.mask_offsets(dirs, k, HL, HW) == R.mask_offsets(dirs, k, HL, HW, window=66), (A, k, HL, HW)


def test_hand_counted_8x8():
    st, ow = R.bar8()
    d2 = R.clearance(st, ow)
    assert d2[:, 4].tolist() == [1, 4, 4, 4, 4, 4, 4, 1] and d2[3, 3] == 1 and d2[3, 2] == 0
    dirs = R.direction_table(2)
    assert dirs.tolist() == [[16384, 0], [0, 16384]]
    assert R.mask_offsets(dirs, 0, 256, 0) == [(-1, 0), (0, 0), (1, 0)] and R.mask_offsets(dirs, 1, 256, 0) == [(0, -1), (0, 0), (0, 1)]
    for fn in (R.footprint, R.footprint_literal):
        out = fn(st, ow, d2, dirs, [R.record(256, 0)], 1)
        f = out["fits"][0]
        assert out["count"][0, :2].tolist() == [18, 8] and not out["count"][0, 2:].any()
        assert (f[1:7, 3] == 1).all() and (f[1:7, 5] == 1).all() and (f[1:7, 4] == 3).all() and f[0, 4] == 2 and f[7, 4] == 2
        assert f[0, 3] == 0 and f[0, 5] == 0 and not f[:, :3].any() and not f[:, 6:].any()
        # the roomiest: dist2 = 4 in rows 1..6 of column 4; the lowest index is (1, 4), the lowest k is 0
        assert out["best"][0].tolist() == [1, 1, 4, 0, 4, 1 + 16, 26, 20]
    out = R.footprint(st, ow, d2, dirs, [R.record(256, 0, mode=R.NEAREST, ai=7, aj=4)], 1)
    assert out["best"][0].tolist() == [1, 7, 4, 1, 1, 0, 26, 20]                     # only across in the last row
    out = R.footprint(st, ow, d2, dirs, [R.record(256, 0, ignore=3)], 1)              # the walls do not block: only the border does
    assert out["count"][0, :2].tolist() == [6 * 8, 8 * 6]


def test_key_orders_on_constructed_ties():
    st, ow = R.table(16)
    dirs = R.direction_table(4)
    flat = np.full((16, 16), 9, np.int32)
    out = R.footprint(st, ow, flat, dirs, [R.record(0, 0)], 1)                       # every cell, every k, one dist2
    assert out["best"][0].tolist() == [1, 0, 0, 0, 9, 0, 4 * 256, 256]               # the lowest index, then the lowest k
    d2 = flat.copy()
    d2[5, 7] = d2[11, 2] = 20
    out = R.footprint(st, ow, d2, dirs, [R.record(0, 0)], 1)
    assert out["best"][0, :5].tolist() == [1, 5, 7, 0, 20]                           # equal dist2: the lower index
    d2[5, 7] = 70000
    d2[11, 2] = 65536
    out = R.footprint(st, ow, d2, dirs, [R.record(0, 0)], 1)
    assert out["best"][0, :5].tolist() == [1, 5, 7, 0, 65536]                        # the clamp makes them equal: the lower index
    d2[:] = -1
    assert R.footprint(st, ow, d2, dirs, [R.record(0, 0)], 1)["best"][0, :5].tolist() == [1, 0, 0, 0, 0]
    # NEAREST: four cells at one distance from an anchor between them; an anchor outside the grid
    d2 = flat.copy()
    ow2, st2 = ow.copy(), st.copy()
    st2[:] = 2
    ow2[:] = 1
    for c in ((4, 5), (5, 4), (5, 6), (6, 5)):
        st2[c], ow2[c] = 1, 0
    out = R.footprint(st2, ow2, d2, dirs, [R.record(0, 0, mode=R.NEAREST, ai=5, aj=5)], 1)
    assert out["best"][0].tolist() == [1, 4, 5, 0, 9, 1, 16, 4]
    out = R.footprint(st2, ow2, d2, dirs, [R.record(0, 0, mode=R.NEAREST, ai=-4096, aj=4095)], 1)
    assert out["best"][0, :4].tolist() == [1, 4, 5, 0] and out["best"][0, 5] == 4100 ** 2 + 4090 ** 2
    # a bar that fits only along k = 1 at the winning cell: k is the lowest SET bit there
    dirs2 = R.direction_table(2)
    st3, ow3 = R.corridor(16, 1, along_i=True, at=6)
    out = R.footprint(st3, ow3, flat, dirs2, [R.record(256, 0)], 1)
    assert out["best"][0, :4].tolist() == [1, 1, 6, 0] and out["count"][0, :2].tolist() == [14, 0]
    st3, ow3 = R.corridor(16, 1, along_i=False, at=6)
    out = R.footprint(st3, ow3, flat, dirs2, [R.record(256, 0)], 1)
    assert out["best"][0, :4].tolist() == [1, 6, 1, 1] and out["count"][0, :2].tolist() == [0, 14]
    assert R.key_of(R.ROOMIEST, 9, 0, 5, 3) > R.key_of(R.ROOMIEST, 9, 0, 6, 0) > R.key_of(R.ROOMIEST, 8, 0, 0, 0)
    assert R.key_of(R.NEAREST, 0, 3, 5, 1) > R.key_of(R.NEAREST, 0, 3, 5, 2) > R.key_of(R.NEAREST, 0, 4, 0, 0) > 0


def test_rect_conversions():
    assert footprint.rect(0.30, 0.06, 10, conservative=False) == (3840, 768, 0, 0, 0, 0, 0, 0)
    assert footprint.rect(0.30, 0.06, 10) == (3840 + 184, 768 + 184, 0, 0, 0, 0, 0, 0)
    assert footprint.rect(0.0, 0.0, 10, conservative=False)[:2] == (0, 0) and footprint.rect(0.0, 0.0, 10)[:2] == (184, 184)
    assert footprint.rect(0.001, 0.001, 3, conservative=False)[:2] == (43, 43)                 # ceil(128 / 3)
    assert footprint.rect(0.1, 0.05, 7, ignore=9, near=(-3, 4000), conservative=False) == (1829, 915, 9, 1, -3, 4000, 0, 0)
    assert footprint.rect(1.28, 0.0, 10, conservative=False)[:2] == (16384, 0)
    assert footprint.INFLATE == R.INFLATE and (footprint.ROOMIEST, footprint.NEAREST) == (R.ROOMIEST, R.NEAREST)
    for bad in (dict(length=1.29, width=0.0, conservative=False), dict(length=1.28, width=0.0), dict(length=1.0, width=1.0),
                dict(length=-0.1, width=0.1), dict(length=0.1, width=0.1, ignore=128), dict(length=0.1, width=0.1, ignore=-1),
                dict(length=0.1, width=0.1, near=(4096, 0)), dict(length=0.1, width=0.1, near=(0, -4097)), dict(length=0.1, width=0.1, cell_mm=0)):
        kw = {**dict(cell_mm=10), **bad}
        with pytest.raises(ValueError):
            footprint.rect(**kw)
    half = torch.tensor([[[0.0, 0.0, 0.0], [0.02, 0.11, 0.3]]])
    fitted = types.SimpleNamespace(half=half)
    assert footprint.of_object(fitted, 0, 1, 10, conservative=False) == (2816, 512, 1, 0, 0, 0, 0, 0)
    assert footprint.of_object(fitted, 0, 1, 10, margin=0.01, near=(2, 3)) == (3072 + 184, 768 + 184, 1, 1, 2, 3, 0, 0)


def test_conservative_rectangles_cover_every_cell_they_touch():
    """The claim of rect(conservative=True): a real rectangle centred on a cell centre, turned by pi k / A, touches no cell
    outside the mask of the inflated record.  float64 separating axes between the cell's square and the rectangle."""
    rng = np.random.default_rng(7)
    cases = 0
    for _ in range(2200):
        A = int(rng.choice([1, 5, 16, 32]))
        k = int(rng.integers(0, A))
        a_mm = int(rng.integers(0, 601))                           # half length up to 60 cells of 10 mm, whole millimetres
        room = int(np.floor((np.sqrt(16384.0 ** 2 - (a_mm * 25.6 + 185) ** 2) - 185) / 25.6))
        b_mm = int(rng.integers(0, min(a_mm, max(room, 0)) + 1))
        rec = footprint.rect(2 * a_mm / 1000.0, 2 * b_mm / 1000.0, 10)
        assert rec[0] == -(-(2 * a_mm * 128) // 10) + 184 and rec[1] == -(-(2 * b_mm * 128) // 10) + 184
        dirs = R.direction_table(A)
        in_mask = set(R.mask_offsets(dirs, k, rec[0], rec[1]))
        a, b, th = a_mm / 10.0, b_mm / 10.0, np.pi * k / A
        u, v = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
        w = int(np.ceil(np.hypot(a, b))) + 2
        di, dj = np.meshgrid(np.arange(-w, w + 1), np.arange(-w, w + 1), indexing="ij")
        c = np.stack([di, dj], axis=-1).astype(np.float64)          # the cells' centres; the square has half side 0.5
        # separating axes: the square's (i, j) and the rectangle's (u, v)
        sep = (np.abs(c[..., 0]) > 0.5 + a * abs(u[0]) + b * abs(v[0])) | (np.abs(c[..., 1]) > 0.5 + a * abs(u[1]) + b * abs(v[1])) \
            | (np.abs(c @ u) > a + 0.5 * (abs(u[0]) + abs(u[1]))) | (np.abs(c @ v) > b + 0.5 * (abs(v[0]) + abs(v[1])))
        touched = [(int(x), int(y)) for x, y in zip(di[~sep], dj[~sep])]
        assert (0, 0) in touched
        missing = [t for t in touched if t not in in_mask]
        assert not missing, (A, k, a_mm, b_mm, missing[:4])
        cases += 1
    assert cases >= 2000


def test_engineered_grids_contain_what_they_are_used_for():
    E = R.ENGINEERED
    dirs2 = R.direction_table(2)
    bar = [R.record(640, 0)]
    st, ow = E["empty_table"]()
    out = R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 1)
    assert out["count"][0, :2].tolist() == [28 * 32, 32 * 28]      # the border band
    assert (out["fits"][0][:2, :] & 1 == 0).all() and (out["fits"][0][:, :2] & 2 == 0).all() and out["fits"][0][2, 2] == 3
    for name in ("all_obstacle", "all_unknown"):
        st, ow = E[name]()
        assert not R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 1)["fits"].any()
    st, ow = E["all_unknown"]()
    assert R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 0)["count"][0, :2].tolist() == [12 * 16, 16 * 12]
    st, ow = E["all_obstacle"]()
    assert not R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 0)["fits"].any()
    assert R.footprint(st, ow, R.clearance(st, ow), dirs2, [R.record(640, 0, ignore=4)], 1)["count"][0, 0] == 12 * 16
    st, ow = E["one_blocker"]()
    out = R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 1)
    assert out["count"][0, :2].tolist() == [28 * 32 - 5, 32 * 28 - 5]
    for name, k, n in (("corridor_i_5", 1, 32), ("corridor_i_4", 1, 0), ("corridor_j_5", 0, 32), ("corridor_j_4", 0, 0)):
        st, ow = E[name]()
        assert R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 1)["count"][0, k] == n, name
    st, ow = E["one_orientation"]()
    out = R.footprint(st, ow, R.clearance(st, ow), R.direction_table(16), [R.record(1920, 128)], 1)      # 15 x 1 cells
    assert out["count"][0, 8] == 3 and out["count"][0].sum() == 3 and out["best"][0, :4].tolist() == [1, 15, 13, 8]
    st, ow = E["last_row_column"]()
    out = R.footprint(st, ow, R.clearance(st, ow), dirs2, bar, 1)
    assert out["fits"][0][15, 2] == 2 and out["fits"][0][2, 15] == 1 and out["fits"][0][15, 13] == 2 and out["fits"][0][15, 14] == 0
    st, ow = E["only_obstacle"]()
    d2 = R.clearance(st, ow)
    seven, nine, none = (R.footprint(st, ow, d2, dirs2, [R.record(640, 0, ignore=g)], 1)["count"][0, 0] for g in (7, 9, 0))
    assert seven == 20 * 24 and nine == none < seven
    st, ow = E["out_of_contract"]()
    d2 = R.clearance(st, ow)
    point = [R.record(0, 0), R.record(0, 0, ignore=7)]
    blocked, open_ = R.footprint(st, ow, d2, dirs2, point, 1), R.footprint(st, ow, d2, dirs2, point, 0)
    assert blocked["count"][0, 0] == 24 * 24 - 6 and blocked["count"][1, 0] == 24 * 24 - 5              # (20, 12) is object 7
    assert open_["count"][0, 0] == 24 * 24 - 1 and open_["count"][1, 0] == 24 * 24
    for A, rects in R.ENGINEERED_SETS:
        R.check_params(R.direction_table(A), rects, 1)
    for G in (8, 64):
        st, ow, d2 = R.random_grid(G, 1)
        P = R.present_id(ow, st)
        assert ((st == 2) & (ow == P)).any() and (d2 == -1).any() or G == 8
        for A, specs, ub in R.RANDOM_SETS:
            R.check_params(R.direction_table(A), R.resolve(specs, P), ub)
    st, ow, d2 = R.random_grid(256, 1)
    assert {-1, 0, 1, 2, 3} <= set(np.unique(st).tolist()) and {-5, 0, 128, 129} <= set(np.unique(ow).tolist())
    assert {-1, 70000} <= set(np.unique(d2).tolist())
    limits = [r for _, specs, _ in R.RANDOM_SETS for r in specs]
    assert any(r[1] == 16384 for r in limits) and any(r[2] == 16384 for r in limits) and any(r[1:3] == (0, 0) for r in limits)
    assert {len(specs) for _, specs, _ in R.RANDOM_SETS} >= {1, 8} and {A for A, _, _ in R.RANDOM_SETS} >= {1, 32}


def test_grid_of_72_has_fitting_cells_past_the_first_ballot_word():
    """What tests/test_footprint_gpu.py's G = 72 case is there for: columns 64..71 are the second ballot word of a row."""
    st, ow, d2 = R.random_grid(72, 1)
    A, specs, ub = R.RANDOM_SETS[0]
    out = R.footprint(st, ow, d2, R.direction_table(A), R.resolve(specs, R.present_id(ow, st)), ub)
    assert (out["fits"][:, :, 64:] != 0).any()


def test_error_paths_through_ctypes():
    lib = _native.lib()
    B, G, A, F = 2, 16, 4, 2
    wsb = lib.uoc_footprint_workspace_bytes
    nws = wsb(B, G, A, F)
    assert nws >= B * F * G * G * 2 + F * A * 131 * 2
    assert wsb(0, G, A, F) == 0 and wsb(65536, G, A, F) == 0 and wsb(65535, G, A, F) > 0 and wsb(-1, G, A, F) == 0
    assert wsb(B, 0, A, F) == 0 and wsb(B, 12, A, F) == 0 and wsb(B, 520, A, F) == 0 and wsb(B, 512, A, F) > 0 and wsb(B, 8, A, F) > 0
    assert wsb(B, G, 0, F) == 0 and wsb(B, G, 33, F) == 0 and wsb(B, G, 32, F) > 0
    assert wsb(B, G, A, 0) == 0 and wsb(B, G, A, 9) == 0 and wsb(B, G, A, 8) > 0
    fake = ctypes.c_void_p(0x1000)                                   # never dereferenced: validation comes first
    good_dirs = R.direction_table(A).reshape(-1).tolist()
    good_rects = list(R.record(640, 200)) + list(R.record(300, 0, 5, R.NEAREST, -4096, 4095))

    def call(B_=B, G_=G, dirs=good_dirs, A_=A, rects=good_rects, F_=F, ub=1, nws_=nws, ws_=fake, drop=None):
        hd = (ctypes.c_int32 * max(len(dirs), 1))(*dirs)
        hr = (ctypes.c_int32 * max(len(rects), 1))(*rects)
        p = {k: fake for k in ("state", "owner", "dist2", "frame", "fits", "count", "best")}
        p["dirs"], p["rects"], p["ws"] = ctypes.cast(hd, ctypes.c_void_p), ctypes.cast(hr, ctypes.c_void_p), ws_
        if drop:
            p[drop] = None
        return lib.uoc_footprint(p["state"], p["owner"], p["dist2"], p["frame"], B_, G_, p["dirs"], A_, p["rects"], F_, ub, p["fits"],
                                 p["count"], p["best"], p["ws"], nws_, None)

    def rects_with(**kw):
        base = dict(HL=640, HW=200, ignore=0, mode=0, ai=0, aj=0, w6=0, w7=0)
        base.update(kw)
        return good_rects[:8] + [base[k] for k in ("HL", "HW", "ignore", "mode", "ai", "aj", "w6", "w7")]

    over = [16384] * 2 * A
    bad = [dict(drop=k) for k in ("state", "owner", "dist2", "dirs", "rects", "fits", "count", "best", "ws")] + [
        dict(B_=0), dict(B_=-1), dict(B_=65536), dict(G_=0), dict(G_=12), dict(G_=520), dict(G_=-8), dict(A_=0), dict(A_=33), dict(F_=0),
        dict(F_=9), dict(ub=2), dict(ub=-1), dict(dirs=over[:-1] + [16385]), dict(dirs=[-16385] + over[1:]),
        dict(rects=rects_with(HL=16385, HW=0)), dict(rects=rects_with(HL=0, HW=16385)), dict(rects=rects_with(HL=-1)), dict(rects=rects_with(HW=-1)),
        dict(rects=rects_with(HL=16384, HW=1)), dict(rects=rects_with(HL=11586, HW=11585)), dict(rects=rects_with(ignore=128)),
        dict(rects=rects_with(ignore=-1)), dict(rects=rects_with(mode=2)), dict(rects=rects_with(mode=-1)), dict(rects=rects_with(ai=4096)),
        dict(rects=rects_with(ai=-4097)), dict(rects=rects_with(aj=4096)), dict(rects=rects_with(aj=-4097)), dict(rects=rects_with(w6=1)),
        dict(rects=rects_with(w7=-1)), dict(rects=rects_with(HL=16385) + good_rects[8:], F_=3),
        dict(nws_=nws - 1), dict(nws_=0), dict(ws_=ctypes.c_void_p(0x1008)), dict(ws_=ctypes.c_void_p(0x1004))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert lib.uoc_last_error()
    for kw, word in ((dict(ws_=ctypes.c_void_p(0x1004)), b"aligned"), (dict(drop="dist2"), b"null"), (dict(A_=33), b"directions"),
                     (dict(F_=9), b"rectangles"), (dict(rects=rects_with(ignore=128)), b"ignore"), (dict(rects=rects_with(mode=2)), b"mode"),
                     (dict(rects=rects_with(ai=4096)), b"anchor"), (dict(rects=rects_with(w6=1)), b"reserved"), (dict(G_=12), b"grid"),
                     (dict(nws_=nws - 1), b"workspace"), (dict(rects=rects_with(HL=16385, HW=0)), b"HL"),
                     (dict(rects=rects_with(HL=16384, HW=1)), b"HL^2"), (dict(dirs=over[:-1] + [16385]), b"direction")):
        assert call(**kw) == EINVAL and word in lib.uoc_last_error(), (kw, lib.uoc_last_error())
    assert (11585 ** 2) * 2 <= 16384 ** 2 < 11586 ** 2 + 11585 ** 2


def test_wrapper_value_errors():
    cpu = torch.zeros((1, 16, 16), dtype=torch.int32)
    dirs = R.direction_table(4)
    with pytest.raises(_native.NativeError):
        footprint.footprint_records(cpu, cpu, cpu, None, dirs, [R.record(0, 0)], 1)       # no CPU fallback
    for rects in ([], [R.record(0, 0)] * 9, [R.record(16385, 0)], [R.record(11586, 11585)], [R.record(1, 1, ignore=128)],
                  [R.record(1, 1, mode=2)], [R.record(1, 1, ai=4096)], [(1, 1, 0, 0, 0, 0, 1, 0)], [(1, 1, 0)], [R.record(-1, 0)]):
        with pytest.raises(ValueError):
            footprint._check_rects(rects)
    assert footprint._check_rects(R.record(5, 6)).tolist() == [[5, 6, 0, 0, 0, 0, 0, 0]]
    placed = types.SimpleNamespace(state=cpu, owner=cpu, dist2=cpu, frame=None, grid=16, cell_mm=10, planes=None, unknown_blocks=True)
    for kw in (dict(angles=0), dict(angles=33), dict(rects=[R.record(16385, 0)])):
        with pytest.raises(ValueError):
            footprint.fit(placed, **{**dict(rects=[R.record(0, 0)]), **kw})
    res = types.SimpleNamespace(fits=torch.tensor([[[[0, 5], [2, -2147483648]]]], dtype=torch.int32), angles=32)
    assert footprint.fits_mask(res, 0).tolist() == [[[False, True], [True, True]]]
    assert footprint.fits_mask(res, 0, 0).tolist() == [[[False, True], [False, False]]]
    assert footprint.fits_mask(res, 0, 31).tolist() == [[[False, False], [False, True]]]
    with pytest.raises(ValueError):
        footprint.fits_mask(res, 0, 32)


def test_pose_on_a_synthetic_result():
    from unseenobjectclustering_amd import placement
    planes = torch.from_numpy(placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0]))
    best = torch.tensor([[[1, 10, 3, 4, 25, 0, 7, 5], list(R.NO_POSE)]], dtype=torch.int32)
    res = types.SimpleNamespace(best=best, dirs=R.direction_table(16), angles=16, planes=planes, grid=16, cell_mm=10)
    assert footprint.pose(res, 0, 1) is None
    p = footprint.pose(res, 0, 0)
    assert (p.k, p.cell, p.dist2) == (4, (10, 3), 25) and abs(p.angle - np.pi / 4) < 1e-15
    assert np.allclose(p.center, placement.cell_to_camera(res, 0, 10, 3), rtol=0, atol=1e-15)
    assert np.allclose(p.center, [0.025, 0.045, 1.0], rtol=0, atol=1e-12)
    assert np.allclose(p.axis, [np.sqrt(0.5), -np.sqrt(0.5), 0.0], rtol=0, atol=1e-4) and abs(np.linalg.norm(p.axis) - 1) < 1e-12
