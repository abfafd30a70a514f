"""One small case per C entry point that takes caller scratch or caller state (include/uoc_hip.h: a parameter d_ws, d_state
or d_mem), for tests/test_workspace_contract_gpu.py.  tests/test_workspace_contract_host.py holds the table to the header:
a new stage without a case here fails there.

A case runs its entry on guarded scratch (tests/scratch_guard.py) of exactly the size function's value and returns the
outputs as named host arrays; its check compares them with the stage's existing reference module through the comparison
helper of the stage's own GPU file, tolerances unchanged.  No reference is written here.

    run(device, shape, rec) -> (bits, raw)     rec: a scratch_guard.Record (fill, offset, alignment); every scratch and
                                               state buffer of the call comes from rec.take or, through the public wrapper,
                                               from guard_workspaces(record=rec); bits: {name: numpy array}; raw: whatever
                                               the check needs beside them
    check(shape, bits, raw)                    asserts

Shapes are the smallest at which a carve has all its regions, more than one frame and more than one block: always B = 2
(frame 1's regions start at the rounded stride); label maps 37 x 53 (odd: scalar loads, two 1024-pixel blocks) and 24 x 32
(n % 4 == 0: vector loads); grids G = 40 (the partial strip of the column pass) and G = 8; clustering n = 1961 with m = 34
and m = 100, both sampling kernels, both metrics, two halves for the wide and the confidence calls.

align: what the entry asks of d_ws.  16 for all but the clustering, network and evaluation entries, whose argument checks
refuse anything below 256 (the header says so); those are run at 256 modulo 512 instead of at 16 modulo 256."""
import ctypes
import functools
import importlib

import numpy as np
import torch

from tests.scratch_guard import guard_workspaces
from unseenobjectclustering_amd import _native

LABEL_SHAPES = [(37, 53), (24, 32)]
GRIDS = [40, 8]
MS_N, MS_M = 1961, (34, 100)
B = 2

EXEMPT = {
    "uoc_conv2d_nhwc": "owns its buffers; no caller scratch",
    "uoc_conv2d_nhwc_algo": "owns its Winograd scratch (NaN-poisoned through this entry in tests/test_wino4_skip_gpu.py)",
    "uoc_conv2d_nhwc_tile": "owns its Winograd scratch, as uoc_conv2d_nhwc_algo",
}


def mod(name):
    """A test or reference module, imported when a case needs it: the table itself imports nothing heavy."""
    return importlib.import_module("tests." + name)


def up(device, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    return t.detach().cpu().numpy()


def tensors_of(res):
    """Every tensor attribute of a result object as a host array."""
    return {k: host(v) for k, v in vars(res).items() if isinstance(v, torch.Tensor)}


def exact(rec, size_name, *shape):
    """A guarded buffer of exactly lib().<size_name>(*shape) bytes -> (view, bytes)."""
    n = int(getattr(_native.lib(), size_name)(*shape))
    assert n > 0, (size_name, shape)
    return rec.take(size_name, n), n


class Case:
    def __init__(self, shapes, run, check, align=16, kind="scratch"):
        self.shapes, self.run, self.check, self.align, self.kind = shapes, run, check, align, kind


# ---- label-map stages ----------------------------------------------------------------------------------------------------
def frames_of(make, *seeds):
    """[(lab, xyz)] per seed -> stacked (labels [B,H,W], xyz [B,3,H,W]) and the frames."""
    frames = [make(s) for s in seeds]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), frames


REL = dict(connectivity=8, gap_mm=15, min_pairs=4)


def relations_run(device, shape, rec):
    from unseenobjectclustering_amd import relations
    T = mod("test_relations_gpu")
    lab, xyz, _ = frames_of(lambda s: T.scene(*shape, s), 1, 2)
    with guard_workspaces(record=rec):
        res = relations.relate(up(device, lab), up(device, xyz), connectivity=REL["connectivity"], gap=REL["gap_mm"] / 1000.0,
                               min_pairs=REL["min_pairs"])
    R = mod("relations_reference")
    return {k: host(getattr(res, k)) for k in R.TABLES + R.FIELDS}, None


def relations_check(shape, bits, raw):
    T, R = mod("test_relations_gpu"), mod("relations_reference")
    for b, seed in enumerate((1, 2)):
        lab, xyz = T.scene(*shape, seed)
        T.check_frame({k: v[b] for k, v in bits.items()}, R.relations(lab, xyz[2], REL["connectivity"], REL["gap_mm"], REL["min_pairs"]),
                      (shape, b))


CC = dict(connectivity=8, min_area=2)


def cc_run(device, shape, rec):
    from unseenobjectclustering_amd import components
    maps = up(device, mod("test_components_gpu").tabletop(*shape))
    bits = {}
    with guard_workspaces(record=rec):
        for mode in ("all", "largest"):
            out, table, counts = components.split_components(maps, mode=mode, **CC)
            bits.update({mode + "/out": host(out), mode + "/table": host(table), mode + "/counts": host(counts)})
    return bits, None


def cc_check(shape, bits, raw):
    T = mod("test_components_gpu")
    for mode in ("all", "largest"):
        want = T.reference(("tabletop",) + tuple(shape), CC["connectivity"], CC["min_area"], mode)
        for k, w in zip(("out", "table", "counts"), want):
            assert np.array_equal(bits[mode + "/" + k], w), (shape, mode, k)


OBJECT_KEYS = ("frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
               "obb_center", "obb_half", "points", "pixel_index", "attrs", "offsets")


@functools.lru_cache(maxsize=None)
def objects_scene(shape):
    return mod("test_objects_gpu").synthetic(B, *shape, seed=shape[0] * 7 + shape[1])


def objects_run(device, shape, rec):
    from unseenobjectclustering_amd import objects as O
    lab, xyz, attrs = objects_scene(shape)
    with guard_workspaces(record=rec):
        objs = O.extract_objects(up(device, lab), up(device, xyz), attrs=up(device, attrs), min_points=0)
    return {k: host(getattr(objs, k)) for k in OBJECT_KEYS}, objs


def objects_check(shape, bits, raw):
    lab, xyz, attrs = objects_scene(shape)
    K, _ = mod("test_objects_gpu").check_against_reference(raw, lab, xyz, attrs)
    assert K > 0


PLANE = dict(num_hyp=64, tau_mm=10, seed=1, noise=0.0005)


def plane_run(device, shape, rec):
    from unseenobjectclustering_amd import support
    T = mod("test_support_gpu")
    lab, xyz, _ = frames_of(lambda s: T.scene(*shape, s, PLANE["noise"]), 1, 2)
    with guard_workspaces(record=rec):
        res = support.fit_plane(up(device, lab), up(device, xyz), num_hyp=PLANE["num_hyp"], tau=PLANE["tau_mm"] / 1000.0,
                                seed=PLANE["seed"], height_map=True)
    return tensors_of(res), res


def plane_check(shape, bits, raw):
    T, R = mod("test_support_gpu"), mod("support_reference")
    found = 0
    for b, s in enumerate((1, 2)):
        lab, xyz = T.scene(*shape, s, PLANE["noise"])
        want = R.fit(lab, xyz, PLANE["num_hyp"], PLANE["tau_mm"], PLANE["seed"], height_map=True)
        T.check_frame(T.host(raw, b), want, (shape, b))
        found += int(want["plane"]["found"])
    assert found == B


PLANES = dict(K=4, num_hyp=256, tau_mm=10, rem_mm=20, seed=1)


def planes_run(device, shape, rec):
    from unseenobjectclustering_amd import support
    T = mod("test_planes_gpu")
    lab, xyz, _ = frames_of(lambda s: T.shelves(*shape, s), 1, 2)
    with guard_workspaces(record=rec):
        res = support.fit_planes(up(device, lab), up(device, xyz), max_planes=PLANES["K"], num_hyp=PLANES["num_hyp"],
                                 tau=PLANES["tau_mm"] / 1000.0, remove=PLANES["rem_mm"] / 1000.0, seed=PLANES["seed"])
    return tensors_of(res), res


def planes_check(shape, bits, raw):
    T, P = mod("test_planes_gpu"), mod("planes_reference")
    mi = P.default_min_inliers(*shape)
    assert raw.min_inliers == mi
    for b, s in enumerate((1, 2)):
        want = T.reference(("shelves",) + tuple(shape) + (s,), PLANES["K"], PLANES["num_hyp"], PLANES["tau_mm"], PLANES["rem_mm"], mi,
                           PLANES["seed"])
        assert want["count"] >= 2
        T.check_planes(raw, b, want, (shape, b))


def normals_inputs(shape):
    T, R = mod("test_normals_gpu"), mod("normals_reference")
    frames = [T.boxes(*shape, s) for s in (1, 2)]
    return np.stack([f[1] for f in frames]), np.stack([f[0] for f in frames]), [R.table_plane()] * B


def normals_run(device, shape, rec):
    T = mod("test_normals_gpu")
    xyz, lab, planes = normals_inputs(shape)
    with guard_workspaces(record=rec):
        n, info, faces, _ = T.run(device, xyz, lab, planes)
    return dict(n=n, info=info, faces=faces), None


def normals_check(shape, bits, raw):
    T, R = mod("test_normals_gpu"), mod("normals_reference")
    xyz, lab, planes = normals_inputs(shape)
    T.check((bits["n"], bits["info"], bits["faces"]), R.estimate_batch(xyz, lab, planes, **T.ref_kwargs(**T.DEFAULTS)), shape)


def signature_frames(kind, shape):
    """B frames (labels, image, xyz) of one of the three maps the accumulator's contract is run on."""
    T = mod("test_identity_gpu")
    if kind == "tabletop":
        return [T.scene(1000 * shape[0] + shape[1] + k, *shape) for k in range(B)]
    if kind == "outside":                       # only out-of-range ids: no id ever votes
        out = []
        for k in range(B):
            lab, img, xyz = T.scene(77 + k, *shape)
            outside = np.array([0, -1, 128, 129, -2 ** 31, 2 ** 31 - 1], np.int32)
            out.append((outside[np.arange(lab.size).reshape(lab.shape) % 6], img, xyz))
        return out
    W = mod("test_wave_groups_gpu")             # "2x64": 64 distinct keys in one wave and a wave without any
    maps = [W.MAPS["2x64"], W.MAPS["2x64_127"]]
    rng = np.random.default_rng(5)
    return [(m, rng.integers(0, 256, size=m.shape + (3,)).astype(np.uint8), mod("relations_reference").xyz_of(W.depth(m, 5 + k)))
            for k, m in enumerate(maps)]


SIGNATURE_MAPS = ("tabletop", "outside", "2x64")


def signature_run(device, shape, rec):
    """uoc_signature's scratch has a stated precondition (all zero before, all zero after): three calls on ONE zeroed
    guarded accumulator, which must be all zero after each."""
    from unseenobjectclustering_amd import identity
    identity._acc.items.clear()                 # the accumulator of this run comes from the guard
    bits = {}
    try:
        with guard_workspaces(record=rec):
            for kind in SIGNATURE_MAPS:
                frames = signature_frames(kind, shape)
                lab, img, xyz = (up(device, np.stack([f[k] for f in frames])) for k in range(3))
                bits[kind + "/sig"] = host(identity.describe(lab, img, xyz).sig)
                acc = identity._acc.of_device(torch.device(device))
                assert len(acc) == 1 and len(rec.items) == 1 and acc[0].data_ptr() == rec.items[0].address
                assert acc[0].numel() == _native.lib().uoc_signature_workspace_bytes(B)
                bits[kind + "/acc_nonzero"] = np.array([int(torch.count_nonzero(acc[0]))])
    finally:
        identity._acc.items.clear()             # and does not outlive it
    return bits, None


def signature_check(shape, bits, raw):
    ir = mod("identity_reference")
    for kind in SIGNATURE_MAPS:
        want = np.stack([ir.describe(*f) for f in signature_frames(kind, shape)])
        assert np.array_equal(bits[kind + "/sig"], want), (shape, kind)
        assert int(bits[kind + "/acc_nonzero"][0]) == 0, (shape, kind, "the accumulator is not all zero after the call")
    assert not bits["outside/sig"].any() and bits["tabletop/sig"][..., 0].any() and (bits["2x64/sig"][0, 1:64, 0] == 1).all()


TRACK = dict(min_iou=0.3, max_age=5, steps=3)


def track_frames(shape):
    T = mod("test_tracking_gpu")
    return [T.make_sequence(seed, *shape)[:TRACK["steps"]] for seed in (1, 2)]


def track_run(device, shape, rec):
    from unseenobjectclustering_amd import tracking
    seqs = track_frames(shape)
    bits = {}
    with guard_workspaces(record=rec):          # the state comes from the guard too, poisoned: the tracker resets it
        tr = tracking.Tracker(min_iou=TRACK["min_iou"], max_age=TRACK["max_age"], streams=B)
        for t in range(TRACK["steps"]):
            out = tr.update(up(device, np.stack([s[t] for s in seqs])))
            bits.update({"out%d" % t: host(out), "lut%d" % t: host(tr.lut), "table%d" % t: host(tr.table),
                         "state%d" % t: host(tr.state_words)})
    assert sorted(rec.names()) == ["uoc_track_state_bytes", "uoc_track_workspace_bytes"]
    return bits, None


def track_check(shape, bits, raw):
    T = mod("test_tracking_gpu")
    hdr, cont, meta = _native.TRACK_HEADER_WORDS, _native.TRACK_CONT_WORDS, _native.TRACK_META_WORD
    n = shape[0] * shape[1]
    for b, frames in enumerate(track_frames(shape)):
        steps, _ = T.run_reference(frames, TRACK["min_iou"], TRACK["max_age"])
        for t, (out8, lut, table, mem8, m) in enumerate(steps):
            where = (shape, b, t)
            words = bits["state%d" % t][b]
            assert np.array_equal(bits["out%d" % t][b], out8.astype(np.int32)), where
            assert np.array_equal(bits["lut%d" % t][b], lut) and np.array_equal(bits["table%d" % t][b], table), where
            assert np.array_equal(words[:128 * 5].reshape(128, 5), table), where
            assert (int(words[meta]) + 1, int(words[meta + 1]), int(words[meta + 2])) == (m["next_uid"], m["step"], m["dropped"]), where
            assert np.array_equal(words[hdr + cont:hdr + cont + n].reshape(shape), mem8.astype(np.int32)), where
            assert not words[hdr:hdr + cont].any(), where


# ---- grid stages ---------------------------------------------------------------------------------------------------------
GRID_LABEL_SHAPES = [(37, 53, 40), (24, 32, 8)]


def placement_params(G):
    return (40, 10, 10, 10, 1, 0) if G == 40 else (8, 50, 20, 8, 1, 0)     # as tests/test_placement_gpu.py: G = 40, PARAMS[4]


def placement_run(device, shape, rec):
    from unseenobjectclustering_amd import placement
    T, R = mod("test_placement_gpu"), mod("placement_reference")
    H, W, G = shape
    lab, xyz, _ = frames_of(lambda s: T.scene(H, W, s), 1, 2)
    plane = R.true_plane()
    with guard_workspaces(record=rec):
        res = placement.free_space(up(device, lab), up(device, xyz), tuple(plane[k] for k in ("normal", "d", "centroid", "u", "v")),
                                   **T.kwargs(placement_params(G), T.scene_queries(G)))
    return tensors_of(res), res


def placement_check(shape, bits, raw):
    T, R = mod("test_placement_gpu"), mod("placement_reference")
    H, W, G = shape
    for b, s in enumerate((1, 2)):
        lab, xyz = T.scene(H, W, s)
        T.check_frame(T.host(raw, b), R.free_space(lab, xyz, R.true_plane(), *placement_params(G), T.scene_queries(G)), (shape, b))


def elevation_params(G):
    return dict(cell=20 if G == 40 else 40, tau=10, step=5, min_pts=1, nobj=4)


def elevation_run(device, shape, rec):
    from unseenobjectclustering_amd import elevation
    T = mod("test_elevation_gpu")
    H, W, G = shape
    p = elevation_params(G)
    lab, xyz, _ = frames_of(lambda s: T.scene(H, W, s, p["nobj"]), 1, 2)
    qs = T.scene_queries(p["cell"])[:3]
    with guard_workspaces(record=rec):
        res = elevation.heights(up(device, lab), up(device, xyz), T.placed_of(device, np.stack([T.TRUE_F] * B), G, p["cell"], p["tau"]),
                                step=p["step"] / 1000.0, min_pts=p["min_pts"], queries=qs)
    return {k: host(getattr(res, k)) for k in T.KEYS}, res


def elevation_check(shape, bits, raw):
    T, R = mod("test_elevation_gpu"), mod("elevation_reference")
    H, W, G = shape
    p = elevation_params(G)
    qs = T.scene_queries(p["cell"])[:3]
    for b, s in enumerate((1, 2)):
        lab, xyz = T.scene(H, W, s, p["nobj"])
        T.check_frame({k: v[b] for k, v in bits.items()}, R.heights(lab, xyz, T.TRUE_F, G, p["cell"], p["tau"], p["step"], p["min_pts"], qs),
                      (shape, b))


GRASP_CFG = (2, 2, 8, 1, 1, 1, 1)               # A = 2 directions, M = 2 offsets: the smallest above 1


def grasp_run(device, G, rec):
    T = mod("test_grasp_gpu")
    frames = [T.random_grid(G, s) for s in (1, 2)]
    with guard_workspaces(record=rec):
        cand, best = T.run(device, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), GRASP_CFG)
    return dict(cand=cand, best=best), None


def grasp_check(G, bits, raw):
    T = mod("test_grasp_gpu")
    for b, s in enumerate((1, 2)):
        T.check(bits["cand"][b], bits["best"][b], *T.random_grid(G, s), GRASP_CFG, (G, b))


FOOT_A = 2


def footprint_inputs(G):
    T, R = mod("test_footprint_gpu"), mod("footprint_reference")
    frames = [T.random_grid(G, s) for s in (1, 2)]
    _, specs, ub = R.RANDOM_SETS[5 % len(R.RANDOM_SETS)]
    rects = R.resolve(specs, R.present_id(frames[0][1], frames[0][0]))
    return frames, rects, ub


def footprint_run(device, G, rec):
    T = mod("test_footprint_gpu")
    frames, rects, ub = footprint_inputs(G)
    with guard_workspaces(record=rec):
        got = T.run(device, *(np.stack([f[k] for f in frames]) for k in range(3)), FOOT_A, rects, ub)
    return got, None


def footprint_check(G, bits, raw):
    T, R = mod("test_footprint_gpu"), mod("footprint_reference")
    frames, rects, ub = footprint_inputs(G)
    assert len(rects) >= 2
    for b in range(B):
        T.check(bits, b, R.footprint(*frames[b], R.direction_table(FOOT_A), rects, ub), (G, b))


def routes_inputs(G):
    T, R = mod("test_routes_gpu"), mod("routes_reference")
    frames = [T.random_grid(G, s) for s in (1, 2)]
    queries = R.random_queries(G, 1, *frames[0])
    picked = [queries[0]] + [q for q in queries[1:] if (q[5], q[0]) != (queries[0][5], queries[0][0])][:1] + [queries[-1]]
    return frames, picked                       # Q = 3: queries that share a passability map and queries that do not


def routes_run(device, G, rec):
    T = mod("test_routes_gpu")
    frames, queries = routes_inputs(G)
    with guard_workspaces(record=rec):
        got = T.run(device, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), queries, 1, 64)
    return got, None


def routes_check(G, bits, raw):
    T, R = mod("test_routes_gpu"), mod("routes_reference")
    frames, queries = routes_inputs(G)
    assert len(queries) == 3
    for b in range(B):
        T.check(bits, b, R.routes(*frames[b], queries, 1, 64), (G, b))


MOTION = dict(A=2, radius=2)


def motion_run(device, G, rec):
    T, R = mod("test_motion_gpu"), mod("motion_reference")
    frames = [T.blobs(G, s) for s in (1, 2)]
    with guard_workspaces(record=rec):
        got = T.run(device, *(np.stack([f[k] for f in frames]) for k in range(4)), MOTION["A"], MOTION["radius"], R.BLOB_PAIRS[:2])
    return got, None


def motion_check(G, bits, raw):
    T, R = mod("test_motion_gpu"), mod("motion_reference")
    for b, s in enumerate((1, 2)):
        T.check(bits, b, R.motion(*T.blobs(G, s), R.rotation_table(MOTION["A"]), MOTION["radius"], R.BLOB_PAIRS[:2]), (G, b))


SCENE = dict(max_age=30, ub=1, steps=3)


def scene_state(rec, device, G, fill=0):
    """The streams' state as a guarded buffer of exactly uoc_scene_state_bytes(B, G) -> int32 [B, words]."""
    from unseenobjectclustering_amd import scene
    n = int(_native.lib().uoc_scene_state_bytes(B, G))
    assert n == B * scene.state_words(G) * 4
    return rec.take("uoc_scene_state_bytes", n, fill, device).view(torch.int32).view(B, -1)


def scene_run(device, G, rec):
    from unseenobjectclustering_amd import scene
    T = mod("test_scene_gpu")
    mem = scene_state(rec, device, G)           # a fresh stream is all zero: the state is an input, only d_ws is poisoned
    bits = {}
    with guard_workspaces(record=rec):
        for t, frames in enumerate(T.seeded(G, B, SCENE["steps"])):
            s, o, frame, drop = T.stack_frames(frames, B)
            out = scene.scene_records(up(device, s), up(device, o), up(device, frame), up(device, drop), mem, SCENE["max_age"], SCENE["ub"],
                                      T.scene_queries(G))
            bits.update({"%s%d" % (k, t): host(v) for k, v in zip(T.KEYS, out)})
            bits["mem%d" % t] = host(mem)
    return bits, None


def scene_check(G, bits, raw):
    T, R = mod("test_scene_gpu"), mod("scene_reference")
    ref = R.new_state(B, G)
    for t, frames in enumerate(T.seeded(G, B, SCENE["steps"])):
        want = R.step(ref, *T.stack_frames(frames, B), SCENE["max_age"], SCENE["ub"], T.scene_queries(G))
        T.compare({k: bits["%s%d" % (k, t)] for k in want}, want, (G, t))
        T.compare({"mem": bits["mem%d" % t]}, {"mem": ref}, (G, t))


IDENT_CASES = ("threshold_inclusive", "orphaned_uid_returns")     # three steps each from an all-zero state, the same q, r, max_lost


def ident_inputs():
    T = mod("test_identity_gpu")
    cases = [T.reference(name) for name in IDENT_CASES]
    assert all(len(c.steps) == 3 and not c.initial_words().any() for c, _ in cases)
    assert len({(c.q, c.r, c.max_lost) for c, _ in cases}) == 1
    return cases, T.ALL_IDS


def ident_run(device, shape, rec):
    from unseenobjectclustering_amd import identity
    cases, ids = ident_inputs()
    bits = {}
    with guard_workspaces(record=rec):          # state and plan both from the guard, poisoned: the identifier resets its state
        ident = identity.Identifier(streams=B)
        ident.q, ident.r, ident.max_lost = cases[0][0].q, cases[0][0].r, cases[0][0].max_lost
        ident.allocate(device, *ids.shape)
        tracked = up(device, np.stack([ids] * B))
        for t in range(3):
            tracks, sig = (up(device, np.stack([c.steps[t][k] for c, _ in cases])) for k in range(2))
            out = ident.step_tables(tracks, sig, tracked)
            bits.update({"out%d" % t: host(out), "lut%d" % t: host(ident.lut), "table%d" % t: host(ident.table),
                         "words%d" % t: host(ident.state_words)})
    assert sorted(rec.names()) == ["uoc_ident_state_bytes", "uoc_ident_workspace_bytes"]
    return bits, None


def ident_check(shape, bits, raw):
    ir = mod("identity_reference")
    cases, ids = ident_inputs()
    for b, (case, run) in enumerate(cases):
        for t in range(3):
            where = (case.name, t)
            assert np.array_equal(bits["lut%d" % t][b], run[t]["lut"]), where
            assert np.array_equal(bits["out%d" % t][b], run[t]["lut"][ir.object_ids(ids)]), where
            assert np.array_equal(bits["table%d" % t][b], run[t]["table"]), where
            assert np.array_equal(bits["words%d" % t][b], run[t]["words"]), where


# ---- clustering: the raw entries with exactly uoc_ms_workspace_bytes -----------------------------------------------------------
COS, EUC = _native.METRIC_COSINE, _native.METRIC_EUCLIDEAN


def ms_modules(metric):
    """(cases, reference, epsilon of the exact whole call) of a metric."""
    if metric == COS:
        return mod("ms_cosine_cases"), mod("ms_cosine_reference"), mod("ms_cosine_cases").EPS_PRODUCT
    return mod("ms_euclidean_cases"), mod("ms_euclidean_reference"), mod("ms_euclidean_cases").WHOLE_EPS


@functools.lru_cache(maxsize=None)
def ms_exact_fields(metric, wide):
    """B fields whose fp32 arithmetic is exact in every summation order (the whole-call fields of the metric's cases)."""
    CS = ms_modules(metric)[0]
    return [CS.whole_field(MS_N, k, wide) for k in range(B)]


def ms_firsts():
    return [(37 * k + 11) % MS_N for k in range(B)]


def ms_planes(fields, wide):
    R = mod("ms_cosine_reference")
    return np.stack([R.planes(f) if wide else f for f in fields])


def ms_ws(rec, n, m, halves=1):
    if halves == 1:
        return exact(rec, "uoc_ms_workspace_bytes", B, n, m)
    return exact(rec, "uoc_ms_workspace_bytes_wide", B, n, m, halves)


def ms_both_kernels(fn):
    """fn(kernel name) -> bits under the on-chip sampling kernel and under the streaming one, the keys prefixed."""
    bits = {}
    mod("ms_stage_calls").both_sampling_kernels(lambda kernel: bits.update({kernel + "/" + k: v for k, v in fn(kernel).items()}))
    return bits


def ms_select_case(entry, metrics, num_init):
    """uoc_ms_select_seeds / _from / _ex: exact fields, every index and seed row against the float64 restatement."""
    def inputs(metric, m):
        R = ms_modules(metric)[1]
        fields = ms_exact_fields(metric, False)
        init = None
        if num_init:                            # the continuation: the first rows given, as the reference's init_seeds
            init = np.zeros((B, m, 64), np.float32)
            for b, X in enumerate(fields):
                init[b, :num_init] = X[R.select_seeds(X, num_init, ms_firsts()[b])[0]]
        return fields, init

    def run(device, shape, rec):
        m, metric = shape

        def one(kernel):
            fields, init = inputs(metric, m)
            X = up(device, np.stack(fields))
            seeds = torch.full((B, m, 64), 9.0, device=device) if init is None else up(device, init)
            idx = torch.full((B, m), -7, dtype=torch.int32, device=device)
            first = None if num_init else torch.tensor(ms_firsts(), dtype=torch.int32, device=device)
            ws, n = ms_ws(rec, MS_N, m)
            head = (X, B, MS_N, m) + ((num_init,) if entry != "uoc_ms_select_seeds" else ())
            tail = ((metric,) if entry.endswith("_ex") else ()) + (ws, n)
            _native.call(entry, device, *head, first, seeds, idx, *tail)
            _native.call("uoc_ms_check", device)
            return dict(idx=host(idx), seeds=host(seeds))
        return ms_both_kernels(one), None

    def check(shape, bits, raw):
        m, metric = shape
        R = ms_modules(metric)[1]
        fields, init = inputs(metric, m)
        for b, X in enumerate(fields):
            if num_init:
                want, _ = R.select_seeds(X, m, None, init[b], num_init)
                rows = R.seed_rows(X, want, init[b])
            else:
                want, _ = R.select_seeds(X, m, ms_firsts()[b])
                rows = R.seed_rows(X, want)
            for kernel in ("on-chip", "streaming"):
                assert np.array_equal(bits[kernel + "/idx"][b], want), (entry, shape, kernel, b)
                assert np.array_equal(bits[kernel + "/seeds"][b], rows), (entry, shape, kernel, b)
    return Case([(m, met) for m in MS_M for met in metrics], run, check, align=256)


@functools.lru_cache(maxsize=None)
def climb_yardstick(metric, field_key, seeds_key):
    """The float64 climb and the tolerance of the metric's own file (ms_*_cases.climb_yardstick / climb_tolerance), once per
    (field, seeds): the yardstick costs seconds."""
    CS = ms_modules(metric)[0]
    out = CS.climb_yardstick(_KEPT[field_key], _KEPT[seeds_key], CS.KAPPA, 10)
    return (out[0], CS.climb_tolerance(*out[1:])) if metric == COS else (out[0], CS.climb_tolerance(out[1]))


_KEPT = {}


def climb_check(metric, got, field, seeds, where):
    """got [m, C] after ten iterations from `seeds` on `field` against float64, as assert_rows of the stage's GPU file."""
    keys = []
    for a in (field, seeds):
        a = np.ascontiguousarray(a)
        keys.append((a.shape, hash(a.tobytes())))
        _KEPT[keys[-1]] = a
    ref, tol = climb_yardstick(metric, *keys)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(where, "kernel %.3e from float64, allowed %.3e" % (err, tol))
    assert np.isfinite(got).all() and err <= tol, (where, err, tol)


def ms_climb_case(entry, metrics):
    """uoc_ms_hill_climb / _ex: ten iterations against float64 under the tolerance of the stage's own file."""
    def inputs(metric, m):
        CS = ms_modules(metric)[0]
        fields = [CS.hc_field(MS_N, seed=1 + b) for b in range(B)]
        return fields, [CS.hc_seeds(X, m, b)[0] for b, X in enumerate(fields)]

    def run(device, shape, rec):
        m, metric = shape
        fields, seeds = inputs(metric, m)
        Z = up(device, np.stack(seeds))
        ws, n = ms_ws(rec, MS_N, m)
        _native.call(entry, device, up(device, np.stack(fields)), B, MS_N, Z, m, mod("ms_cosine_cases").KAPPA, 10,
                     *((metric,) if entry.endswith("_ex") else ()), ws, n)
        return dict(Z=host(Z)), None

    def check(shape, bits, raw):
        m, metric = shape
        fields, seeds = inputs(metric, m)
        assert np.isfinite(bits["Z"]).all()
        b = MS_M.index(m) % B                   # one field per shape against float64; both fields across the two m
        climb_check(metric, bits["Z"][b], fields[b], seeds[b], (entry, shape, b))
    return Case([(m, met) for m in MS_M for met in metrics], run, check, align=256)


@functools.lru_cache(maxsize=None)
def ms_assign_inputs(metric, m):
    """Exact fields, their seeds (rows of the field), the seeds' components: what the whole call hands its assignment."""
    R, eps = ms_modules(metric)[1], ms_modules(metric)[2]
    fields = ms_exact_fields(metric, False)
    Z = [X[R.select_seeds(X, m, f)[0]] for X, f in zip(fields, ms_firsts())]
    sl = [np.asarray(R.seed_components(z, eps)[0] if metric == COS else R.seed_components(z, eps)) for z in Z]
    return fields, Z, np.stack(sl).astype(np.int32), [len(np.unique(s)) for s in sl]


def ms_assign_case(entry, metrics):
    def run(device, shape, rec):
        m, metric = shape
        fields, Z, sl, nu = ms_assign_inputs(metric, m)
        labels, closest = (torch.full((B, MS_N), -7, dtype=torch.int32, device=device) for _ in range(2))
        ws, n = ms_ws(rec, MS_N, m)
        _native.call(entry, device, up(device, np.stack(fields)), B, MS_N, up(device, np.stack(Z)), up(device, sl),
                     up(device, np.asarray(nu, np.int32)), m, *((metric,) if entry.endswith("_ex") else ()), labels, closest, ws, n)
        return dict(labels=host(labels), closest=host(closest)), None

    def check(shape, bits, raw):
        m, metric = shape
        R = ms_modules(metric)[1]
        fields, Z, sl, nu = ms_assign_inputs(metric, m)
        for b in range(B):
            want = (R.assign if metric == COS else R.assign_exact)(fields[b], Z[b], sl[b], nu[b])
            assert np.array_equal(bits["closest"][b], want[1]) and np.array_equal(bits["labels"][b], want[0]), (entry, shape, b)
    return Case([(m, met) for m in MS_M for met in metrics], run, check, align=256)


def ms_cluster_case(entry, metrics, halves):
    """The whole calls.  iters = 0 on exact fields: sampling, components, assignment and swap are all exact and every integer
    is compared.  iters = 10 on the climbing fields runs the hill-climbing region of the carve as well: the returned seeds
    against float64 from the returned indices, as the stage's 128-d test does."""
    wide = halves == 2

    def fields_of(metric, iters):
        if iters == 0:
            return ms_exact_fields(metric, wide)
        CS = ms_modules(metric)[0]
        return [CS.hc_field(MS_N, seed=7 + b, channels=64 * halves) for b in range(B)]

    def eps_of(metric, iters):
        return ms_modules(metric)[2] if iters == 0 or not wide or metric == COS else mod("ms_euclidean_cases").WIDE_EPS

    def run(device, shape, rec):
        m, metric, iters = shape

        def one(kernel):
            fields = fields_of(metric, iters)
            X = up(device, ms_planes(fields, wide))
            labels = torch.full((B, MS_N), -7, dtype=torch.int32, device=device)
            idx = torch.full((B, m), -7, dtype=torch.int32, device=device)
            Z = torch.full((B,) + ((2,) if wide else ()) + (m, 64), 9.0, device=device)
            sl = torch.full((B, m), -7, dtype=torch.int32, device=device)
            ws, n = ms_ws(rec, MS_N, m, halves)
            first = torch.tensor(ms_firsts(), dtype=torch.int32, device=device)
            args = (X,) + ((halves,) if "wide" in entry else ()) + (B, MS_N, m, mod("ms_cosine_cases").KAPPA, iters, float(eps_of(metric, iters)))
            args += ((metric,) if entry.endswith("_ex") else ()) + (first, labels, idx, Z, sl, ws, n)
            _native.call(entry, device, *args)
            _native.call("uoc_ms_check", device)
            return dict(labels=host(labels), idx=host(idx), Z=host(Z), sl=host(sl))
        return ms_both_kernels(one), None

    def check(shape, bits, raw):
        m, metric, iters = shape
        R, G = ms_modules(metric)[1], mod("ms_cosine_reference")
        fields = fields_of(metric, iters)
        for kernel in ("on-chip", "streaming"):
            got = {k: bits[kernel + "/" + k] for k in ("labels", "idx", "Z", "sl")}
            if iters == 0:
                for b, X in enumerate(fields):
                    if metric == COS:
                        wl, wi, _, wsl = R.cluster(X, mod("ms_cosine_cases").KAPPA, m, 0, eps_of(metric, iters), ms_firsts()[b])
                    else:
                        wl, wi, _, wsl = R.cluster_exact(X, m, eps_of(metric, iters), ms_firsts()[b])
                    where = (entry, shape, kernel, b)
                    assert np.array_equal(got["idx"][b], wi), where
                    assert np.array_equal(got["Z"][b], G.planes(X[wi]) if wide else X[wi]), where
                    assert np.array_equal(got["sl"][b], wsl) and np.array_equal(got["labels"][b], wl), where
            else:
                idx = got["idx"]
                assert (idx[:, 0] == ms_firsts()).all() and idx.min() >= 0 and idx.max() < MS_N
                Z = got["Z"][0].transpose(1, 0, 2).reshape(m, 128) if wide else got["Z"][0]
                climb_check(metric, Z, fields[0], fields[0][idx[0]], (entry, shape, kernel))
                assert np.isfinite(got["Z"]).all() and got["labels"].min() >= 0 and (got["sl"] >= 0).all()
    return Case([(m, met, 0) for m in MS_M for met in metrics] + [(MS_M[-1], met, 10) for met in metrics], run, check, align=256)


def confidence_inputs(m):
    T = mod("test_confidence_gpu")
    rng = np.random.default_rng(1000 * m + MS_N)
    X, Z = T.unit(rng, B, MS_N, 128), T.unit(rng, B, m, 128)
    planes = lambda a: np.ascontiguousarray(a.reshape(B, -1, 2, 64).transpose(0, 2, 1, 3))       # noqa: E731
    return planes(X), planes(Z), np.stack([T.seeded_labels(rng, m) for _ in range(B)])


def confidence_run(device, m, rec):
    from unseenobjectclustering_amd import confidence as CF
    X, Z, sl = confidence_inputs(m)
    with guard_workspaces(record=rec):
        res = CF.assign_confidence(up(device, X), up(device, Z), up(device, sl))
    assert rec.names() == ["uoc_ms_confidence_workspace_bytes"]
    return {k: host(getattr(res, k)) for k in mod("test_confidence_gpu").FIELDS}, None


def confidence_check(m, bits, raw):
    T = mod("test_confidence_gpu")
    X, Z, sl = confidence_inputs(m)
    for b in range(B):
        T.check_against_reference({k: v[b] for k, v in bits.items()}, X[b], Z[b], sl[b])


# ---- evaluation, glue, network: the raw entries with exactly the size function's value -----------------------------------------
class EvalTables(ctypes.Structure):
    _fields_ = [("cont", ctypes.c_int32 * (128 * 128)), ("prec_tp", ctypes.c_int32 * (128 * 128)), ("rec_tp", ctypes.c_int32 * (128 * 128)),
                ("bnd_pred", ctypes.c_int32 * 128), ("bnd_gt", ctypes.c_int32 * 128), ("bad_label", ctypes.c_int32)]


def eval_inputs(shape):
    H, W, bad = shape
    rng = np.random.default_rng(3)
    gt = rng.integers(0, 5, size=(H, W)).astype(np.int32)
    pred = np.roll(gt, 1, axis=1)
    if bad:                                     # ids outside [0, 128): the pixels are skipped and bad_label is raised
        pred[5, 7], pred[H - 1, W - 1], gt[11, 3] = 1000, -3, 128
    return pred, gt


def eval_run(device, shape, rec):
    from unseenobjectclustering_amd.utils import evaluation as EV
    H, W, _ = shape
    pred, gt = eval_inputs(shape)
    tables = torch.full((ctypes.sizeof(EvalTables),), 0x77, dtype=torch.uint8, device=device)
    ws, n = exact(rec, "uoc_eval_workspace_bytes", H, W)
    _native.call("uoc_eval_pair_stats", device, up(device, pred), up(device, gt), H, W, int(EV.bound_pixels((H, W))), tables, ws, n)
    t = EvalTables.from_buffer_copy(host(tables).tobytes())
    return {k: np.ctypeslib.as_array(getattr(t, k)).copy() for k in ("cont", "prec_tp", "rec_tp", "bnd_pred", "bnd_gt")} | \
        {"bad_label": np.array([t.bad_label], np.int32)}, None


def eval_check(shape, bits, raw):
    from unseenobjectclustering_amd.utils import evaluation as EV
    H, W, bad = shape
    if bad:                                     # no reference takes such maps: the flag, and (in the test) the same bits under every fill
        assert bits["bad_label"][0] != 0
        return
    pred, gt = eval_inputs(shape)
    want = mod("evaluation_reference").pair_tables(pred, gt, int(EV.bound_pixels((H, W))))
    assert bits["bad_label"][0] == 0
    for k in ("cont", "prec_tp", "rec_tp", "bnd_pred", "bnd_gt"):
        assert np.array_equal(bits[k].reshape(want[k].shape), want[k]), k


def roi_ws(rec):
    return exact(rec, "uoc_roi_workspace_bytes")


def z_plane(depth_d, H, W):
    return ctypes.c_void_p(depth_d.data_ptr() + 2 * H * W * 4)


def filter_run(device, thr, rec):
    labels, depth, _ = mod("glue_cases").filter_batch()        # three items: the statistics are reset per item
    Bf, H, W = labels.shape
    depth_d, lab = depth.to(device).contiguous(), labels.to(torch.int32).to(device).contiguous()
    ws, n = roi_ws(rec)
    _native.call("uoc_filter_labels_depth", device, lab, z_plane(depth_d, H, W), 3 * H * W, Bf, H, W, float(thr), ws, n)
    return dict(labels=host(lab)), None


def filter_want(thr):
    G = importlib.import_module("oracle.glue_oracle")
    raw, depth, clean, invalid = mod("glue_cases").filter_raw_abi()
    filtered = G.filter_labels_depth(clean.float(), depth, thr)
    want = filtered.to(torch.int32)
    want[invalid] = raw[invalid]
    return want, filtered


def filter_check(thr, bits, raw):
    G = importlib.import_module("oracle.glue_oracle")
    labels, depth, _ = mod("glue_cases").filter_batch()
    want = G.filter_labels_depth(labels, depth, thr)
    assert labels.shape[0] >= 2 and bool((want != labels).any())
    assert np.array_equal(bits["labels"], want.to(torch.int32).numpy())


def roi_build_run(device, thr, rec):
    from unseenobjectclustering_amd.fcn import test_dataset as TD
    raw, depth, _, _ = mod("glue_cases").filter_raw_abi()
    _, H, W = raw.shape
    depth_d, lab = depth.to(device).contiguous(), raw[0].to(device).contiguous()
    table = torch.full((_native.ROI_TABLE_BYTES,), 0x77, dtype=torch.uint8, device=device)
    ws, n = roi_ws(rec)
    _native.call("uoc_roi_build", device, lab, z_plane(depth_d, H, W), H, W, float(thr), TD.PAD_FRACTION, table, ws, n)
    return dict(labels=host(lab), table=host(table)), None


def roi_build_check(thr, bits, raw):
    G = importlib.import_module("oracle.glue_oracle")
    want, filtered = filter_want(thr)
    ids, boxes = G.roi_boxes(filtered[0])
    t = _native.RoiTable.from_buffer_copy(bits["table"].tobytes())
    assert np.array_equal(bits["labels"], want[0].numpy())
    assert t.K == len(ids) and list(t.label[:t.K]) == ids and [list(t.box[k]) for k in range(t.K)] == boxes.tolist()


def match_stats_run(device, K, rec):
    labels, mask, depth = mod("glue_cases").stats_case(K)
    S = labels.shape[-1]
    keep = torch.full((K, 128), -7, dtype=torch.int32, device=device)
    meanz = torch.full((K,), 123.0, device=device)
    ws, n = roi_ws(rec)
    _native.call("uoc_roi_match_stats", device, labels.to(torch.int32).reshape(K, -1).to(device), mask.to(device).contiguous(),
                 depth.to(device).contiguous(), K, S, keep, meanz, ws, n)
    return dict(keep=host(keep), meanz=host(meanz)), None


def match_stats_check(K, bits, raw):
    C = mod("glue_cases")
    want_keep, want_meanz, _ = C.oracle_keep_meanz(*C.stats_case(K))
    assert np.array_equal(bits["keep"], want_keep.numpy())
    nan = torch.isnan(want_meanz).numpy()
    assert np.array_equal(np.isnan(bits["meanz"]), nan)
    assert np.array_equal(bits["meanz"][~nan].view(np.int32), want_meanz.numpy()[~nan].view(np.int32)), "bit-equal means"


def match_run(device, shape, rec):
    C = mod("glue_cases")
    c, raw, _ = C.match_raw_abi()
    K, S = raw.shape[0], raw.shape[-1]
    _, H, W = c["initial_masks"].shape
    table = torch.frombuffer(bytearray(bytes(C.roi_table(c["rois"].long().tolist(), [0] * K))), dtype=torch.uint8).to(device)
    refined = torch.full((H * W,), -77, dtype=torch.int32, device=device)
    keep = torch.full((K, 128), -77, dtype=torch.int32, device=device)
    plan = torch.full((K + K * 128,), -77, dtype=torch.int32, device=device)
    status = torch.zeros((1,), dtype=torch.int32, device=device)
    ws, n = roi_ws(rec)
    _native.call("uoc_roi_match", device, raw.to(torch.int32).reshape(K, -1).to(device), c["mask"].to(device).contiguous(),
                 c["depth"].to(device).contiguous(), table, K, S, H, W, refined, keep, plan, status, ws, n)
    return dict(refined=host(refined), keep=host(keep), plan=host(plan), status=host(status)), None


def match_check(shape, bits, raw):
    G, C = importlib.import_module("oracle.glue_oracle"), mod("glue_cases")
    c, _, clean = C.match_raw_abi()
    _, H, W = c["initial_masks"].shape
    want, _ = G.match_label_crop(c["initial_masks"], clean, c["mask"], c["rois"], c["depth"])
    want_keep, _, _ = C.oracle_keep_meanz(clean, c["mask"], c["depth"])
    assert bits["status"][0] == 0
    assert np.array_equal(bits["keep"], want_keep.numpy())
    assert np.array_equal(bits["refined"].reshape(H, W), want[0].to(torch.int32).numpy())


NET = dict(wseed=5, H=64, W=96)


@functools.lru_cache(maxsize=None)
def net_frames():
    from unseenobjectclustering_amd import synth
    frames = [synth.rgbd_frame(12 + k, NET["H"], NET["W"], 3) for k in range(B)]
    return np.concatenate([f["image_color"] for f in frames]), np.concatenate([f["depth"] for f in frames])


_nets = {}


def net_run(device, shape, rec):
    key = str(device)
    if key not in _nets:                        # one network per process: building it uploads every weight
        _nets[key] = mod("test_backbone_gpu")._net(NET["wseed"], device)
    net, _ = _nets[key]
    dev = torch.device(device)
    net._ensure_native(dev)
    img, dep = (up(dev, a) for a in net_frames())
    H, W = NET["H"], NET["W"]
    embed = torch.full((B, H * W, 64), 9.0, device=dev)
    n = int(_native.lib().uoc_net_workspace_bytes(net._handle, B, H, W))
    ws = rec.take("uoc_net_workspace_bytes", n)
    _native.call("uoc_net_forward", dev, net._handle, img, dep, B, H, W, embed, ws, n)
    return dict(embed=host(embed)), None


def net_check(shape, bits, raw):
    from unseenobjectclustering_amd import synth
    BO, T = importlib.import_module("oracle.backbone_oracle"), mod("test_backbone_gpu")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(NET["wseed"]).items()}
    img, dep = (torch.from_numpy(a) for a in net_frames())
    want = BO.segnet_forward(sd, img, dep)
    got = torch.from_numpy(bits["embed"]).view(B, NET["H"], NET["W"], 64).permute(0, 3, 1, 2)
    assert (got - want).abs().max().item() < T.EMBED_TOL
    assert np.abs(np.linalg.norm(bits["embed"], axis=2) - 1).max() < 1e-5


# ---- (d) the three persistent stages: what the state test drives ----------------------------------------------------------------
class TrackState:
    """uoc_track_reset / uoc_track_step through the C ABI: B streams of 37 x 53, three frames each."""
    reset_entry, state_size = "uoc_track_reset", "uoc_track_state_bytes"
    shape = LABEL_SHAPES[0]
    outputs = ("out", "lut", "tracks")
    optional = ("lut", "tracks")                # the wrapper allocates these with torch.zeros; the header says every word is written

    def __init__(self):
        self.frames = track_frames(self.shape)
        self.q = 19661                          # round(0.3 * 65536)

    def size_args(self):
        return (B,) + tuple(self.shape)

    def stream_bytes(self):
        return int(_native.lib().uoc_track_state_bytes(*self.size_args())) // B

    def reset(self, device, state, which):
        _native.call("uoc_track_reset", device, state, B, *self.shape, which)

    def step(self, device, state, inputs, rec, out_fill):
        H, W = self.shape
        lab = up(device, np.stack(inputs))
        out = torch.empty_like(lab)
        lut = torch.full((B, 128), out_fill, dtype=torch.int32, device=device)
        tracks = torch.full((B, 128, 5), out_fill, dtype=torch.int32, device=device)
        ws, n = exact(rec, "uoc_track_workspace_bytes", B)
        _native.call("uoc_track_step", device, lab, B, H, W, self.q, TRACK["max_age"], state, out, lut, tracks, ws, n)
        return dict(out=host(out), lut=host(lut), tracks=host(tracks))


class IdentState:
    """uoc_ident_reset / uoc_ident_step: stream b steps the tables of IDENT_CASES[b]."""
    reset_entry, state_size = "uoc_ident_reset", "uoc_ident_state_bytes"
    outputs = ("out", "lut", "ident")
    optional = ("lut", "ident")

    def __init__(self):
        cases, self.ids = ident_inputs()
        self.case = cases[0][0]
        self.frames = [[c.steps[t] for t in range(3)] for c, _ in cases]

    def size_args(self):
        return (B,)

    def stream_bytes(self):
        return int(_native.lib().uoc_ident_state_bytes(B)) // B

    def reset(self, device, state, which):
        _native.call("uoc_ident_reset", device, state, B, which)

    def step(self, device, state, inputs, rec, out_fill):
        H, W = self.ids.shape
        tracked = up(device, np.stack([self.ids] * B))
        tracks, sig = (up(device, np.stack([i[k] for i in inputs])) for k in range(2))
        out = torch.empty_like(tracked)
        lut = torch.full((B, 128), out_fill, dtype=torch.int32, device=device)
        ident = torch.full((B, 128, 5), out_fill, dtype=torch.int32, device=device)
        ws, n = exact(rec, "uoc_ident_workspace_bytes", B)
        _native.call("uoc_ident_step", device, tracked, tracks, sig, B, H, W, self.case.q, self.case.r, self.case.max_lost, state, out, lut,
                     ident, ws, n)
        return dict(out=host(out), lut=host(lut), ident=host(ident))


class SceneState:
    """uoc_scene_reset / uoc_scene_step: two streams of G = 8 on the hand sequence of tests/test_scene_gpu.py's reset test."""
    reset_entry, state_size = "uoc_scene_reset", "uoc_scene_state_bytes"
    G = 8
    optional = ()

    def __init__(self):
        R = mod("scene_reference")
        seq = R.hand_sequences()["blank_then_forgotten"][0]
        self.frames = [list(seq[:3]), list(seq[1:4])]
        self.outputs = mod("test_scene_gpu").KEYS

    def size_args(self):
        return (B, self.G)

    def stream_bytes(self):
        return int(_native.lib().uoc_scene_state_bytes(B, self.G)) // B

    def reset(self, device, state, which):
        _native.call("uoc_scene_reset", device, state, B, self.G, which)

    def step(self, device, state, inputs, rec, out_fill):
        from unseenobjectclustering_amd import scene
        T = mod("test_scene_gpu")
        s, o, frame, drop = T.stack_frames(inputs, B)
        with guard_workspaces(record=rec):
            out = scene.scene_records(up(device, s), up(device, o), up(device, frame), up(device, drop), state.view(torch.int32).view(B, -1),
                                      5, 1, T.QUERIES8)
        return {k: host(v) for k, v in zip(T.KEYS, out)}


STATE_STAGES = {"uoc_track_reset": TrackState, "uoc_ident_reset": IdentState, "uoc_scene_reset": SceneState}


def state_case(name):
    return Case([None], None, None, kind="state")


# ---- the table --------------------------------------------------------------------------------------------------------------
BOTH = (COS, EUC)
CASES = {
    "uoc_ms_select_seeds": ms_select_case("uoc_ms_select_seeds", (COS,), 0),
    "uoc_ms_select_seeds_from": ms_select_case("uoc_ms_select_seeds_from", (COS,), 3),
    "uoc_ms_select_seeds_ex": ms_select_case("uoc_ms_select_seeds_ex", BOTH, 0),
    "uoc_ms_hill_climb": ms_climb_case("uoc_ms_hill_climb", (COS,)),
    "uoc_ms_hill_climb_ex": ms_climb_case("uoc_ms_hill_climb_ex", BOTH),
    "uoc_ms_assign": ms_assign_case("uoc_ms_assign", (COS,)),
    "uoc_ms_assign_ex": ms_assign_case("uoc_ms_assign_ex", BOTH),
    "uoc_ms_cluster": ms_cluster_case("uoc_ms_cluster", (COS,), 1),
    "uoc_ms_cluster_ex": ms_cluster_case("uoc_ms_cluster_ex", BOTH, 1),
    "uoc_ms_cluster_wide": ms_cluster_case("uoc_ms_cluster_wide", (COS,), 2),
    "uoc_ms_cluster_wide_ex": ms_cluster_case("uoc_ms_cluster_wide_ex", BOTH, 2),
    "uoc_ms_confidence": Case(list(MS_M), confidence_run, confidence_check),
    "uoc_net_forward": Case([(B, NET["H"], NET["W"])], net_run, net_check, align=256),
    "uoc_filter_labels_depth": Case([0.8], filter_run, filter_check),
    "uoc_roi_build": Case([0.8], roi_build_run, roi_build_check),
    "uoc_roi_match_stats": Case([2], match_stats_run, match_stats_check),
    "uoc_roi_match": Case([None], match_run, match_check),
    "uoc_eval_pair_stats": Case([(37, 53, False), (37, 53, True)], eval_run, eval_check, align=256),
    "uoc_objects": Case(LABEL_SHAPES, objects_run, objects_check),
    "uoc_track_reset": state_case("uoc_track_reset"),
    "uoc_track_step": Case(LABEL_SHAPES, track_run, track_check),
    "uoc_cc_split": Case(LABEL_SHAPES, cc_run, cc_check),
    "uoc_support_plane": Case(LABEL_SHAPES, plane_run, plane_check),
    "uoc_support_planes": Case(LABEL_SHAPES, planes_run, planes_check),
    "uoc_relations": Case(LABEL_SHAPES, relations_run, relations_check),
    "uoc_placement": Case(GRID_LABEL_SHAPES, placement_run, placement_check),
    "uoc_grasp": Case(GRIDS, grasp_run, grasp_check),
    "uoc_elevation": Case(GRID_LABEL_SHAPES, elevation_run, elevation_check),
    "uoc_footprint": Case(GRIDS, footprint_run, footprint_check),
    "uoc_routes": Case(GRIDS, routes_run, routes_check),
    "uoc_normals": Case(LABEL_SHAPES, normals_run, normals_check),
    "uoc_signature": Case(LABEL_SHAPES, signature_run, signature_check, kind="signature"),
    "uoc_ident_reset": state_case("uoc_ident_reset"),
    "uoc_ident_step": Case([(2, 66)], ident_run, ident_check),
    "uoc_motion": Case(GRIDS, motion_run, motion_check),
    "uoc_scene_reset": state_case("uoc_scene_reset"),
    "uoc_scene_step": Case(GRIDS, scene_run, scene_check),
}
