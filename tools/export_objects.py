#!/usr/bin/env python
"""Per-object point clouds and 3D boxes for a directory of RGB-D frames: the two-stage segmentation of
tools/test_images.py, then extract_objects on the device (unseenobjectclustering_amd/objects.py).

    python tools/export_objects.py --imgdir tests/golden/demo --out objs/ [--max-points 2048]
                                   [--pretrained ckpt.pth --pretrained_crop crop.pth] [--cfg experiments/cfgs/<experiment>.yml]
                                   [--track [--track-min-iou 0.3] [--track-max-age 5]]
                                   [--reid [--reid-min-sim 0.7] [--reid-min-size 0.25] [--reid-max-lost 300]]
                                   [--motion [--motion-angles 32] [--motion-radius 8]]
                                   [--components {all,largest} [--min-area 1]]
                                   [--plane [--min-height M]]
                                   [--relations [--relations-gap 0.015] [--relations-min-pairs 8]]
                                   [--placement RADIUS_M [--grid 256] [--cell-mm 10] [--memory AGE]]
                                   [--grasp MAX_OPEN_M [--grasp-angles 16] [--grasp-offsets 2]]
                                   [--elevation STEP_M [--elevation-min-pts 2]]
                                   [--putdown LENGTH_M WIDTH_M [--putdown-angles 16]]
                                   [--confidence [WEAK]]
                                   [--normals]
                                   [--planes K [--planes-up X Y Z]]

Writes <frame>_objects.npz per frame: the label map the objects come from (`label_map`), one row per object (`frame`,
`label`, `pixels`, `count`, `box`, `centroid`, `cov`, `aabb_min`, `aabb_max`, `eigenvalues`, `axes`, `obb_center`,
`obb_half`) and the packed clouds (`points`, `pixel_index`, `offsets`: object k is points[offsets[k]:offsets[k+1]]).
Without checkpoints the calibrated synthetic weights are used (test_images.load_weights).

With --track the frames are taken as one stream in file order: every final label map goes through the device-side tracker
(unseenobjectclustering_amd/tracking.py) and the objects are extracted from the TRACKED map, so `label` is the track slot
an object keeps from frame to frame, `label_map` the tracked map, `raw_label_map` the segmentation's own numbering and
`track_uid` the stream-wide object number of every row.

With --reid (it needs --track) the tracked map and the colour image also go through the device-side re-identification
(unseenobjectclustering_amd/identity.py): per row `identity`, the identity entry in 1..127 that the object keeps across a
jump with no mask overlap or an occlusion longer than --track-max-age, and `identity_pid`, that identity's stream-wide
number; `identity_map` is the label map renumbered by identity.  Every other key is as without the flag.

With --components the final label map is first split into its spatially connected pieces on the device
(unseenobjectclustering_amd/components.py): `largest` keeps the largest piece of every id and drops the rest (speckle),
`all` renumbers every piece of at least --min-area pixels 1..127 (look-alike objects that shared an id come apart).  The
order is segmentation, split, --track if given, extract_objects; `component_src`, `component_area` and
`component_siblings` give per row the raw id the piece came from, its pixels and the number of pieces that id had.

With --plane the support plane of the exported label map is fitted on the device (unseenobjectclustering_amd/support.py):
`plane_found`, `plane_candidates`, `plane_inliers`, `plane_hyp`, `plane_normal`, `plane_d`, `plane_centroid`, `plane_eig`,
`plane_rms`, `plane_u`, `plane_v` describe it, and per row `height_min`, `height_max`, `foot`, `cov2`, `upright_axis`,
`upright_half`, `upright_center` give the object's height above it and its upright box.  --min-height M adds `standing`
per row: whether the object's top is at least M metres above the plane.

With --relations the relations of the objects of the exported label map (the tracked or split one when --track or
--components is given: those are ordinary label maps) are computed on the device (unseenobjectclustering_amd/relations.py,
8-connected pixel pairs): per row `layer`, `free`, `order`, `n_above` and `edge`, and `front` / `touch`, the K x K
sub-matrices of the pair tables over the exported objects in row order (front[i][j]: pairs where row i is nearer than
row j by at least --relations-gap metres; touch[i][j]: pairs closer than that).  --relations-min-pairs pairs make a relation.

With --placement RADIUS_M the free space on the support plane of the exported label map (the tracked or split one
likewise) is computed on the device (unseenobjectclustering_amd/placement.py) on a grid of --grid x --grid cells of
--cell-mm millimetres: `place_state` (0 unknown, 1 table, 2 obstacle) and `place_dist2` (squared clearance in cells), the
--grid x --grid maps; `place_widest_cell` = (i, j, dist2, ok), the table cell with the most room and whether a disc of
RADIUS_M metres fits there ((-1, -1, 0, 0) without a table cell), and `place_widest_xyz`, that cell's centre in camera
coordinates (NaN without one).  The plane is fitted for it whether or not --plane is given.

With --grasp MAX_OPEN_M the parallel-jaw grasp candidates of the exported objects are computed on the device
(unseenobjectclustering_amd/grasp.py) on the --grid x --grid grid of the placement stage, which runs for it with its
defaults whether or not --placement is given, for a gripper that opens to MAX_OPEN_M metres: per row `grasp_best` =
(ok, k, m, tlo, w, ax, ay, n_ok) and `grasp_cand`, the (code, tlo) of every direction and lateral offset; and the pose
of the best candidate, `grasp_center` and `grasp_axis` (camera coordinates; NaN for a row without a candidate),
`grasp_width` and `grasp_opening` (metres; NaN likewise).  `grasp_dirs` is the direction table.

With --elevation STEP_M the elevation map of the frame is computed on the device (unseenobjectclustering_amd/elevation.py)
on the --grid x --grid grid of the placement stage, which runs for it with its defaults whether or not --placement is
given; cells that climb at most STEP_M metres from one to the next and hold --elevation-min-pts points near their top are
level.  Per row `top_cells` and `top_level`, the object's solid and level cells; `top_cell` = (i, j), the level cell with
the most room ((-1, -1) without one), `top_clear_m`, the distance from there to the nearest cell that is not level,
`top_height_m`, its height above the plane, and `top_xyz`, its centre lifted onto the top, camera coordinates (NaN
without a level cell).  With --placement RADIUS_M also `top_fits`: whether a disc of RADIUS_M metres fits there.

With --motion (it needs --track) every object's motion on the table since the frame before is registered on the device
(unseenobjectclustering_amd/motion.py) on the --grid x --grid grid: a rotation about the plane normal, one of
--motion-angles over a full turn, and an in-plane shift.  The support plane fitted on the FIRST frame serves the whole
stream (the camera must stand still), the ids are those of the exported label map (the identities under --reid).  Every
frame but the first gets `motion_ids` [P], `motion_best` [P,16] = (status, k, si, sj, cost, n_a, n_b, still, pi, pj, qi,
qj, ti, tj, second, 0) and `motion_T` [P,4,4], the rigid motion in camera coordinates (NaN where status is not 1).

With --memory AGE (it needs --placement) the table grid is fused over the frames on the device
(unseenobjectclustering_amd/scene.py): a cell that this frame does not observe keeps its last sighting for AGE steps, a
cell whose observation contradicts the memory is flagged.  The support plane of the FIRST frame serves the whole stream
(the camera must stand still).  Every frame gets `memory_state`, `memory_owner`, `memory_age` (steps since the cell was
seen, -1: unknown), `memory_change` (0 same, 1 appeared, 2 vanished, 3 reowned) [G,G], `memory_ids` [128,8] =
(cells_now, cells_kept, oldest, appeared, vanished, reowned_in, reowned_out, forgotten) per owner id and `memory_info` [8]
= (status, steps, observed, kept, forgotten, appeared, vanished, reowned).  With --motion the remembered cells of the ids
that moved (motion.moved) are dropped, and the ids are those --motion follows.

With --putdown LENGTH_M WIDTH_M the oriented put-down poses of a LENGTH_M x WIDTH_M rectangle (conservative: inflated by
0.72 cell) are computed on the device (unseenobjectclustering_amd/footprint.py) on the --grid x --grid grid of the
placement stage, which runs for it with its defaults whether or not --placement is given, over --putdown-angles
orientations of half a turn: `putdown_fits` [G,G] int32, bit k set where the rectangle fits along direction k;
`putdown_count` [32], the cells per direction; `putdown_best` = (ok, i, j, k, dist2, da, poses, cells), the roomiest
pose; `putdown_center` and `putdown_axis`, that cell's centre and the rectangle's long axis in camera coordinates (NaN
without a pose).  `putdown_dirs` is the direction table.

With --route ID RADIUS_M (which needs --placement) the way of object ID, as a disc of RADIUS_M metres that its own cells do
not block, from the cell of its centre to the widest spot --placement found is computed on the device
(unseenobjectclustering_amd/routes.py): `route_cost` [G,G] int32, the least cost of sliding there from the source (5 per
orthogonal, 7 per diagonal move, -1: not reachable); `route_info` = (src_ok, ok, ci, cj, cost, steps, reached, passable);
`route_path` [n,2] int32, the cells from the source to the goal (empty without a path); `route_xyz` [n,3], their centres
in camera coordinates, and `route_length_m` (NaN without a path).

With --confidence [WEAK] the frame goes through the segmentation with the assignment margins alongside
(unseenobjectclustering_amd/confidence.py; the label maps are the same): `conf_map` [H,W] float32, per pixel how far the
nearest seed of another cluster lay behind the one that gave the pixel its label (0: a coin toss; 0 also where the two
stages disagree), and per row, over the pixels of the exported label map (the tracked or split one likewise),
`conf_mean`, `conf_min` (float64, in steps of 1/65536) and `conf_weak_share`, the share of the object's pixels whose margin
is below WEAK (default 0.02).  Cosine metric only: under the euclidean opt-in the tool stops with NotImplementedError.

With --normals the surface normals of the frame are computed on the device (unseenobjectclustering_amd/normals.py) from the
XYZ planes, the exported label map (the tracked or split one likewise) and its support plane, which is fitted for it
whether or not --plane is given: `normal` [H,W,3] int32, the integer normal per pixel (zero without one), `normal_info`
[H,W] int32 = class | grazing << 3 | azimuth bin << 8 | nX << 16 | nY << 24 (class 1 up, 2 side, 3 oblique, 4 down), and
per row `faces` [40] int32 = (pixels, with_normal, up, side, oblique, down, grazing, peak) and the histogram of the
object's side pixels over 16 azimuth bins of a full turn in the plane's axes (`plane_u`, `plane_v` of --plane).

With --planes K up to K (1..8) planes of the exported label map's background are extracted on the device
(unseenobjectclustering_amd/support.py, fit_planes): shelves, walls and the plane the objects stand on.  `plane_count`,
and per plane slot `plane_normal` [K,3], `plane_d`, `plane_inliers`, `plane_cos0` (cosine with plane 0), `plane_offset0`
(distance of its centroid from plane 0) and `plane_extent` [K,4] (min / max of its inliers along its axes); `plane_index`
[H,W] int32, the map (-2 not background, k an inlier of plane k, 16 + k its fringe, -1 left over); per row `stands_on`, the
plane the object stands on (-1: none), and `plane_support`, the plane most objects stand on.  That plane, not the
dominant one, is then the support plane of --placement, --grasp, --elevation, --putdown and --normals.  --planes-up X Y Z
gives the direction away from the floor in camera coordinates; without it plane 0 decides which planes are horizontal,
which is wrong in a view that a wall dominates.  Not together with --plane, whose `plane_*` arrays describe one plane.
"""
import argparse
import glob
import json
import os
import sys
from functools import cached_property
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from test_images import load_weights  # noqa: E402
from unseenobjectclustering_amd import footprint, identity, io as uio, motion, networks, normals, routes, scene, synth  # noqa: E402
from unseenobjectclustering_amd.fcn.config import cfg, cfg_from_file, network_mode  # noqa: E402
from unseenobjectclustering_amd.components import split_components  # noqa: E402
from unseenobjectclustering_amd.confidence import summarize  # noqa: E402
from unseenobjectclustering_amd.elevation import heights, spot  # noqa: E402
from unseenobjectclustering_amd.grasp import candidates, pose  # noqa: E402
from unseenobjectclustering_amd.objects import extract_objects, segment_objects  # noqa: E402
from unseenobjectclustering_amd.placement import WIDEST, cell_to_camera, free_space, need2  # noqa: E402
from unseenobjectclustering_amd.relations import relate  # noqa: E402
from unseenobjectclustering_amd.support import choose_support, fit_plane, fit_planes, standing_objects, standing_on  # noqa: E402
from unseenobjectclustering_amd.tracking import Tracker  # noqa: E402

FIELDS = ("frame", "label", "pixels", "count", "box", "centroid", "cov", "aabb_min", "aabb_max", "eigenvalues", "axes",
          "obb_center", "obb_half", "offsets", "points", "pixel_index")
PLANE_KEYS = ("found", "candidates", "inliers", "hyp", "normal", "d", "centroid", "eig", "rms", "u", "v")
OBJECT_KEYS = {"height_min": "height_min", "height_max": "height_max", "foot": "foot", "cov2": "cov2", "axis": "upright_axis",
               "half": "upright_half", "center": "upright_center"}


def plane_arrays(fitted, ids, min_height=None):
    """The --plane arrays of one frame: the plane of frame 0 of `fitted` and, per exported object (ids = its labels), the
    height and upright-box fields."""
    rec = {"plane_" + k: getattr(fitted, k)[0].cpu().numpy() for k in PLANE_KEYS}
    rec.update({name: getattr(fitted, k)[0][ids].cpu().numpy() for k, name in OBJECT_KEYS.items()})
    if min_height is not None:
        rec["standing"] = standing_objects(fitted, min_height)[0][ids].cpu().numpy()
    return rec


PLANES_KEYS = {"count": "plane_count", "normal": "plane_normal", "d": "plane_d", "inliers": "plane_inliers", "cos0": "plane_cos0",
               "offset0": "plane_offset0", "extent": "plane_extent", "index": "plane_index"}


def planes_arrays(several, ids, up=None):
    """The --planes arrays of one frame: frame 0 of `several` (a support.fit_planes result), per exported object (ids =
    its labels) the plane it stands on, and the plane most of them stand on."""
    rec = {name: getattr(several, k)[0].cpu().numpy() for k, name in PLANES_KEYS.items()}
    rec["stands_on"] = standing_on(several, 0 if up is None else tuple(up))[0][ids].cpu().numpy()
    rec["plane_support"] = choose_support(several, up=None if up is None else tuple(up))[0].cpu().numpy()
    return rec


GRASP_KEYS = ("grasp_best", "grasp_cand", "grasp_dirs", "grasp_center", "grasp_axis", "grasp_width", "grasp_opening")


def grasp_arrays(grasped, ids):
    """The --grasp arrays of one frame: per exported object (ids = its labels) the best record, the candidate table and
    the pose of the best candidate of frame 0 of `grasped`."""
    ids = [int(a) for a in ids]
    rec = {"grasp_best": grasped.best[0][ids].cpu().numpy(), "grasp_cand": grasped.cand[0][ids].cpu().numpy(),
           "grasp_dirs": np.asarray(grasped.dirs, np.int32)}
    poses = [pose(grasped, 0, a) for a in ids]
    nan3 = np.full(3, np.nan)
    rec["grasp_center"] = np.array([p.center if p else nan3 for p in poses], np.float64).reshape(len(ids), 3)
    rec["grasp_axis"] = np.array([p.axis if p else nan3 for p in poses], np.float64).reshape(len(ids), 3)
    rec["grasp_width"] = np.array([p.width_m if p else np.nan for p in poses], np.float64)
    rec["grasp_opening"] = np.array([p.opening_m if p else np.nan for p in poses], np.float64)
    return rec


ELEVATION_KEYS = ("top_cells", "top_level", "top_cell", "top_clear_m", "top_height_m", "top_xyz")


def elevation_arrays(raised, ids, radius=None):
    """The --elevation arrays of one frame: per exported object (ids = its labels) the row of tops of frame 0 of `raised`
    and its widest level spot; with a radius (metres) also whether a disc of that radius fits there."""
    ids = [int(a) for a in ids]
    tops = raised.tops[0][ids].cpu().numpy().reshape(len(ids), 8)
    spots = [spot(raised, 0, a) for a in ids]
    rec = {"top_cells": tops[:, 0].copy(), "top_level": tops[:, 1].copy(), "top_cell": tops[:, 2:4].copy(),
           "top_clear_m": np.array([s.clearance_m if s else np.nan for s in spots], np.float64),
           "top_height_m": np.array([s.height_m if s else np.nan for s in spots], np.float64),
           "top_xyz": np.array([s.xyz if s else np.full(3, np.nan) for s in spots], np.float64).reshape(len(ids), 3)}
    if radius is not None:
        rec["top_fits"] = (tops[:, 1] > 0) & (tops[:, 4] >= need2(radius, raised.cell_mm / 1000.0))
    return rec


PUTDOWN_KEYS = ("putdown_fits", "putdown_count", "putdown_best", "putdown_dirs", "putdown_center", "putdown_axis")


def putdown_arrays(fitting):
    """The --putdown arrays of one frame: rectangle 0 of frame 0 of `fitting` (a footprint.fit result) and its best pose."""
    p = footprint.pose(fitting, 0, 0)
    nan3 = np.full(3, np.nan)
    return {"putdown_fits": fitting.fits[0, 0].cpu().numpy(), "putdown_count": fitting.count[0, 0].cpu().numpy(),
            "putdown_best": fitting.best[0, 0].cpu().numpy(), "putdown_dirs": np.asarray(fitting.dirs, np.int32),
            "putdown_center": np.asarray(p.center if p else nan3, np.float64), "putdown_axis": np.asarray(p.axis if p else nan3, np.float64)}


ROUTE_KEYS = ("route_cost", "route_info", "route_path", "route_xyz", "route_length_m")


def route_arrays(routed):
    """The --route arrays of one frame: query 0 of frame 0 of `routed` (a routes.plan result)."""
    w = routes.waypoints(routed, 0, 0)
    length = routes.length_m(routed, 0, 0)
    return {"route_cost": routed.cost[0, 0].cpu().numpy(), "route_info": routed.info[0, 0].cpu().numpy(),
            "route_path": w.cells.astype(np.int32) if w else np.zeros((0, 2), np.int32),
            "route_xyz": routes.path_to_camera(routed, 0, 0) if w else np.zeros((0, 3), np.float64),
            "route_length_m": np.float64(np.nan if length is None else length)}


CONFIDENCE_KEYS = ("conf_map", "conf_mean", "conf_min", "conf_weak_share")


def confidence_arrays(summary, ids, margin):
    """The --confidence arrays of one frame: the margin map and, per exported object (ids = its labels), the rows of frame
    0 of `summary` (a confidence.summarize result over the exported label map)."""
    ids = [int(a) for a in ids]
    return {"conf_map": margin.cpu().numpy().astype(np.float32), "conf_mean": np.asarray(summary.mean[0][ids], np.float64),
            "conf_min": np.asarray(summary.min[0][ids], np.float64), "conf_weak_share": np.asarray(summary.weak_share[0][ids], np.float64)}


NORMALS_KEYS = ("normal", "normal_info", "faces")


def normals_arrays(estimated, ids):
    """The --normals arrays of one frame: the normals and the info words of frame 0 of `estimated` (a normals.estimate
    result) and, per exported object (ids = its labels), its row of faces."""
    ids = [int(a) for a in ids]
    return {"normal": estimated.n[0].cpu().numpy(), "normal_info": estimated.info[0].cpu().numpy(),
            "faces": estimated.faces[0][ids].cpu().numpy().reshape(len(ids), normals.FACE_WORDS)}


RELATION_KEYS = ("layer", "free", "order", "n_above", "edge")


def relation_arrays(related, ids):
    """The --relations arrays of one frame: per exported object (ids = its labels) the record fields of RELATION_KEYS,
    and the front / touch tables of frame 0 of `related` restricted to those objects."""
    rec = {k: getattr(related, k)[0][ids].cpu().numpy() for k in RELATION_KEYS}
    rec.update({k: getattr(related, k)[0][ids][:, ids].cpu().numpy() for k in ("front", "touch")})
    return rec


MOTION_KEYS = ("motion_ids", "motion_best", "motion_T")


def motion_arrays(res):
    """The --motion arrays of one frame against the frame before: frame 0 of `res` (a motion.register result, None when no
    id is on both grids).  motion_ids [P], the ids followed; motion_best [P,16], motion.BEST_FIELDS per id; motion_T
    [P,4,4], the rigid motion in camera coordinates (NaN for an id that was not evaluated)."""
    if res is None:
        return {"motion_ids": np.zeros((0,), np.int32), "motion_best": np.zeros((0, 16), np.int32), "motion_T": np.zeros((0, 4, 4), np.float64)}
    moves = [motion.transform(res, 0, p) for p in range(len(res.pairs))]
    return {"motion_ids": np.asarray(res.pairs[:, 0], np.int32), "motion_best": res.best[0].cpu().numpy(),
            "motion_T": np.stack([np.full((4, 4), np.nan) if m is None else m.T for m in moves])}


MEMORY_KEYS = ("memory_state", "memory_owner", "memory_age", "memory_change", "memory_ids", "memory_info")


def memory_arrays(res):
    """The --memory arrays of one frame: frame 0 of `res` (a scene.Memory.update result).  memory_state, memory_owner,
    memory_age, memory_change [G,G]: the fused grid, how many steps ago each cell was seen (-1: unknown) and its change
    code (scene.CODES); memory_ids [128,8], scene.ID_FIELDS per owner id; memory_info [8], scene.INFO_FIELDS."""
    return {"memory_" + k: getattr(res, k)[0].cpu().numpy() for k in ("state", "owner", "age", "change", "ids", "info")}


def moved_ids_mask(res, device):
    """[1,128] bool on the device: the ids motion.moved reports for frame 0 of `res` (None: no id), built without a host
    read; what --memory drops."""
    mask = torch.zeros((1, 128), dtype=torch.bool, device=device)
    if res is not None:
        mask[0, torch.from_numpy(np.asarray(res.pairs[:, 0], np.int64)).to(device)] = motion.moved(res)[0]
    return mask


def placement_arrays(placed):
    """The --placement arrays of one frame: the grid maps of frame 0 of `placed` (a placement.free_space result whose
    query 0 is the widest spot for the disc) and that spot."""
    ans = placed.answers[0, 0].cpu().numpy()
    spot = cell_to_camera(placed, 0, ans[0], ans[1]) if ans[0] >= 0 else np.full(3, np.nan)
    return {"place_state": placed.state[0].cpu().numpy(), "place_dist2": placed.dist2[0].cpu().numpy(),
            "place_widest_cell": ans, "place_widest_xyz": spot.astype(np.float64)}


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--imgdir", required=True)
    ap.add_argument("--color", default="*-color.png")
    ap.add_argument("--depth", default="*-depth.png")
    ap.add_argument("--pretrained", default=None)
    ap.add_argument("--pretrained_crop", default=None)
    ap.add_argument("--cfg", dest="cfg_file", default=None, help="experiment yml")
    ap.add_argument("--out", required=True, help="output directory for <frame>_objects.npz")
    ap.add_argument("--max-points", type=int, default=0, help="points kept per object (0 = all)")
    ap.add_argument("--track", action="store_true", help="stable ids across the frames (taken in file order)")
    ap.add_argument("--track-min-iou", type=float, default=0.3)
    ap.add_argument("--track-max-age", type=int, default=5)
    ap.add_argument("--reid", action="store_true", help="with --track: identities that survive a jump or a long occlusion")
    ap.add_argument("--reid-min-sim", type=float, default=0.7)
    ap.add_argument("--reid-min-size", type=float, default=0.25)
    ap.add_argument("--reid-max-lost", type=int, default=300)
    ap.add_argument("--motion", action="store_true", help="with --track: how every object moved on the table since the frame before")
    ap.add_argument("--motion-angles", type=int, default=32, help="with --motion: rotations over a full turn (1..64)")
    ap.add_argument("--motion-radius", type=int, default=8, help="with --motion: the largest shift past the centroids' travel, cells (0..16)")
    ap.add_argument("--components", choices=["all", "largest"], default=None,
                    help="split the label map into connected components first (off by default)")
    ap.add_argument("--min-area", type=int, default=1, help="components below this many pixels become background")
    ap.add_argument("--plane", action="store_true", help="fit the support plane and add heights and upright boxes")
    ap.add_argument("--min-height", type=float, default=None, help="with --plane: add `standing` (top at least this high, metres)")
    ap.add_argument("--relations", action="store_true", help="add layers, pick order and the front / touch tables of the objects")
    ap.add_argument("--relations-gap", type=float, default=0.015, help="depth step (metres) that puts a pixel in front of its neighbour")
    ap.add_argument("--relations-min-pairs", type=int, default=8, help="pixel pairs that make a relation")
    ap.add_argument("--placement", type=float, default=None, metavar="RADIUS_M",
                    help="add the free space on the support plane and the widest spot for a disc of this radius (metres)")
    ap.add_argument("--grid", type=int, default=256, help="with --placement: cells per side (a multiple of 8 in 8..512)")
    ap.add_argument("--cell-mm", type=int, default=10, help="with --placement: cell size in millimetres")
    ap.add_argument("--memory", type=int, default=None, metavar="AGE",
                    help="with --placement: fuse the table grid over the frames; a hidden cell keeps its last sighting for AGE steps")
    ap.add_argument("--grasp", type=float, default=None, metavar="MAX_OPEN_M",
                    help="add the parallel-jaw grasp candidates of the objects for a gripper that opens this far (metres)")
    ap.add_argument("--grasp-angles", type=int, default=16, help="with --grasp: closing directions over half a turn (1..32)")
    ap.add_argument("--grasp-offsets", type=int, default=2, help="with --grasp: lateral offsets to either side, in cells (0..8)")
    ap.add_argument("--elevation", type=float, default=None, metavar="STEP_M",
                    help="add the tops of the objects on the elevation map; cells climbing at most this far (metres) are level")
    ap.add_argument("--elevation-min-pts", type=int, default=2, help="with --elevation: points near a cell's top that make it solid")
    ap.add_argument("--putdown", type=float, nargs=2, default=None, metavar=("LENGTH_M", "WIDTH_M"),
                    help="add the oriented put-down poses of a rectangle of this length and width (metres) on the table grid")
    ap.add_argument("--putdown-angles", type=int, default=16, help="with --putdown: orientations over half a turn (1..32)")
    ap.add_argument("--route", nargs=2, default=None, metavar=("ID", "RADIUS_M"),
                    help="with --placement: add the slide path of object ID, as a disc of this radius (metres), to the widest spot")
    ap.add_argument("--confidence", type=float, nargs="?", const=0.02, default=None, metavar="WEAK",
                    help="add the assignment-margin map and per object its mean, minimum and the share of pixels below WEAK (0.02)")
    ap.add_argument("--normals", action="store_true",
                    help="add the per-pixel surface normals, their classes against the support plane and the faces of the objects")
    ap.add_argument("--planes", type=int, default=None, metavar="K",
                    help="extract up to K planes (1..8) and add them, the index map and the plane every object stands on")
    ap.add_argument("--planes-up", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="with --planes: the direction away from the floor, camera coordinates")
    return ap


CHECKS = (       # what parse_args refuses, in the order it looks: (whether the command line is wrong, what ap.error then says)
    (lambda a: a.confidence is not None and not 0.0 <= a.confidence <= 1.0, "--confidence WEAK: a margin in 0..1"),
    (lambda a: a.reid and not a.track, "--reid needs --track (identities are kept per track)"),
    (lambda a: a.reid and not (0.0 < a.reid_min_sim <= 1.0 and 0.0 <= a.reid_min_size <= 1.0 and a.reid_max_lost >= 0),
     "--reid-min-sim in (0, 1], --reid-min-size in [0, 1], --reid-max-lost not negative"),
    (lambda a: a.motion and not a.track, "--motion needs --track (an object is followed by the id it keeps)"),
    (lambda a: a.motion and not (1 <= a.motion_angles <= 64 and 0 <= a.motion_radius <= 16), "--motion-angles in 1..64, --motion-radius in 0..16"),
    (lambda a: a.memory is not None and a.placement is None, "--memory needs --placement (it remembers the grid that --placement computes)"),
    (lambda a: a.memory is not None and not 0 <= a.memory <= 32767, "--memory AGE: AGE in 0..32767"),
    (lambda a: a.planes is not None and not 1 <= a.planes <= 8, "--planes K: K in 1..8"),
    (lambda a: a.planes is not None and a.plane, "--planes and --plane both write plane_* arrays: give one of them"),
    (lambda a: a.planes_up is not None and a.planes is None, "--planes-up needs --planes"),
    (lambda a: a.planes_up is not None and not any(a.planes_up), "--planes-up X Y Z: not the zero vector"),
    (lambda a: a.route is not None and a.placement is None, "--route needs --placement (it routes to the spot that --placement finds)"),
)


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    for wrong, message in CHECKS:
        if wrong(args):
            ap.error(message)
    if args.route is not None:
        try:
            args.route = (int(args.route[0]), float(args.route[1]))
        except ValueError:
            ap.error("--route ID RADIUS_M: an integer id and a radius in metres")
        if not 1 <= args.route[0] <= 127 or args.route[1] < 0:
            ap.error("--route ID RADIUS_M: ID in 1..127, RADIUS_M not negative")
    return args


class Frame:
    """One frame on its way through the stages.  `final` (host) and `labels` (device) are the label map the stages pass on,
    from `record` on the exported one as int32; it and the XYZ planes go to the device once, here.  The methods below the
    properties are stages: they take the stream's state and args and return the arrays they add to the file, if any."""

    def __init__(self, args, sample, final, objs, conf):
        self.args, self.sample, self.final, self.objs, self.conf, self.rec = args, sample, final, objs, conf, {}
        self.xyz1 = sample["depth"][:1].to(cfg.device)     # [1,3,H,W], as extract_objects and the identifier take them
        self.labels, self.xyz = final.to(cfg.device), self.xyz1[0]

    @cached_property
    def several(self):
        return fit_planes(self.labels, self.xyz, max_planes=self.args.planes)

    @cached_property
    def plane(self):
        """The support plane of the exported label map, fitted when a stage first asks: under --planes the one most objects stand on."""
        if self.args.planes is None:
            return fit_plane(self.labels, self.xyz)
        return self.several.plane(choose_support(self.several, up=None if self.args.planes_up is None else tuple(self.args.planes_up)))

    @cached_property
    def grid(self):
        """The table grid of --placement, --route, --grasp, --elevation and --putdown on that plane, with the widest-spot
        query of --placement where that is given: the grid itself does not depend on the queries."""
        a, cell = self.args, self.args.cell_mm / 1000.0
        queries = None if a.placement is None else [(need2(a.placement, cell), 0, 0, WIDEST)]
        return free_space(self.labels, self.xyz, self.plane, grid=a.grid, cell=cell, queries=queries)

    def split(self, stream, args):
        split, table, _ = split_components(self.labels, connectivity=8, min_area=args.min_area, mode=args.components)
        if stream.tracker is None:
            self.objs = extract_objects(split, self.xyz1, max_points_per_object=args.max_points)
        self.comp, self.labels, self.final = table[0], split, split.cpu()

    def track(self, stream, args):
        self.raw_map = self.final.numpy().astype(np.int32)
        self.labels = stream.tracker.update(self.labels)
        self.objs = extract_objects(self.labels, self.xyz1, max_points_per_object=args.max_points)
        self.final = self.labels.cpu()

    def record(self, stream, args):
        self.labels = self.ids_map = self.labels.to(torch.int32)     # ids_map: the ids --motion and --memory follow
        self.ids = self.objs.label.long()
        self.id_list = self.ids.cpu().tolist()
        return {**{k: getattr(self.objs, k).cpu().numpy() for k in FIELDS}, "label_map": self.final.numpy().astype(np.int32)}

    def identify(self, stream, args):       # per row: the identity entry of its track slot and that identity's running number
        self.ids_map = stream.identifier.update(self.labels, stream.tracker, identity.image_u8(self.sample).to(cfg.device), self.xyz1)
        entries = stream.identifier.lut[0][self.ids]
        return {"identity": entries.cpu().numpy(), "identity_pid": stream.identifier.table[0, :, 0][entries.long()].cpu().numpy(),
                "identity_map": self.ids_map.cpu().numpy().astype(np.int32)}

    def follow(self, stream, args):
        """The follower keeps a plane of its own for the whole stream, that of the first frame's id map (the camera stands
        still); the first frame has nothing to be registered against."""
        first = stream.follower is None
        if first:
            stream.follower = motion.Follower(fit_plane(self.ids_map, self.xyz), args.grid, args.cell_mm / 1000.0, args.motion_angles, args.motion_radius)
        stream.moved = stream.follower.update(self.ids_map, self.xyz)
        return None if first else motion_arrays(stream.moved)

    def component_rows(self, stream, args):     # per row: the component its pixels came from
        ids = self.ids
        if stream.tracker is not None:          # through the tracker's lut: track slot -> the split map's id
            inverse = torch.zeros(128, dtype=torch.int64, device=cfg.device)
            inverse[stream.tracker.lut[0].long()] = torch.arange(128, device=cfg.device)
            ids = inverse[ids]
        rows = self.comp[ids].cpu().numpy()
        return {"component_src": rows[:, 0], "component_area": rows[:, 1], "component_siblings": rows[:, 3]}

    def route(self, stream, args):
        spot = self.rec["place_widest_cell"]
        goal = (int(spot[0]), int(spot[1])) if spot[0] >= 0 else None
        return route_arrays(routes.plan(self.grid, [routes.of_object(self.grid, self.plane, 0, args.route[0], goal, radius_m=args.route[1])]))

    def remember(self, stream, args):
        """The memory keeps the support plane of the first frame for the whole stream (the camera stands still) and, beside
        --motion, holds the ids that follows: a free_space of its own, which self.grid equals on the first frame alone."""
        if stream.memory_plane is None:
            stream.memory_plane = self.plane
        seen = free_space(self.ids_map if args.motion else self.labels, self.xyz, stream.memory_plane, grid=args.grid, cell=args.cell_mm / 1000.0)
        return memory_arrays(stream.memory.update(seen, drop=moved_ids_mask(stream.moved, cfg.device) if args.motion else None))


STAGES = (      # in the order they run, which is the order of the keys in the file, each with the option that enables it
    ("components", Frame.split),
    ("track", Frame.track),
    (None, Frame.record),
    ("reid", Frame.identify),
    ("track", lambda f, s, a: {"raw_label_map": f.raw_map, "track_uid": s.tracker.table[0, :, 0][f.ids].cpu().numpy()}),
    ("motion", Frame.follow),
    ("components", Frame.component_rows),
    ("planes", lambda f, s, a: planes_arrays(f.several, f.ids, a.planes_up)),
    ("plane", lambda f, s, a: plane_arrays(f.plane, f.ids, a.min_height)),
    ("placement", lambda f, s, a: placement_arrays(f.grid)),
    ("route", Frame.route),
    ("memory", Frame.remember),
    ("grasp", lambda f, s, a: grasp_arrays(candidates(f.grid, angles=a.grasp_angles, offsets=a.grasp_offsets, max_open=a.grasp), f.id_list)),
    ("elevation", lambda f, s, a: elevation_arrays(heights(f.labels, f.xyz, f.grid, step=a.elevation, min_pts=a.elevation_min_pts), f.id_list, a.placement)),
    ("putdown", lambda f, s, a: putdown_arrays(footprint.fit(f.grid, [footprint.rect(*a.putdown, a.cell_mm)], angles=a.putdown_angles))),
    ("relations", lambda f, s, a: relation_arrays(relate(f.labels, f.xyz, connectivity=8, gap=a.relations_gap, min_pairs=a.relations_min_pairs), f.ids)),
    ("confidence", lambda f, s, a: confidence_arrays(summarize(f.labels, f.conf.margin, weak=a.confidence), f.id_list, f.conf.margin)),
    ("normals", lambda f, s, a: normals_arrays(normals.estimate(f.xyz, f.labels, f.plane), f.id_list)),
)


def main():
    args = parse_args()
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    if network_mode() != "RGBD_ADD":
        raise SystemExit("export_objects needs an RGB-D network (the objects are cut from the XYZ planes)")
    np.random.seed(cfg.RNG_SEED)
    cfg.gpu_id = args.gpu
    cfg.device = torch.device("cuda:%d" % args.gpu)
    colors = sorted(glob.glob(os.path.join(args.imgdir, args.color)))
    depths = sorted(glob.glob(os.path.join(args.imgdir, args.depth)))
    assert len(colors) == len(depths) and colors, "need matching colour/depth images"
    cam_file = os.path.join(args.imgdir, "camera_params.json")
    cam = json.load(open(cam_file)) if os.path.exists(cam_file) else dict(synth.DEMO_CAMERA)
    network = networks.seg_resnet34_8s_embedding(2, cfg.TRAIN.NUM_UNITS, load_weights(args.pretrained)).eval()
    network_crop = networks.seg_resnet34_8s_embedding(2, cfg.TRAIN.NUM_UNITS, load_weights(args.pretrained_crop)).eval()
    os.makedirs(args.out, exist_ok=True)
    stream = SimpleNamespace(        # what lasts from frame to frame; the follower and the memory's plane are made on the first one
        tracker=Tracker(min_iou=args.track_min_iou, max_age=args.track_max_age) if args.track else None,
        identifier=identity.Identifier(min_sim=args.reid_min_sim, min_size=args.reid_min_size, max_lost=args.reid_max_lost) if args.reid else None,
        memory=scene.Memory(args.grid, max_age=args.memory, device=cfg.device) if args.memory is not None else None,
        follower=None, memory_plane=None, moved=None)
    stages = [run for option, run in STAGES if option is None or (getattr(args, option) is not None and getattr(args, option) is not False)]
    for fc, fd in zip(colors, depths):
        sample = uio.read_sample(fc, fd, cam)
        confident = dict(confidence=True, confidence_args=dict(weak=args.confidence)) if args.confidence is not None else {}
        out_label, out_refined, objs, *conf = segment_objects(sample, network, network_crop, max_points_per_object=args.max_points, **confident)
        frame = Frame(args, sample, (out_refined if out_refined is not None else out_label)[0], objs, conf[0] if conf else None)
        for run in stages:
            frame.rec.update(run(frame, stream, args) or {})
        stem = os.path.basename(fc)
        stem = stem[:-len("-color.png")] if stem.endswith("-color.png") else os.path.splitext(stem)[0]
        name = os.path.join(args.out, stem + "_objects.npz")
        np.savez(name, **frame.rec)
        print("save objects to {}  ({} objects, {} points)".format(name, len(frame.objs), int(frame.objs.points.shape[0])))


if __name__ == "__main__":
    main()
