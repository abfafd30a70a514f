"""ctypes binding of libuoc_hip.so (include/uoc_hip.h).  No CPU fallback: if the library is
missing or a call fails, this raises — the product path never routes around the HIP kernels."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_size_t, c_void_p, POINTER

from .build import LIB_PATH

_lib = None


class NativeError(RuntimeError):
    pass


def _declare(lib):
    P = c_void_p
    lib.uoc_version.restype = c_int
    lib.uoc_is_dev_build.argtypes = []
    lib.uoc_is_dev_build.restype = c_int
    lib.uoc_config_fingerprint.argtypes = []
    lib.uoc_config_fingerprint.restype = ctypes.c_ulonglong
    lib.uoc_shutdown.restype = c_int
    lib.uoc_reload_env.argtypes = []
    lib.uoc_reload_env.restype = c_int
    lib.uoc_shutdown.argtypes = []
    lib.uoc_last_error.restype = c_char_p
    lib.uoc_ms_set_persistent_fps.argtypes = [c_int]
    lib.uoc_ms_set_persistent_fps.restype = c_int
    lib.uoc_ms_set_stream_ordering.argtypes = [c_int]
    lib.uoc_ms_set_stream_ordering.restype = c_int
    lib.uoc_ms_fps_fallbacks.argtypes = []
    lib.uoc_ms_fps_fallbacks.restype = c_int
    lib.uoc_ms_workspace_bytes.restype = c_size_t
    lib.uoc_ms_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_ms_select_seeds.argtypes = [P, c_int, c_int, c_int, P, P, P, P, c_size_t, P]
    lib.uoc_ms_select_seeds_from.argtypes = [P, c_int, c_int, c_int, c_int, P, P, P, P, c_size_t, P]
    lib.uoc_ms_hill_climb.argtypes = [P, c_int, c_int, P, c_int, c_float, c_int, P, c_size_t, P]
    lib.uoc_ms_seed_components.argtypes = [P, c_int, c_int, c_float, P, P, P]
    lib.uoc_ms_assign.argtypes = [P, c_int, c_int, P, P, P, c_int, P, P, P, c_size_t, P]
    lib.uoc_ms_cluster.argtypes = [P, c_int, c_int, c_int, c_float, c_int, c_float, P, P, P, P, P, P, c_size_t, P]
    lib.uoc_ms_check.argtypes = [P]
    lib.uoc_ms_check.restype = c_int
    lib.uoc_ms_workspace_bytes_wide.restype = c_size_t
    lib.uoc_ms_workspace_bytes_wide.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_ms_cluster_wide.argtypes = [P, c_int, c_int, c_int, c_int, c_float, c_int, c_float, P, P, P, P, P, P, c_size_t, P]
    lib.uoc_ms_cluster_wide.restype = c_int
    # the same calls with the embedding metric (METRIC_COSINE / METRIC_EUCLIDEAN) as an argument
    lib.uoc_ms_select_seeds_ex.argtypes = [P, c_int, c_int, c_int, c_int, P, P, P, c_int, P, c_size_t, P]
    lib.uoc_ms_hill_climb_ex.argtypes = [P, c_int, c_int, P, c_int, c_float, c_int, c_int, P, c_size_t, P]
    lib.uoc_ms_seed_components_ex.argtypes = [P, c_int, c_int, c_float, c_int, P, P, P]
    lib.uoc_ms_assign_ex.argtypes = [P, c_int, c_int, P, P, P, c_int, c_int, P, P, P, c_size_t, P]
    lib.uoc_ms_cluster_ex.argtypes = [P, c_int, c_int, c_int, c_float, c_int, c_float, c_int, P, P, P, P, P, P, c_size_t, P]
    lib.uoc_ms_cluster_wide_ex.argtypes = [P, c_int, c_int, c_int, c_int, c_float, c_int, c_float, c_int, P, P, P, P, P, P,
                                           c_size_t, P]
    for name in METRIC_SYMBOLS:
        getattr(lib, name).restype = c_int
    lib.uoc_net_embed_dim.argtypes = [P]
    lib.uoc_net_embed_dim.restype = c_int
    lib.uoc_net_create.argtypes = [POINTER(P)]
    lib.uoc_net_create_mode.argtypes = [POINTER(P), c_int]
    lib.uoc_net_destroy.argtypes = [P]
    lib.uoc_net_load_param.argtypes = [P, c_char_p, P, c_size_t]
    lib.uoc_net_finalize.argtypes = [P]
    lib.uoc_net_workspace_bytes.restype = c_size_t
    lib.uoc_net_workspace_bytes.argtypes = [P, c_int, c_int, c_int]
    lib.uoc_net_forward.argtypes = [P, P, P, c_int, c_int, c_int, P, P, c_size_t, P]
    lib.uoc_net_set_split_precision.argtypes = [P, c_int]
    lib.uoc_net_set_split_precision.restype = c_int
    lib.uoc_conv2d_nhwc.argtypes = [P, P, P, P, P] + [c_int] * 11 + [P]
    lib.uoc_conv2d_nhwc_algo.argtypes = [P, P, P, P, P] + [c_int] * 12 + [P]
    lib.uoc_conv2d_nhwc_algo.restype = c_int
    # test entries: one tile instantiation at a time; stem, pooling and head on their own
    lib.uoc_conv2d_tile_list.argtypes = [c_int, P, c_int]
    lib.uoc_conv2d_nhwc_tile.argtypes = [P, P, P, P, P] + [c_int] * 12 + [P, c_int, c_int]
    lib.uoc_conv2d_tile_choice.argtypes = [c_int] * 10 + [P, P, P]
    lib.uoc_net_stem.argtypes = [P, P, P, P] + [c_int] * 5 + [P, P]
    lib.uoc_maxpool3x3s2_nhwc.argtypes = [P, P] + [c_int] * 4 + [P]
    lib.uoc_head.argtypes = [P, P, P] + [c_int] * 6 + [P]
    for name in TILE_SYMBOLS:
        getattr(lib, name).restype = c_int
    for name in ("uoc_net_create", "uoc_net_create_mode", "uoc_net_destroy", "uoc_net_load_param", "uoc_net_finalize", "uoc_net_forward",
                 "uoc_conv2d_nhwc"):
        getattr(lib, name).restype = c_int
    lib.uoc_eval_workspace_bytes.restype = c_size_t
    lib.uoc_eval_workspace_bytes.argtypes = [c_int, c_int]
    lib.uoc_eval_pair_stats.argtypes = [P, P, c_int, c_int, c_int, P, P, c_size_t, P]
    lib.uoc_eval_pair_stats.restype = c_int
    lib.uoc_roi_workspace_bytes.restype = c_size_t
    lib.uoc_roi_workspace_bytes.argtypes = []
    lib.uoc_prep_rgbd.argtypes = [P, P, c_int, c_int] + [c_float] * 7 + [P, P, P]
    lib.uoc_prep_rgbd.restype = c_int
    lib.uoc_filter_labels_depth.argtypes = [P, P, ctypes.c_long, c_int, c_int, c_int, c_float, P, c_size_t, P]
    lib.uoc_roi_build.argtypes = [P, P, c_int, c_int, c_float, c_float, P, P, c_size_t, P]
    lib.uoc_roi_crop.argtypes = [P, P, P, c_int, c_int, P, c_int, c_int, P, P, P, P]
    lib.uoc_roi_match_stats.argtypes = [P, P, P, c_int, c_int, P, P, P, c_size_t, P]
    lib.uoc_roi_paste.argtypes = [P, P, P, P, c_int, c_int, c_int, c_int, P, P]
    lib.uoc_labels_to_u8.argtypes = [P, ctypes.c_long, P, P, P]
    lib.uoc_roi_match.argtypes = [P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, c_size_t, P]
    for name in ("uoc_filter_labels_depth", "uoc_roi_build", "uoc_roi_crop", "uoc_roi_match_stats", "uoc_roi_paste", "uoc_labels_to_u8", "uoc_roi_match"):
        getattr(lib, name).restype = c_int
    lib.uoc_objects_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_objects_workspace_bytes.restype = c_size_t
    lib.uoc_objects.argtypes = [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, ctypes.c_long, P, P, c_size_t, P]
    lib.uoc_objects.restype = c_int
    lib.uoc_track_state_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_track_state_bytes.restype = c_size_t
    lib.uoc_track_workspace_bytes.argtypes = [c_int]
    lib.uoc_track_workspace_bytes.restype = c_size_t
    lib.uoc_track_reset.argtypes = [P, c_int, c_int, c_int, c_int, P]
    lib.uoc_track_reset.restype = c_int
    lib.uoc_track_step.argtypes = [P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, c_size_t, P]
    lib.uoc_track_step.restype = c_int
    lib.uoc_cc_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_cc_workspace_bytes.restype = c_size_t
    lib.uoc_cc_split.argtypes = [P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, c_size_t, P]
    lib.uoc_cc_split.restype = c_int
    lib.uoc_plane_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_plane_workspace_bytes.restype = c_size_t
    lib.uoc_support_plane.argtypes = [P, P, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint32, P, P, P, P, c_size_t, P]
    lib.uoc_support_plane.restype = c_int
    lib.uoc_planes_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.uoc_planes_workspace_bytes.restype = c_size_t
    lib.uoc_support_planes.argtypes = [P, P] + [c_int] * 8 + [ctypes.c_uint32, P, P, P, P, P, P, c_size_t, P]
    lib.uoc_support_planes.restype = c_int
    lib.uoc_relations_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_relations_workspace_bytes.restype = c_size_t
    lib.uoc_relations.argtypes = [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, c_size_t, P]
    lib.uoc_relations.restype = c_int
    lib.uoc_placement_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_placement_workspace_bytes.restype = c_size_t
    lib.uoc_placement.argtypes = [P, P, P] + [c_int] * 9 + [P, c_int, P, P, P, P, P, P, P, c_size_t, P]
    lib.uoc_placement.restype = c_int
    lib.uoc_grasp_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_grasp_workspace_bytes.restype = c_size_t
    lib.uoc_grasp.argtypes = [P, P, c_int, c_int, P] + [c_int] * 7 + [P, P, P, c_size_t, P]
    lib.uoc_grasp.restype = c_int
    lib.uoc_elevation_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_elevation_workspace_bytes.restype = c_size_t
    lib.uoc_elevation.argtypes = [P, P, P] + [c_int] * 8 + [P, c_int] + [P] * 9 + [c_size_t, P]
    lib.uoc_elevation.restype = c_int
    lib.uoc_footprint_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_footprint_workspace_bytes.restype = c_size_t
    lib.uoc_footprint.argtypes = [P, P, P, P, c_int, c_int, P, c_int, P, c_int, c_int, P, P, P, P, c_size_t, P]
    lib.uoc_footprint.restype = c_int
    lib.uoc_routes_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_routes_workspace_bytes.restype = c_size_t
    lib.uoc_routes.argtypes = [P, P, P, c_int, c_int, P, c_int, c_int, c_int, P, P, P, P, c_size_t, P]
    lib.uoc_routes.restype = c_int
    lib.uoc_ms_confidence_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.uoc_ms_confidence_workspace_bytes.restype = c_size_t
    lib.uoc_ms_confidence.argtypes = [P, c_int, c_int, c_int, P, P, P, c_int, c_int, P, P, P, P, P, P, c_size_t, P]
    lib.uoc_ms_confidence.restype = c_int
    lib.uoc_conf_paste.argtypes = [P, P, P, P, c_int, c_int, c_int, c_int, P, P]
    lib.uoc_conf_paste.restype = c_int
    lib.uoc_conf_objects.argtypes = [P, P, c_int, c_int, c_int, c_int, P, P]
    lib.uoc_conf_objects.restype = c_int
    lib.uoc_normals_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.uoc_normals_workspace_bytes.restype = c_size_t
    lib.uoc_normals.argtypes = [P, P, P] + [c_int] * 7 + [P, c_int, c_int, c_int, P, P, P, P, c_size_t, P]
    lib.uoc_normals.restype = c_int
    lib.uoc_lzf_decompress.argtypes = [P, c_size_t, P, c_size_t]
    lib.uoc_lzf_decompress.restype = ctypes.c_long
    lib.uoc_prof_enable.argtypes = [c_int]
    lib.uoc_prof_reset.argtypes = []
    lib.uoc_prof_report.argtypes = [ctypes.c_char_p, c_size_t]
    for name in ("uoc_prof_enable", "uoc_prof_reset", "uoc_prof_report"):
        getattr(lib, name).restype = c_int
    for name in ("uoc_ms_select_seeds", "uoc_ms_select_seeds_from", "uoc_ms_hill_climb", "uoc_ms_seed_components", "uoc_ms_assign",
                 "uoc_ms_cluster"):
        getattr(lib, name).restype = c_int


# include/uoc_hip.h: UOC_METRIC_COSINE / UOC_METRIC_EUCLIDEAN, the metric argument of the *_ex clustering calls
METRIC_COSINE = 0
METRIC_EUCLIDEAN = 1
METRICS = {"cosine": METRIC_COSINE, "euclidean": METRIC_EUCLIDEAN}
METRIC_SYMBOLS = ("uoc_ms_select_seeds_ex", "uoc_ms_hill_climb_ex", "uoc_ms_seed_components_ex", "uoc_ms_assign_ex",
                  "uoc_ms_cluster_ex", "uoc_ms_cluster_wide_ex")


TILE_SYMBOLS = ("uoc_conv2d_tile_list", "uoc_conv2d_nhwc_tile", "uoc_conv2d_tile_choice", "uoc_net_stem",
                "uoc_maxpool3x3s2_nhwc", "uoc_head")


def metric_code(metric) -> int:
    """cfg.TRAIN.EMBEDDING_METRIC / the reference's metric= string -> the C ABI's metric argument."""
    if metric not in METRICS:
        raise NotImplementedError(f"metric={metric!r}: only 'cosine' and 'euclidean' are implemented on gfx950")
    return METRICS[metric]


# every symbol include/uoc_hip.h declares (tests check the .so exports them all)
EXPORTED_SYMBOLS = (
    "uoc_version", "uoc_is_dev_build", "uoc_config_fingerprint", "uoc_shutdown", "uoc_last_error", "uoc_reload_env", "uoc_ms_set_persistent_fps", "uoc_ms_set_stream_ordering", "uoc_ms_fps_fallbacks", "uoc_ms_check", "uoc_ms_workspace_bytes", "uoc_ms_select_seeds", "uoc_ms_select_seeds_from", "uoc_ms_hill_climb",
    "uoc_ms_seed_components", "uoc_ms_assign", "uoc_ms_cluster", "uoc_ms_workspace_bytes_wide", "uoc_ms_cluster_wide",
) + METRIC_SYMBOLS + (
    "uoc_net_embed_dim",
    "uoc_net_create", "uoc_net_create_mode", "uoc_net_destroy", "uoc_net_load_param", "uoc_net_finalize", "uoc_net_workspace_bytes",
    "uoc_net_forward", "uoc_net_set_split_precision", "uoc_conv2d_nhwc", "uoc_conv2d_nhwc_algo",
) + TILE_SYMBOLS + (
    "uoc_roi_workspace_bytes", "uoc_prep_rgbd", "uoc_filter_labels_depth", "uoc_roi_build", "uoc_roi_crop", "uoc_roi_match_stats",
    "uoc_roi_paste", "uoc_roi_match", "uoc_labels_to_u8", "uoc_eval_workspace_bytes", "uoc_eval_pair_stats", "uoc_objects_workspace_bytes", "uoc_objects",
    "uoc_track_state_bytes", "uoc_track_workspace_bytes", "uoc_track_reset", "uoc_track_step",
    "uoc_cc_workspace_bytes", "uoc_cc_split", "uoc_plane_workspace_bytes", "uoc_support_plane",
    "uoc_planes_workspace_bytes", "uoc_support_planes",
    "uoc_relations_workspace_bytes", "uoc_relations", "uoc_placement_workspace_bytes", "uoc_placement",
    "uoc_grasp_workspace_bytes", "uoc_grasp", "uoc_elevation_workspace_bytes", "uoc_elevation",
    "uoc_footprint_workspace_bytes", "uoc_footprint", "uoc_routes_workspace_bytes", "uoc_routes",
    "uoc_ms_confidence_workspace_bytes", "uoc_ms_confidence", "uoc_conf_paste", "uoc_conf_objects",
    "uoc_normals_workspace_bytes", "uoc_normals", "uoc_lzf_decompress", "uoc_prof_enable", "uoc_prof_reset", "uoc_prof_report",
)


class RoiTable(ctypes.Structure):
    """Mirror of uoc_roi_table (include/uoc_hip.h)."""
    _fields_ = [("K", c_int32), ("label", c_int32 * 128), ("box", (c_int32 * 4) * 128)]


ROI_TABLE_BYTES = ctypes.sizeof(RoiTable)


class UocObject(ctypes.Structure):
    """Mirror of uoc_object (include/uoc_hip.h): one per (frame, id)."""
    _fields_ = [("pixels", c_int32), ("count", c_int32), ("box", c_int32 * 4), ("centroid", c_float * 3), ("cov", c_float * 6),
                ("aabb_min", c_float * 3), ("aabb_max", c_float * 3), ("eig", c_float * 3), ("axes", c_float * 9),
                ("obb_center", c_float * 3), ("obb_half", c_float * 3), ("offset", c_int32), ("kept", c_int32)]


OBJECT_BYTES = ctypes.sizeof(UocObject)


class UocPlane(ctypes.Structure):
    """Mirror of uoc_plane (include/uoc_hip.h): one per frame."""
    _fields_ = [("found", c_int32), ("candidates", c_int32), ("inliers", c_int32), ("hyp", c_int32), ("normal", c_float * 3),
                ("d", c_float), ("centroid", c_float * 3), ("eig", c_float * 3), ("rms", c_float), ("u", c_float * 3),
                ("v", c_float * 3)]


class UocPlaneObject(ctypes.Structure):
    """Mirror of uoc_plane_object (include/uoc_hip.h): one per (frame, id)."""
    _fields_ = [("count", c_int32), ("height_min", c_float), ("height_max", c_float), ("foot", c_float * 2),
                ("cov2", c_float * 3), ("axis", c_float * 2), ("half", c_float * 3), ("center", c_float * 3)]


class UocPlaneInfo(ctypes.Structure):
    """Mirror of uoc_plane_info (include/uoc_hip.h): one per (frame, plane)."""
    _fields_ = [("round_candidates", c_int32), ("removed", c_int32), ("cos0", c_float), ("offset0", c_float),
                ("extent", c_float * 4)]


class UocRelationObject(ctypes.Structure):
    """Mirror of uoc_relation_object (include/uoc_hip.h): one per (frame, id)."""
    _fields_ = [(name, c_int32) for name in ("pixels", "edge", "border", "border_bg", "hidden", "n_touch", "n_above", "n_below",
                                             "layer", "free", "order")]


REL_BORDER, REL_TOUCH, REL_FRONT = 0, 1, 2      # include/uoc_hip.h: UOC_REL_*, the planes of uoc_relations' d_pairs
REL_MAX_GAP_MM = 65535
PLANE_MAX_HYP = 1024            # include/uoc_hip.h: num_hyp in 1..1024, tau_mm in 1..1000
PLANE_MAX_TAU_MM = 1000
PLANES_MAX = 8                  # uoc_support_planes: max_planes in 1..8
PLANES_FRINGE = 16              # its index map: 16 + r marks plane r's removal band outside its inliers
PLACE_WIDEST, PLACE_NEAREST = 0, 1              # include/uoc_hip.h: UOC_PLACE_*, the mode of a placement query
PLACE_MAX_QUERIES = 16
PLACE_MAX_GRID = 512                            # grid: a multiple of 8 in 8..512
PLACE_MAX_MM = 1000                             # cell_mm, tau_mm in 1..1000, h_obs_mm in 0..1000
PLACE_MAX_MIN_PTS = 65535
PLACE_MAX_ANCHOR = 4096                         # a query's anchor cell lies in -4096..4095
PLACE_SCALE = 16384                             # S of the integer frame
GRASP_MISS, GRASP_WIDE, GRASP_PINCHED, GRASP_BLOCKED = -1, -2, -3, -4      # include/uoc_hip.h: UOC_GRASP_*, a candidate's code
GRASP_SCALE = 16384                             # S of the direction table and of the anchor
GRASP_MAX_DIRS = 32                             # A in 1..32
GRASP_MAX_OFFSETS = 8                           # M in 0..8
GRASP_MAX_OPEN = 64                             # Wmax in 1..64 cells
GRASP_MAX_GAP = 4                               # gap in 0..4 cells
GRASP_MAX_FINGER = 8                            # F in 1..8 cells
GRASP_MAX_PAD = 4                               # Hp in 0..4 cells
ELEV_NONE = -32768                              # include/uoc_hip.h: UOC_ELEV_NONE, the elev of a cell without a point
ELEV_MAX_QUERIES = 16                           # UOC_ELEV_MAX_QUERIES
FOOT_MAX_RECTS = 8                              # include/uoc_hip.h: UOC_FOOT_MAX_RECTS
FOOT_MAX_HALF = 16384                           # UOC_FOOT_MAX_HALF: a half extent in 1/256 cell, and HL^2 + HW^2 <= its square
FOOT_ROOMIEST, FOOT_NEAREST = 0, 1              # UOC_FOOT_*: a rectangle's mode
ROUTES_MAX_QUERIES = 8                          # include/uoc_hip.h: UOC_ROUTES_MAX_QUERIES
ROUTES_MAX_NEED2 = 4096                         # UOC_ROUTES_MAX_NEED2: a query's need2 in 0..4096
ROUTES_MAX_PATH = 4096                          # UOC_ROUTES_MAX_PATH: max_path in 1..4096
CONF_MAX_N = 1 << 30                            # include/uoc_hip.h: UOC_CONF_MAX_N, pixels per field / frame of the confidence calls
CONF_ONE = 65536                                # the fixed-point unit of uoc_conf_objects' q
NORMAL_UP, NORMAL_SIDE, NORMAL_OBLIQUE, NORMAL_DOWN = 1, 2, 3, 4      # include/uoc_hip.h: UOC_NORMAL_*, the class of a normal
NORMALS_MAX_DIRS = 32                           # UOC_NORMALS_MAX_DIRS: A in 1..32
NORMALS_FACE_WORDS = 40                         # UOC_NORMALS_FACE_WORDS: eight counters and the histogram per id


class UocTrack(ctypes.Structure):
    """Mirror of uoc_track (include/uoc_hip.h): one per (stream, slot)."""
    _fields_ = [("uid", c_int32), ("age", c_int32), ("hits", c_int32), ("area", c_int32), ("born", c_int32)]


TRACK_FIELDS = tuple(name for name, _ in UocTrack._fields_)
TRACK_SLOTS = 128               # slot 0 is never a track
TRACK_HEADER_WORDS = 1024       # int32 words of a stream's state before its contingency scratch (include/uoc_hip.h)
TRACK_META_WORD = 640           # ... of which words 640, 641, 642 = uids handed out, step, dropped
TRACK_CONT_WORDS = 128 * 128
CC_ALL, CC_LARGEST = 0, 1      # include/uoc_hip.h: UOC_CC_ALL / UOC_CC_LARGEST, the mode argument of uoc_cc_split
CC_MODES = {"all": CC_ALL, "largest": CC_LARGEST}
CC_FIELDS = ("src", "area", "root", "siblings")        # the columns of uoc_cc_split's table
OBJECTS_MAX_ATTR = 8        # include/uoc_hip.h: UOC_OBJECTS_MAX_ATTR


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} not found: build it with `python -m unseenobjectclustering_amd.build` "
                "(or __graft_entry__.build()).  There is no CPU fallback.")
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so); it must be the one the process
        # loads first, otherwise this library would pull /opt/rocm's copy in and the two runtimes clash
        # ("no ROCm-capable device is detected").  Importing torch before dlopen guarantees sharing.
        import torch  # noqa: F401
        l = ctypes.CDLL(LIB_PATH)
        try:
            _declare(l)
        except AttributeError as e:          # a library built from an older tree: no quiet fall-back, rebuild it
            raise NativeError(f"{LIB_PATH} lacks a symbol of include/uoc_hip.h ({e}): rebuild it with "
                              "`python -m unseenobjectclustering_amd.build`") from e
        _lib = l
        import atexit
        atexit.register(l.uoc_shutdown)
    return _lib


CONV_DIRECT, CONV_WINOGRAD4, CONV_WINOGRAD4_BF16X3 = 0, 4, 5       # include/uoc_hip.h: UOC_CONV_*


def config_fingerprint() -> int:
    """uoc_config_fingerprint(): what could make two ranks compute different bits (library version / development build and
    its rounding-affecting knobs).  runner.run_sharded compares it across ranks."""
    return int(lib().uoc_config_fingerprint())


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().uoc_last_error().decode("utf-8", "replace")
        raise NativeError(f"{what} failed (rc={rc}): {msg}")


def on_gpu(t) -> bool:
    """True for a torch tensor on a GPU: what every entry point without a CPU fallback asks of its inputs."""
    import torch
    return isinstance(t, torch.Tensor) and t.device.type == "cuda"


class Fields:
    """Base of every result class: the keyword arguments become the attributes.  A result class derives from it and adds
    its name, its docstring and what methods it has."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def as_labels(labels):
    """A label map as the kernels read it: int32 and contiguous; a tensor that already is comes back itself."""
    import torch
    return (labels if labels.dtype == torch.int32 else labels.to(torch.int32)).contiguous()


def label_input(who, labels):
    """The labels-only input check: `labels` on the GPU, else `who`'s NativeError, then as_labels.  Shapes are the
    caller's: the stages that take labels alone differ in what they accept."""
    if not on_gpu(labels):
        raise NativeError(f"{who}: labels must be a tensor on the GPU (there is no CPU fallback)")
    return as_labels(labels)


def frame_inputs(who, labels, xyz):
    """The input check of every stage that takes a label map with its XYZ planes: both on the GPU, [H,W] and [3,H,W]
    batched to B = 1, [B,H,W] against [B,3,H,W], one device; else `who`'s NativeError.  Returns (labels int32, xyz
    float32), both contiguous; a tensor that already is comes back itself, so the hot path copies nothing."""
    import torch
    for t, what in ((labels, "labels"), (xyz, "xyz")):
        if not on_gpu(t):
            raise NativeError(f"{who}: {what} must be a tensor on the GPU (there is no CPU fallback)")
    if labels.dim() == 2:
        labels = labels[None]
    if xyz.dim() == 3:
        xyz = xyz[None]
    if labels.dim() != 3 or xyz.dim() != 4 or xyz.shape[1] != 3 or xyz.shape[0] != labels.shape[0] \
            or tuple(xyz.shape[2:]) != tuple(labels.shape[1:]):
        raise NativeError(f"{who}: labels {tuple(labels.shape)} and xyz {tuple(xyz.shape)} do not match "
                          "([B,H,W] and [B,3,H,W])")
    if xyz.device != labels.device:
        raise NativeError(f"{who}: labels and xyz are on different devices")
    return as_labels(labels), xyz.to(torch.float32).contiguous()


def ptr(t):
    """Device (or host) pointer of a torch tensor as c_void_p; None -> NULL."""
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


def stream_ptr(device=None):
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def stream_key(device):
    """(device type, index, current HIP stream handle): the key of every per-stream scratch cache, so that frames in
    flight on different streams never share a workspace."""
    import torch
    return (device.type, device.index, int(torch.cuda.current_stream(device).cuda_stream))


_retired = []
GRAPHS_ALIVE = 0          # captured hipGraphs in this process (fcn/graph_replay.py)


def retire(t):
    """A per-stream scratch buffer that is being replaced by a larger one.  Captured hipGraphs bake device addresses, so
    once any graph exists the old buffer is kept alive (a bounded leak: buffers grow geometrically / by ROI count)
    instead of going back to the allocator."""
    if t is not None and GRAPHS_ALIVE > 0:
        _retired.append(t)


def prof_enable(on: bool):
    lib().uoc_prof_reset()
    lib().uoc_prof_enable(1 if on else 0)


def prof_report():
    """Per-kernel-class totals recorded since prof_enable(True): list of dicts."""
    import json
    buf = ctypes.create_string_buffer(1 << 19)
    check(lib().uoc_prof_report(buf, len(buf)), "uoc_prof_report")
    return json.loads(buf.value.decode())
