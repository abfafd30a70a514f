"""ctypes binding of libuoc_hip.so (include/uoc_hip.h).  No CPU fallback: if the library is
missing or a call fails, this raises — the product path never routes around the HIP kernels."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_long, c_size_t, c_uint32, c_ulonglong, c_void_p, POINTER

from .build import LIB_PATH

_lib = None


class NativeError(RuntimeError):
    pass


# The C ABI of include/uoc_hip.h, in its order: name -> (restype, argtypes).  tests/test_native_abi.py parses the header and
# holds every entry to its prototype.  Every pointer is a c_void_p: a tensor's data_ptr(), None or a ctypes array passes.
P, I, F, Z, L, U = c_void_p, c_int, c_float, c_size_t, c_long, c_uint32
ABI = {
    "uoc_version": (I, []),
    "uoc_is_dev_build": (I, []),
    "uoc_config_fingerprint": (c_ulonglong, []),
    "uoc_shutdown": (I, []),
    "uoc_last_error": (c_char_p, []),
    "uoc_reload_env": (I, []),
    "uoc_ms_set_persistent_fps": (I, [I]),
    "uoc_ms_set_stream_ordering": (I, [I]),
    "uoc_ms_fps_fallbacks": (I, []),
    "uoc_ms_check": (I, [P]),
    "uoc_ms_workspace_bytes": (Z, [I, I, I]),
    "uoc_ms_select_seeds": (I, [P, I, I, I, P, P, P, P, Z, P]),
    "uoc_ms_select_seeds_from": (I, [P, I, I, I, I, P, P, P, P, Z, P]),
    "uoc_ms_hill_climb": (I, [P, I, I, P, I, F, I, P, Z, P]),
    "uoc_ms_seed_components": (I, [P, I, I, F, P, P, P]),
    "uoc_ms_assign": (I, [P, I, I, P, P, P, I, P, P, P, Z, P]),
    "uoc_ms_cluster": (I, [P, I, I, I, F, I, F, P, P, P, P, P, P, Z, P]),
    "uoc_ms_workspace_bytes_wide": (Z, [I, I, I, I]),
    "uoc_ms_cluster_wide": (I, [P, I, I, I, I, F, I, F, P, P, P, P, P, P, Z, P]),
    "uoc_ms_select_seeds_ex": (I, [P, I, I, I, I, P, P, P, I, P, Z, P]),
    "uoc_ms_hill_climb_ex": (I, [P, I, I, P, I, F, I, I, P, Z, P]),
    "uoc_ms_seed_components_ex": (I, [P, I, I, F, I, P, P, P]),
    "uoc_ms_assign_ex": (I, [P, I, I, P, P, P, I, I, P, P, P, Z, P]),
    "uoc_ms_cluster_ex": (I, [P, I, I, I, F, I, F, I, P, P, P, P, P, P, Z, P]),
    "uoc_ms_cluster_wide_ex": (I, [P, I, I, I, I, F, I, F, I, P, P, P, P, P, P, Z, P]),
    "uoc_net_create": (I, [POINTER(P)]),
    "uoc_net_create_mode": (I, [POINTER(P), I]),
    "uoc_net_embed_dim": (I, [P]),
    "uoc_net_destroy": (I, [P]),
    "uoc_net_load_param": (I, [P, c_char_p, P, Z]),
    "uoc_net_finalize": (I, [P]),
    "uoc_net_workspace_bytes": (Z, [P, I, I, I]),
    "uoc_net_set_split_precision": (I, [P, I]),
    "uoc_net_forward": (I, [P, P, P, I, I, I, P, P, Z, P]),
    "uoc_conv2d_nhwc": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "uoc_conv2d_nhwc_algo": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "uoc_conv2d_tile_list": (I, [I, P, I]),
    "uoc_conv2d_nhwc_tile": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I]),
    "uoc_conv2d_tile_choice": (I, [I, I, I, I, I, I, I, I, I, I, P, P, P]),
    "uoc_net_stem": (I, [P, P, P, P, I, I, I, I, I, P, P]),
    "uoc_maxpool3x3s2_nhwc": (I, [P, P, I, I, I, I, P]),
    "uoc_head": (I, [P, P, P, I, I, I, I, I, I, P]),
    "uoc_roi_workspace_bytes": (Z, []),
    "uoc_prep_rgbd": (I, [P, P, I, I, F, F, F, F, F, F, F, P, P, P]),
    "uoc_filter_labels_depth": (I, [P, P, L, I, I, I, F, P, Z, P]),
    "uoc_roi_build": (I, [P, P, I, I, F, F, P, P, Z, P]),
    "uoc_roi_crop": (I, [P, P, P, I, I, P, I, I, P, P, P, P]),
    "uoc_roi_match_stats": (I, [P, P, P, I, I, P, P, P, Z, P]),
    "uoc_roi_paste": (I, [P, P, P, P, I, I, I, I, P, P]),
    "uoc_roi_match": (I, [P, P, P, P, I, I, I, I, P, P, P, P, P, Z, P]),
    "uoc_labels_to_u8": (I, [P, L, P, P, P]),
    "uoc_eval_workspace_bytes": (Z, [I, I]),
    "uoc_eval_pair_stats": (I, [P, P, I, I, I, P, P, Z, P]),
    "uoc_objects_workspace_bytes": (Z, [I, I, I]),
    "uoc_objects": (I, [P, P, P, I, I, I, I, I, P, P, P, P, L, P, P, Z, P]),
    "uoc_track_state_bytes": (Z, [I, I, I]),
    "uoc_track_workspace_bytes": (Z, [I]),
    "uoc_track_reset": (I, [P, I, I, I, I, P]),
    "uoc_track_step": (I, [P, I, I, I, I, I, P, P, P, P, P, Z, P]),
    "uoc_cc_workspace_bytes": (Z, [I, I, I]),
    "uoc_cc_split": (I, [P, I, I, I, I, I, I, P, P, P, P, Z, P]),
    "uoc_plane_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_support_plane": (I, [P, P, I, I, I, I, I, U, P, P, P, P, Z, P]),
    "uoc_planes_workspace_bytes": (Z, [I, I, I, I, I]),
    "uoc_support_planes": (I, [P, P, I, I, I, I, I, I, I, I, U, P, P, P, P, P, P, Z, P]),
    "uoc_relations_workspace_bytes": (Z, [I, I, I]),
    "uoc_relations": (I, [P, P, I, I, I, I, I, I, P, P, P, Z, P]),
    "uoc_placement_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_placement": (I, [P, P, P, I, I, I, I, I, I, I, I, I, P, I, P, P, P, P, P, P, P, Z, P]),
    "uoc_grasp_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_grasp": (I, [P, P, I, I, P, I, I, I, I, I, I, I, P, P, P, Z, P]),
    "uoc_elevation_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_elevation": (I, [P, P, P, I, I, I, I, I, I, I, I, P, I, P, P, P, P, P, P, P, P, P, Z, P]),
    "uoc_footprint_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_footprint": (I, [P, P, P, P, I, I, P, I, P, I, I, P, P, P, P, Z, P]),
    "uoc_routes_workspace_bytes": (Z, [I, I, I]),
    "uoc_routes": (I, [P, P, P, I, I, P, I, I, I, P, P, P, P, Z, P]),
    "uoc_ms_confidence_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_ms_confidence": (I, [P, I, I, I, P, P, P, I, I, P, P, P, P, P, P, Z, P]),
    "uoc_conf_paste": (I, [P, P, P, P, I, I, I, I, P, P]),
    "uoc_conf_objects": (I, [P, P, I, I, I, I, P, P]),
    "uoc_normals_workspace_bytes": (Z, [I, I, I]),
    "uoc_normals": (I, [P, P, P, I, I, I, I, I, I, I, P, I, I, I, P, P, P, P, Z, P]),
    "uoc_signature_workspace_bytes": (Z, [I]),
    "uoc_signature": (I, [P, P, P, I, I, I, P, P, Z, P]),
    "uoc_sig_similarity": (I, [P, P, I, P, P]),
    "uoc_ident_state_bytes": (Z, [I]),
    "uoc_ident_workspace_bytes": (Z, [I]),
    "uoc_ident_reset": (I, [P, I, I, P]),
    "uoc_ident_step": (I, [P, P, P, I, I, I, I, I, I, P, P, P, P, P, Z, P]),
    "uoc_motion_workspace_bytes": (Z, [I, I, I, I]),
    "uoc_motion": (I, [P, P, P, P, P, P, I, I, P, I, I, P, I, P, P, P, Z, P]),
    "uoc_scene_state_bytes": (Z, [I, I]),
    "uoc_scene_workspace_bytes": (Z, [I, I]),
    "uoc_scene_reset": (I, [P, I, I, I, P]),
    "uoc_scene_step": (I, [P, P, P, P, I, I, I, I, P, I, P, P, P, P, P, P, P, P, P, P, Z, P]),
    "uoc_lzf_decompress": (L, [P, Z, P, Z]),
    "uoc_prof_enable": (I, [I]),
    "uoc_prof_reset": (I, []),
    "uoc_prof_report": (I, [c_char_p, Z]),
}
EXPORTED_SYMBOLS = tuple(ABI)


def _declare(lib):
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


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
SIG_WORDS = 104                                 # include/uoc_hip.h: UOC_SIG_*, the words of a signature
SIG_MAX_N = 1 << 24                             # pixels per frame of uoc_signature: a vote counter is 32 bits
SIG_PIXELS, SIG_VALID, SIG_AREA, SIG_HIST, SIG_DARK, SIG_INTENSITY = 0, 1, 2, 8, 89, 90
IDENT_WORDS = 5                                 # UOC_IDENT_*: an entry of the identity table, IDENT_FIELDS below
IDENT_HEADER_WORDS = 1024                       # int32 words of a stream's identity state before its signatures
IDENT_META_WORD = 640                           # ... of which words 640, 641, 642 = pids handed out, step, evicted
IDENT_FIELDS = ("pid", "uid", "seen", "hits", "pixels")
MOTION_MAX_ROT = 64                             # include/uoc_hip.h: UOC_MOTION_*: A in 1..64 over a full turn
MOTION_MAX_RADIUS = 16                          # R in 0..16 cells
MOTION_MAX_PAIRS = 16                           # P in 1..16
MOTION_MAX_CELLS = 4096                         # cells of a mask; above it status 3
MOTION_SCALE = 16384                            # S of the rotation table
MOTION_ROT_WORDS, MOTION_BEST_WORDS = 4, 16     # a row of rot (cost, si, sj, 0) and of best (motion.BEST_FIELDS)
SCENE_META_WORD, SCENE_MEM_WORD = 32, 48        # include/uoc_hip.h: UOC_SCENE_*: int32 words of a stream's state before its meta / memory words
SCENE_MAX_AGE = 32767                           # max_age in 0..32767
SCENE_ID_WORDS, SCENE_INFO_WORDS = 8, 8         # a row of ids (scene.ID_FIELDS) and of info (scene.INFO_FIELDS)
SCENE_SAME, SCENE_APPEARED, SCENE_VANISHED, SCENE_REOWNED = 0, 1, 2, 3      # a cell's change code


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


CONV_DIRECT, CONV_WINOGRAD4, CONV_WINOGRAD4_BF16X3, CONV_WINOGRAD4_DENSE = 0, 4, 5, 6       # include/uoc_hip.h: UOC_CONV_*


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


def grid_inputs(who, state, owner):
    """The input check of every stage that takes the two table grids of placement.free_space: both on the GPU, [G,G]
    batched to B = 1, square grids of equal shape on one device; else `who`'s NativeError.  Returns (state, owner) int32
    and contiguous; a tensor that already is comes back itself."""
    for t, what in ((state, "state"), (owner, "owner")):
        if not on_gpu(t):
            raise NativeError(f"{who}: {what} must be a tensor on the GPU (there is no CPU fallback)")
    state, owner = (t[None] if t.dim() == 2 else t for t in (state, owner))
    if state.dim() != 3 or state.shape[1] != state.shape[2] or tuple(owner.shape) != tuple(state.shape) or owner.device != state.device:
        raise NativeError(f"{who}: state {tuple(state.shape)} and owner {tuple(owner.shape)} are not two [B,G,G] grids on one device")
    return as_labels(state), as_labels(owner)


def ptr(t):
    """Device (or host) pointer of a torch tensor as c_void_p; None -> NULL."""
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


def stream_ptr(device=None):
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, device, *args, stream=True):
    """lib().<name>(*args, current stream of `device`) under torch.cuda.device(device); a non-zero status raises NativeError
    with uoc_last_error.  A tensor passes as its data_ptr(), None as NULL, ctypes arrays and numbers as they are.
    stream=False: the entry point has no stream argument; device None: it does no device work either."""
    import torch
    fn = getattr(lib(), name)
    args = [a.data_ptr() if hasattr(a, "data_ptr") else a for a in args]
    if device is None:
        rc = fn(*args)
    else:
        with torch.cuda.device(device):
            rc = fn(*args, torch.cuda.current_stream(device).cuda_stream) if stream else fn(*args)
    check(rc, name)


def workspace(name, device, *shape, who, hint, floor=0, zero=False):
    """The scratch tensor (uint8, from torch's stream-ordered cache: no allocation in steady state) of the size the
    *_workspace_bytes function `name` gives for `shape`; a size of 0 is `who`'s NativeError "bad shape <hint>".
    floor > 0: at least that many bytes and no error here, the entry point reports a bad shape itself.  zero: zero-filled,
    for scratch whose contract is "all zero before and after every call"."""
    import torch
    nbytes = getattr(lib(), name)(*shape)
    if nbytes == 0 and floor == 0:
        raise NativeError(f"{who}: bad shape {hint}")
    return (torch.zeros if zero else torch.empty)(max(nbytes, floor), dtype=torch.uint8, device=device)


def host_words(rows, width):
    """A host table of int32 records (queries, directions) as the ctypes array the h_* arguments take: len(rows) * width
    words, at least `width` so that an empty table still has an address."""
    flat = [int(x) for row in rows for x in row]
    return (c_int32 * max(len(flat), width))(*flat)


def stream_key(device):
    """(device type, index, current HIP stream handle): the key of every per-stream scratch cache, so that frames in
    flight on different streams never share a workspace.  A device without an index is the current one: torch.device("cuda")
    and torch.device("cuda", current_device()) give the same key."""
    import torch
    index = torch.cuda.current_device() if device.index is None else device.index
    return (device.type, index, int(torch.cuda.current_stream(device).cuda_stream))


_retired = []
GRAPHS_ALIVE = 0          # captured hipGraphs in this process (fcn/graph_replay.py)


def retire(t):
    """A per-stream scratch buffer that is being replaced by a larger one.  Captured hipGraphs bake device addresses, so
    once any graph exists the old buffer is kept alive (a bounded leak: buffers grow geometrically / by ROI count)
    instead of going back to the allocator."""
    if t is not None and GRAPHS_ALIVE > 0:
        _retired.append(t)


class PerStream:
    """One scratch object per stream_key: get(device, need) returns the current stream's, made by make(device, need) when
    there is none yet or, with a `size` rule, when size(object) < need; the one it replaces is retired."""

    def __init__(self, make, size=None):
        self.make, self.size, self.items = make, size, {}

    def get(self, device, need=0):
        key = stream_key(device)
        obj = self.items.get(key)
        if obj is None or (self.size is not None and self.size(obj) < need):
            retire(obj)
            obj = self.items[key] = self.make(device, need)
        return obj

    def of_device(self, device):
        """The objects of every stream of `device`."""
        where = stream_key(device)[:2]
        return [obj for key, obj in self.items.items() if key[:2] == where]


def prof_enable(on: bool):
    lib().uoc_prof_reset()
    lib().uoc_prof_enable(1 if on else 0)


def prof_report():
    """Per-kernel-class totals recorded since prof_enable(True): list of dicts."""
    import json
    buf = ctypes.create_string_buffer(1 << 19)
    call("uoc_prof_report", None, buf, len(buf))
    return json.loads(buf.value.decode())
