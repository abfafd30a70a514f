"""The C-ABI library builds, loads, and exports every symbol include/uoc_hip.h declares.
No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

from unseenobjectclustering_amd import _native
from unseenobjectclustering_amd.build import LIB_PATH, build_native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uoc_hip.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(uoc_[a-z0-9_]+)\s*\(", src)))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_prototypes():
    """[(name, return type, [argument types])] of every function the header declares, in its order, as C type strings
    without the argument names."""
    out = []
    for ret, name, args in re.findall(r"^([A-Za-z_][\w \*]*?)\b(uoc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M):
        args = [] if args.strip() == "void" else [re.match(r"(.*?)\w+$", a.strip()).group(1).strip() for a in args.split(",")]
        out.append((name, ret.strip(), args))
    return out


def header_constants():
    """{name: value} of the header's #define and enum constants with an integer value."""
    src, out = header_text(), {}
    pairs = re.findall(r"^#define\s+(UOC_\w+)\s+(.+?)\s*$", src, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", src):
        pairs += [tuple(x.strip() for x in item.split("=")) for item in body.split(",") if "=" in item]
    for name, value in pairs:
        if re.fullmatch(r"[-\d\s()<*+]+", value):
            out[name] = eval(value)
    return out


# C scalar -> the ctypes of the same size and signedness; a pointer of any kind matches any ctypes pointer type
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "long": ctypes.c_long,
           "uint32_t": ctypes.c_uint32, "unsigned long long": ctypes.c_ulonglong}


def matches(c_type, ct):
    if "*" in c_type:
        return ct in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ct, type) and issubclass(ct, ctypes._Pointer))
    return SCALARS[re.sub(r"\bconst\b", "", c_type).strip()] is ct


def abi_mismatches(table):
    protos = header_prototypes()
    bad = [f"{name}: not in the table" for name, _, _ in protos if name not in table]
    for name, ret, args in protos:
        if name not in table:
            continue
        restype, argtypes = table[name]
        if not matches(ret, restype):
            bad.append(f"{name}: returns {ret}, the table says {restype}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments, the table has {len(argtypes)}")
        bad += [f"{name}: argument {i} is {a}, the table says {t}" for i, (a, t) in enumerate(zip(args, argtypes)) if not matches(a, t)]
    return bad


def test_abi_table_matches_every_prototype():
    protos = header_prototypes()
    assert len(protos) >= 87 and sorted(p[0] for p in protos) == declared_symbols()     # the parser misses no declaration
    assert list(_native.ABI) == [p[0] for p in protos]              # the table is in header order, nothing extra
    assert all(restype is not None and isinstance(argtypes, list) for restype, argtypes in _native.ABI.values())
    assert abi_mismatches(_native.ABI) == []
    lib = _native.lib()                                             # and the loaded library carries exactly the table
    for name, (restype, argtypes) in _native.ABI.items():
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def test_abi_check_catches_a_wrong_entry():
    """The comparison itself: a c_int for a size_t, a missing argument and a wrong return type are each reported."""
    I, Z, P = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    ret, args = _native.ABI["uoc_grasp"]
    for name, entry in (("uoc_grasp", (ret, [I if t is Z else t for t in args])), ("uoc_grasp", (ret, args[:-1])),
                        ("uoc_grasp_workspace_bytes", (I, [I] * 4)), ("uoc_ms_check", (I, [I])),
                        ("uoc_support_plane", (ret, [I if t is ctypes.c_uint32 else t for t in _native.ABI["uoc_support_plane"][1]]))):
        bad = abi_mismatches({**_native.ABI, name: entry})
        assert len(bad) == 1 and bad[0].startswith(name + ":"), bad


# module constants of _native that are no mirror of a header constant
NOT_MIRRORED = {"ROI_TABLE_BYTES", "OBJECT_BYTES", "GRAPHS_ALIVE"}


def test_mirrored_constants_equal_the_header():
    """Every upper-case integer of _native is the header's UOC_<name>, value for value."""
    consts = header_constants()
    mirrored = {k: v for k, v in vars(_native).items() if k.isupper() and type(v) is int and k not in NOT_MIRRORED}
    assert len(mirrored) >= 50
    for name, value in mirrored.items():
        assert "UOC_" + name in consts, f"_native.{name} has no UOC_{name} in include/uoc_hip.h"
        assert consts["UOC_" + name] == value, f"_native.{name} = {value}, the header says {consts['UOC_' + name]}"
    assert _native.METRICS == {"cosine": consts["UOC_METRIC_COSINE"], "euclidean": consts["UOC_METRIC_EUCLIDEAN"]}
    assert _native.CC_MODES == {"all": consts["UOC_CC_ALL"], "largest": consts["UOC_CC_LARGEST"]}


def test_struct_mirrors_have_the_header_sizes():
    """ctypes.sizeof of every struct mirror against the sizeof the header's static_assert states."""
    sizes = {n: int(v) for n, v in re.findall(r"static_assert\(sizeof\((uoc_\w+)\) == (\d+)", header_text())}
    mirrors = {"uoc_roi_table": _native.RoiTable, "uoc_object": _native.UocObject, "uoc_track": _native.UocTrack,
               "uoc_plane": _native.UocPlane, "uoc_plane_object": _native.UocPlaneObject, "uoc_plane_info": _native.UocPlaneInfo,
               "uoc_relation_object": _native.UocRelationObject}
    assert set(sizes) == set(mirrors)
    for name, cls in mirrors.items():
        assert ctypes.sizeof(cls) == sizes[name], name
    assert all(issubclass(v, ctypes.Structure) and v in mirrors.values() for v in vars(_native).values()
               if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure)


def test_library_builds_and_loads():
    path = build_native()
    assert os.path.exists(path)
    lib = _native.lib()
    assert lib.uoc_version() >= 100


def test_every_declared_symbol_is_exported():
    build_native()
    lib = ctypes.CDLL(LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 8
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/uoc_hip.h but not exported by libuoc_hip.so"
    assert set(_native.EXPORTED_SYMBOLS) == set(syms)


def test_argument_validation_without_gpu():
    """Validation errors are reported through the error channel before any HIP call."""
    lib = _native.lib()
    assert lib.uoc_ms_workspace_bytes(1, 307200, 100) > 307200 * 4
    rc = lib.uoc_ms_cluster(None, 1, 100, 100, 20.0, 10, 0.04, None, None, None, None, None, None, 0, None)
    assert rc == -22
    assert b"null" in lib.uoc_last_error().lower()
    rc = lib.uoc_ms_seed_components(None, 1, 1000, 0.04, None, None, None)
    assert rc == -22
    rc = lib.uoc_ms_select_seeds_from(None, 1, 100, 10, 3, None, None, None, None, 0, None)      # continuation entry
    assert rc == -22
    # 128-d entry points: halves in {1, 2}; the 2-plane workspace is larger
    assert lib.uoc_ms_workspace_bytes_wide(1, 50176, 100, 2) > lib.uoc_ms_workspace_bytes_wide(1, 50176, 100, 1) > 0
    assert lib.uoc_ms_workspace_bytes_wide(1, 50176, 100, 1) == lib.uoc_ms_workspace_bytes(1, 50176, 100)
    assert lib.uoc_ms_workspace_bytes_wide(1, 50176, 100, 3) == 0
    rc = lib.uoc_ms_cluster_wide(None, 3, 1, 100, 100, 20.0, 10, 0.04, None, None, None, None, None, None, 0, None)
    assert rc == -22 and b"halves" in lib.uoc_last_error().lower()
    # network handle: unknown mode rejected, embedding width per mode, parameter intake is host-only
    h = ctypes.c_void_p()
    assert lib.uoc_net_create_mode(ctypes.byref(h), 9) == -22
    for mode, dim in ((0, 64), (1, 64), (2, 64), (3, 64), (4, 128)):
        h = ctypes.c_void_p()
        assert lib.uoc_net_create_mode(ctypes.byref(h), mode) == 0
        assert lib.uoc_net_embed_dim(h) == dim
        assert lib.uoc_net_workspace_bytes(h, 1, 480, 640) > 100 << 20
        arr = (ctypes.c_float * 4)(1, 2, 3, 4)
        assert lib.uoc_net_load_param(h, b"fcn.resnet34_8s.fc.bias", arr, 4) == 0
        assert lib.uoc_net_forward(h, None, None, 1, 64, 64, None, None, 0, None) == -22      # not finalized
        assert lib.uoc_net_destroy(h) == 0
    # evaluation and glue entries validate their pointers first
    assert lib.uoc_eval_workspace_bytes(480, 640) >= 2 * 480 * 640 * 4
    assert lib.uoc_eval_pair_stats(None, None, 480, 640, 3, None, None, 0, None) == -22
    assert lib.uoc_roi_crop(None, None, None, 480, 640, None, 1, 224, None, None, None, None) == -22
    # round 6: the device-side match_label_crop and the split-precision switch validate first, too
    assert lib.uoc_roi_match(None, None, None, None, 1, 224, 480, 640, None, None, None, None, None, 0, None) == -22
    assert lib.uoc_net_set_split_precision(None, 1) == -22
    h = ctypes.c_void_p()
    assert lib.uoc_net_create(ctypes.byref(h)) == 0
    assert lib.uoc_net_set_split_precision(h, 1) == -22            # not finalized
    assert lib.uoc_net_destroy(h) == 0


def test_shipped_library_has_no_result_affecting_knobs():
    """The library reads only the speed-only variables INTEGRATION.md lists, and its configuration fingerprint does not move with
    the rounding-affecting knobs the development builds of rounds 3-5 had (there is no development build any more)."""
    lib = _native.lib()
    assert lib.uoc_is_dev_build() == 0
    blob = open(LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"UOC_[A-Z0-9_]{3,}\x00", blob))
    names = {n.rstrip("\x00") for n in names}
    assert names <= {"UOC_CONV_AUTOTUNE", "UOC_CONV_TUNE_CACHE", "UOC_CONV_VERBOSE", "UOC_FPS_PERSISTENT", "UOC_SPLIT_MAX_MB", "UOC_HC_PARTS"}, names
    fp = _native.config_fingerprint()
    assert fp != 0
    old = {k: os.environ.get(k) for k in ("UOC_WINOGRAD_F", "UOC_HC_QUAD", "UOC_WINOGRAD_MIN_CIN")}
    try:
        os.environ.update(UOC_WINOGRAD_F="2", UOC_HC_QUAD="0", UOC_WINOGRAD_MIN_CIN="0")
        lib.uoc_reload_env()
        assert _native.config_fingerprint() == fp
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        lib.uoc_reload_env()
    # the explicit-algorithm conv entry validates before any HIP call
    assert lib.uoc_conv2d_nhwc_algo(None, None, None, None, None, 1, 1, 8, 8, 32, 64, 5, 1, 1, 1, 0, 0, None) == -22


def test_conv_tile_entries_validate_without_gpu():
    """The tile lists and the static model are host arithmetic; the single-tile entry and the stand-alone stem / pooling / head
    entries refuse bad arguments before any HIP call."""
    lib = _native.lib()
    lists = {}
    for algo, n in ((_native.CONV_DIRECT, 14), (_native.CONV_WINOGRAD4, 8), (_native.CONV_WINOGRAD4_BF16X3, 6)):
        assert lib.uoc_conv2d_tile_list(algo, None, 0) == n
        buf = (ctypes.c_int32 * (2 * n))()
        assert lib.uoc_conv2d_tile_list(algo, buf, n) == n
        lists[algo] = [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]
        assert len(set(lists[algo])) == n
        short = (ctypes.c_int32 * 4)(-1, -1, -1, -1)                  # a short array is filled as far as it goes, no further
        assert lib.uoc_conv2d_tile_list(algo, short, 1) == n and (short[0], short[1]) == lists[algo][0] and short[2] == -1
    assert lib.uoc_conv2d_tile_list(1, None, 0) == -22
    assert set(c for c, _ in lists[_native.CONV_DIRECT]) == {0, 1, 2, 3}
    assert set(c for c, _ in lists[_native.CONV_WINOGRAD4]) == {64, 128}
    cfg, bm, fam = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_int32 * 4)()
    # the fc layer at 480x640: Cout = 64 admits the two 64-wide families only
    assert lib.uoc_conv2d_tile_choice(2, 1, 60, 80, 512, 64, 1, 1, 1, _native.CONV_DIRECT, ctypes.byref(cfg), ctypes.byref(bm), fam) == 0
    assert (cfg.value, bm.value) in lists[_native.CONV_DIRECT] and fam[0] == fam[1] == 0 and fam[cfg.value] == bm.value
    assert all((i, fam[i]) in lists[_native.CONV_DIRECT] for i in (2, 3))
    assert lib.uoc_conv2d_tile_choice(2, 1, 60, 80, 256, 256, 3, 1, 2, _native.CONV_WINOGRAD4, ctypes.byref(cfg), ctypes.byref(bm), None) == 0
    assert (cfg.value, bm.value) in lists[_native.CONV_WINOGRAD4]
    assert lib.uoc_conv2d_tile_choice(2, 1, 60, 80, 256, 256, 3, 2, 1, _native.CONV_WINOGRAD4, ctypes.byref(cfg), ctypes.byref(bm), None) == -22
    assert lib.uoc_conv2d_tile_choice(2, 1, 60, 80, 48, 64, 3, 1, 1, _native.CONV_DIRECT, ctypes.byref(cfg), ctypes.byref(bm), None) == -22
    one = ctypes.c_void_p(16)                                            # never dereferenced: every call below is refused first
    tile = lambda algo, Cout, c, b: lib.uoc_conv2d_nhwc_tile(one, one, None, None, one, 1, 1, 8, 8, 32, Cout, 3, 1, 1, 1, 0, algo, None, c, b)
    assert tile(_native.CONV_DIRECT, 128, 0, 64) == -22 and b"no tile" in lib.uoc_last_error().lower()
    assert tile(_native.CONV_DIRECT, 64, 0, 96) == -22                  # Cout = 64 under a 128-wide family
    assert tile(_native.CONV_WINOGRAD4, 128, 128, 80) == -22
    assert tile(_native.CONV_WINOGRAD4, 64, 128, 96) == -22
    assert tile(_native.CONV_WINOGRAD4_BF16X3, 128, 128, 192) == -22
    assert lib.uoc_conv2d_nhwc_tile(None, None, None, None, None, 1, 1, 8, 8, 32, 64, 3, 1, 1, 1, 0, 0, None, 3, 64) == -22
    assert lib.uoc_net_stem(None, None, None, None, 1, 1, 8, 8, 1, None, None) == -22
    assert lib.uoc_maxpool3x3s2_nhwc(None, None, 1, 8, 8, 64, None) == -22
    assert lib.uoc_maxpool3x3s2_nhwc(one, ctypes.c_void_p(32), 1, 8, 8, 6, None) == -22      # C % 4 != 0
    assert lib.uoc_head(None, None, None, 1, 1, 1, 8, 8, 0, None) == -22
    assert lib.uoc_head(one, None, one, 1, 1, 1, 8, 8, 1, None) == -22                       # cat needs both branches


def test_product_path_refuses_cpu_tensors():
    import torch
    from unseenobjectclustering_amd.utils.mean_shift import mean_shift_smart_init
    X = torch.nn.functional.normalize(torch.randn(128, 64), dim=1)
    with pytest.raises(_native.NativeError):
        mean_shift_smart_init(X, 20.0)
