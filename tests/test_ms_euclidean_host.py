"""The euclidean embedding metric without a GPU: configuration, the float64 restatement against the reference's goldens,
the C ABI of the metric entry points, argument validation and the runner's configuration fingerprint."""
import os
import re
import socket
import ctypes

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ms_euclidean_reference as R
from tests.golden.cases import MEANSHIFT_CASES, WIDE_MEANSHIFT_CASES, KAPPA, EPSILON
from unseenobjectclustering_amd import _native, runner, synth
from unseenobjectclustering_amd.fcn import config as C
from unseenobjectclustering_amd.utils import mean_shift as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {**MEANSHIFT_CASES, **WIDE_MEANSHIFT_CASES}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "meanshift_euclidean.npz"))


def _names(golden):
    return sorted({k.split("/")[0] for k in golden.files})


def _field(name):
    c = CASES[name]
    d = 128 if name.startswith("wide") else 64
    X, _ = synth.embedding_field(c["seed"], c["H"], c["W"], d, c["num_objects"], c["noise"])
    return X, c


def test_euclidean_metric_passes_config_validation(tmp_path):
    saved = C.cfg.TRAIN.EMBEDDING_METRIC
    try:
        C.cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        C.require_supported()
        assert C.euclidean_enabled()
        C.cfg.TRAIN.EMBEDDING_METRIC = "manhattan"
        with pytest.raises(NotImplementedError):
            C.require_supported()
        C.cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        C.cfg.TRAIN.EMBEDDING_NORMALIZATION = False        # still out of scope
        with pytest.raises(NotImplementedError):
            C.require_supported()
    finally:
        C.cfg.TRAIN.EMBEDDING_NORMALIZATION = True
        C.cfg.TRAIN.EMBEDDING_METRIC = saved


def test_a_yml_names_euclidean_only_after_the_opt_in(tmp_path):
    saved = C.cfg.TRAIN.EMBEDDING_METRIC
    y = tmp_path / "euclidean.yml"
    y.write_text("TRAIN:\n  EMBEDDING_METRIC: euclidean\n  EMBEDDING_ALPHA: 0.02\n")
    c = tmp_path / "cosine.yml"
    c.write_text("TRAIN:\n  EMBEDDING_METRIC: cosine\n")
    try:
        C.cfg.TRAIN.EMBEDDING_METRIC = "cosine"
        with pytest.raises(NotImplementedError):       # no opt-in: refused, as before
            C.cfg_from_file(str(y))
        assert C.cfg.TRAIN.EMBEDDING_METRIC == "cosine"
        C.cfg.TRAIN.EMBEDDING_METRIC = "euclidean"      # the program opts in
        C.cfg_from_file(str(y))
        assert C.cfg.TRAIN.EMBEDDING_METRIC == "euclidean"
        C.cfg_from_file(str(c))                         # a cosine yml switches back
        assert C.cfg.TRAIN.EMBEDDING_METRIC == "cosine"
    finally:
        C.cfg.TRAIN.EMBEDDING_METRIC = saved


def test_the_environment_opts_in(tmp_path):
    import subprocess
    import sys
    y = tmp_path / "euclidean.yml"
    y.write_text("TRAIN:\n  EMBEDDING_METRIC: euclidean\n")
    code = ("from unseenobjectclustering_amd.fcn import config as C; C.cfg_from_file(%r); "
            "print(C.cfg.TRAIN.EMBEDDING_METRIC)" % str(y))
    env = dict(os.environ, UOC_EMBEDDING_METRIC="euclidean", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("euclidean"), r.stderr
    env.pop("UOC_EMBEDDING_METRIC")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NotImplementedError" in r.stderr


def test_restatement_reproduces_the_reference_goldens(golden):
    names = _names(golden)
    assert len(names) >= 5 and any(n.startswith("wide") for n in names)
    for name in names:
        X, c = _field(name)
        first = int(golden[name + "/indices"][0])
        labels, idx, Z, sl = R.cluster(X, KAPPA, c["m"], c["iters"], EPSILON, first)
        assert np.array_equal(idx, golden[name + "/indices"]), name
        assert np.abs(Z - golden[name + "/Z"]).max() < 1e-4, name
        assert np.array_equal(sl, golden[name + "/seed_labels"]), name
        assert R.labels_equal_up_to_permutation(labels, golden[name + "/labels"]), name


def _header_decls():
    text = open(os.path.join(ROOT, "include", "uoc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(uoc_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(2)] = [a.strip() for a in m.group(3).split(",") if a.strip() and a.strip() != "void"]
    return out


def _ctype_of(arg: str):
    if "*" in arg:
        return ctypes.c_void_p
    base = arg.rsplit(" ", 1)[0].strip()
    return {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[base]


def test_metric_symbols_match_the_header():
    decls = _header_decls()
    lib = _native.lib()
    assert set(_native.METRIC_SYMBOLS) <= set(decls)
    for name in _native.METRIC_SYMBOLS:
        fn = getattr(lib, name)
        want = [_ctype_of(a) for a in decls[name]]
        assert list(fn.argtypes) == want, name
        assert fn.restype == ctypes.c_int
        assert "int metric" in decls[name], name
    # the cosine calls keep their signatures: the _ex call is the same list with `int metric` inserted
    for old in ("uoc_ms_hill_climb", "uoc_ms_seed_components", "uoc_ms_assign", "uoc_ms_cluster", "uoc_ms_cluster_wide"):
        ex = [a for a in decls[old + "_ex"] if a != "int metric"]
        assert ex == decls[old], old
    assert [a for a in decls["uoc_ms_select_seeds_ex"] if a != "int metric"] == decls["uoc_ms_select_seeds_from"]
    assert _native.METRIC_COSINE == 0 and _native.METRIC_EUCLIDEAN == 1
    h = open(os.path.join(ROOT, "include", "uoc_hip.h")).read()
    assert re.search(r"#define UOC_METRIC_COSINE 0\b", h) and re.search(r"#define UOC_METRIC_EUCLIDEAN 1\b", h)


@pytest.mark.parametrize("metric", [-1, 2, 7])
def test_bad_metric_values_are_rejected_before_anything_runs(metric):
    lib = _native.lib()
    P = None
    calls = {
        "uoc_ms_cluster_ex": lambda: lib.uoc_ms_cluster_ex(P, 1, 100, 100, 20.0, 10, 0.04, metric, P, P, P, P, P, P, 0, P),
        "uoc_ms_cluster_wide_ex": lambda: lib.uoc_ms_cluster_wide_ex(P, 2, 1, 100, 100, 20.0, 10, 0.04, metric, P, P, P, P, P,
                                                                     P, 0, P),
        "uoc_ms_select_seeds_ex": lambda: lib.uoc_ms_select_seeds_ex(P, 1, 100, 10, 0, P, P, P, metric, P, 0, P),
        "uoc_ms_hill_climb_ex": lambda: lib.uoc_ms_hill_climb_ex(P, 1, 100, P, 10, 20.0, 10, metric, P, 0, P),
        "uoc_ms_seed_components_ex": lambda: lib.uoc_ms_seed_components_ex(P, 1, 10, 0.04, metric, P, P, P),
        "uoc_ms_assign_ex": lambda: lib.uoc_ms_assign_ex(P, 1, 100, P, P, P, 10, metric, P, P, P, 0, P),
    }
    for name, call in calls.items():
        assert call() == -22, name
        err = lib.uoc_last_error().decode()
        assert f"metric={metric}" in err, (name, err)     # the metric is checked before the pointers


def test_python_surface_rejects_unknown_metrics():
    X = torch.zeros((1, 16, 64))
    for fn in (lambda: MS.cluster_batch(X, [0], metric="manhattan"),
               lambda: MS.mean_shift_smart_init(X[0], 20, metric="cityblock"),
               lambda: MS.select_smart_seeds(X[0], 4, metric="cos"),
               lambda: MS.seed_hill_climbing_ball(X[0], X[0, :4], 20, metric="l1"),
               lambda: MS.connected_components(X[0, :4], 0.04, metric=None),
               lambda: MS.mean_shift_with_seeds(X[0], X[0, :4], 20, metric="EUCLIDEAN")):
        with pytest.raises(NotImplementedError):
            fn()
    with pytest.raises(NotImplementedError):
        _native.metric_code("sqeuclidean")
    # without the opt-in the reference-surface functions refuse 'euclidean', as they always did
    saved = C.cfg.TRAIN.EMBEDDING_METRIC
    try:
        C.cfg.TRAIN.EMBEDDING_METRIC = "cosine"
        for fn in (lambda: MS.mean_shift_smart_init(X[0], 20, metric="euclidean"),
                   lambda: MS.select_smart_seeds(X[0], 4, metric="euclidean"),
                   lambda: MS.seed_hill_climbing_ball(X[0], X[0, :4], 20, metric="euclidean"),
                   lambda: MS.connected_components(X[0, :4], 0.04, metric="euclidean"),
                   lambda: MS.mean_shift_with_seeds(X[0], X[0, :4], 20, metric="euclidean")):
            with pytest.raises(NotImplementedError, match="opt-in"):
                fn()
    finally:
        C.cfg.TRAIN.EMBEDDING_METRIC = saved
    assert _native.metric_code("euclidean") == 1 and _native.metric_code("cosine") == 0


def test_the_fingerprint_folds_in_the_metric():
    saved = C.cfg.TRAIN.EMBEDDING_METRIC
    try:
        C.cfg.TRAIN.EMBEDDING_METRIC = "cosine"
        cos = runner.config_fingerprint()
        assert cos == _native.config_fingerprint() & 0x7FFFFFFFFFFFFFFF
        C.cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        euc = runner.config_fingerprint()
        assert euc != cos and 0 < euc <= 0x7FFFFFFFFFFFFFFF
        assert euc == runner.config_fingerprint()          # a pure function of the configuration
    finally:
        C.cfg.TRAIN.EMBEDDING_METRIC = saved


def _frame(i):
    return torch.full((6, 8), i % 250, dtype=torch.int32)


def _metric_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    C.cfg.TRAIN.EMBEDDING_METRIC = "euclidean" if rank == 1 else "cosine"
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=60))
    try:
        runner.run_sharded(4, _frame, 6, 8, torch.device("cpu"), rank, world)
        msg = "no error"
    except (RuntimeError, AttributeError) as e:
        msg = f"{type(e).__name__}: {e}"
    open(os.path.join(out_dir, f"r{rank}.txt"), "w").write(msg)
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_with_different_metrics_fail_before_the_gather(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_metric_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert "different libuoc_hip configurations" in open(os.path.join(str(tmp_path), f"r{r}.txt")).read()
