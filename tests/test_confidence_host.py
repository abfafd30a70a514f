"""Label confidence without a GPU: every UOC_EINVAL of the three entries through ctypes (validation comes before any device
work, so fabricated pointers are never dereferenced), the Python wrappers' refusals, and the fp64 reference of the GPU
tests against the oracle's own margin (oracle/margins.py) and against hand-made cases."""
import ctypes

import numpy as np
import pytest
import torch

from tests import confidence_reference as R
from unseenobjectclustering_amd import _native, confidence as CF

EINVAL = -22
P = lambda a: ctypes.c_void_p(a)      # a fabricated, 16-byte aligned device address: rejected calls never touch it
X, Z, SL, NU, LAB, MAR, SEC, CLO, RIV, WS = (P(0x10000000 * (i + 1)) for i in range(10))


def err():
    return _native.lib().uoc_last_error().decode()


def conf_call(**kw):
    a = dict(X=X, halves=1, batch=1, n=1000, Z=Z, sl=SL, nu=NU, m=100, metric=0, labels=LAB, margin=MAR, second=SEC, closest=CLO,
             rival=RIV, ws=WS, ws_bytes=None)
    a.update(kw)
    L = _native.lib()
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(L.uoc_ms_confidence_workspace_bytes(max(a["batch"], 1), 1000, 100, 1), 512)
    return L.uoc_ms_confidence(a["X"], a["halves"], a["batch"], a["n"], a["Z"], a["sl"], a["nu"], a["m"], a["metric"], a["labels"],
                               a["margin"], a["second"], a["closest"], a["rival"], a["ws"], a["ws_bytes"], None)


def test_workspace_bytes():
    L = _native.lib()
    assert L.uoc_ms_confidence_workspace_bytes(1, 307200, 100, 1) >= 128 * 4
    assert L.uoc_ms_confidence_workspace_bytes(7, 50176, 100, 2) >= 7 * 128 * 4
    for bad in ((0, 100, 10, 1), (65536, 100, 10, 1), (1, 0, 10, 1), (1, (1 << 30) + 1, 10, 1), (1, 100, 0, 1), (1, 100, 129, 1),
                (1, 100, 10, 0), (1, 100, 10, 3)):
        assert L.uoc_ms_confidence_workspace_bytes(*bad) == 0, bad


@pytest.mark.parametrize("kw,word", [
    (dict(X=None), "d_X is null"), (dict(Z=None), "d_Z is null"), (dict(sl=None), "d_seed_labels is null"),
    (dict(nu=None), "d_num_unique is null"), (dict(labels=None), "d_labels is null"), (dict(margin=None), "d_margin is null"),
    (dict(ws=None), "d_ws is null"),
    (dict(halves=0), "halves"), (dict(halves=3), "halves"), (dict(batch=0), "batch"), (dict(batch=65536), "batch"),
    (dict(n=0), "n = 0"), (dict(n=(1 << 30) + 1), "n = "), (dict(m=0), "m = 0"), (dict(m=129), "m = 129"),
    (dict(metric=1), "not built"), (dict(metric=2), "metric = 2"), (dict(metric=-1), "metric = -1"),
    (dict(X=P(0x10000004)), "d_X is not 16-byte aligned"), (dict(Z=P(0x20000008)), "d_Z is not 16-byte aligned"),
    (dict(ws_bytes=511), "workspace"), (dict(ws=P(0xA0000008)), "workspace not 16-byte aligned"),
    (dict(labels=X), "d_labels aliases the input d_X"), (dict(labels=P(0x10000000 + 4000)), "d_labels aliases the input d_X"),
    (dict(labels=Z), "d_labels aliases the input d_Z"), (dict(labels=SL), "d_labels aliases the input d_seed_labels"),
    (dict(labels=NU), "d_labels aliases the input d_num_unique"), (dict(margin=X), "d_margin aliases the input d_X"),
    (dict(second=SL), "d_second aliases the input d_seed_labels"), (dict(closest=Z), "d_closest aliases the input d_Z"),
    (dict(rival=X), "d_rival aliases the input d_X"), (dict(margin=LAB), "d_labels overlaps d_margin"),
    (dict(rival=P(0x50000000 + 3996)), "d_labels overlaps d_rival"),
])
def test_ms_confidence_rejects(kw, word):
    assert conf_call(**kw) == EINVAL
    assert word in err(), err()


def test_ms_confidence_euclidean_message():
    assert conf_call(metric=_native.METRIC_EUCLIDEAN) == EINVAL
    assert "euclidean" in err() and "not built" in err()


@pytest.mark.parametrize("kw,word", [
    (dict(values=None), "d_values_crop is null"), (dict(labels=None), "d_labels_crop is null"), (dict(table=None), "d_table is null"),
    (dict(plan=None), "d_plan is null"), (dict(out=None), "d_out is null"), (dict(K=0), "K = 0"), (dict(K=128), "K = 128"),
    (dict(S=0), "S = 0"), (dict(S=4097), "S = 4097"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"),
    (dict(H=65536, W=65536), "bad shape"), (dict(out=X), "d_out aliases d_values_crop"),
    (dict(out=P(0x10000000 + 1000)), "d_out aliases d_values_crop"),          # a partial overlap, not the same pointer
    (dict(out=P(0x10000000 - 4096)), "d_out aliases d_values_crop"),          # d_out [H*W] runs into the values from below
    (dict(out=Z), "d_out aliases d_labels_crop"), (dict(out=P(0x20000000 + 602108)), "d_out aliases d_labels_crop"),
    (dict(out=SL), "d_out aliases d_table"), (dict(out=NU), "d_out aliases d_plan"),
    (dict(out=P(0x40000000 - 100)), "d_out aliases d_plan"),
])
def test_conf_paste_rejects(kw, word):
    a = dict(values=X, labels=Z, table=SL, plan=NU, K=3, S=224, H=480, W=640, out=LAB)
    a.update(kw)
    rc = _native.lib().uoc_conf_paste(a["values"], a["labels"], a["table"], a["plan"], a["K"], a["S"], a["H"], a["W"], a["out"], None)
    assert rc == EINVAL and word in err(), err()


@pytest.mark.parametrize("kw,word", [
    (dict(labels=None), "d_labels is null"), (dict(conf=None), "d_conf is null"), (dict(stats=None), "d_stats is null"),
    (dict(B=0), "B = 0"), (dict(B=65536), "B = 65536"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"),
    (dict(H=1 << 16, W=(1 << 14) + 1), "bad shape"), (dict(weak_q=-1), "weak_q = -1"), (dict(weak_q=65536), "weak_q = 65536"),
    (dict(stats=P(0x30000004)), "d_stats is not 8-byte aligned"),
])
def test_conf_objects_rejects(kw, word):
    a = dict(labels=X, conf=Z, B=2, H=37, W=53, weak_q=1311, stats=SL)
    a.update(kw)
    rc = _native.lib().uoc_conf_objects(a["labels"], a["conf"], a["B"], a["H"], a["W"], a["weak_q"], a["stats"], None)
    assert rc == EINVAL and word in err(), err()


def test_segment_confidence_refuses_the_euclidean_opt_in():
    """test_sample follows cfg.TRAIN.EMBEDDING_METRIC; no margin is built for the euclidean metric, so the two-stage entry
    refuses instead of segmenting the frame with another metric: before any RNG draw, before any device is looked for."""
    from unseenobjectclustering_amd.fcn.config import cfg
    sample = dict(image_color=torch.zeros(1, 3, 8, 8), depth=torch.zeros(1, 3, 8, 8))
    boom = lambda *a: (_ for _ in ()).throw(AssertionError("the network must not run"))      # noqa: E731
    old = cfg.TRAIN.EMBEDDING_METRIC
    try:
        cfg.TRAIN.EMBEDDING_METRIC = "euclidean"
        np.random.seed(3)
        before = np.random.get_state()[1].copy()
        with pytest.raises(NotImplementedError, match="cosine"):
            CF.segment_confidence(sample, boom, boom)
        assert np.array_equal(np.random.get_state()[1], before)
    finally:
        cfg.TRAIN.EMBEDDING_METRIC = old


def test_wrappers_refuse_host_tensors_and_bad_thresholds():
    Xc = torch.nn.functional.normalize(torch.randn(1, 32, 64), dim=2)
    with pytest.raises(_native.NativeError):
        CF.assign_confidence(Xc, Xc[:, :4], torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(_native.NativeError):
        CF.summarize(torch.zeros((4, 4), dtype=torch.int32), torch.zeros((4, 4)))
    assert CF.weak_to_q(0.0) == 0 and CF.weak_to_q(0.02) == 1311 and CF.weak_to_q(1.0) == 65535 and CF.weak_to_q(0.5) == 32768
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            CF.weak_to_q(bad)


def test_reference_margin_is_the_oracles():
    """The fp64 restatement against oracle/margins.py::assign_margins (torch, float32 inputs upcast) on a field with three seed
    labels, and its tie rules on a hand-made case."""
    from oracle import margins as MG
    rng = np.random.default_rng(5)
    Xn = rng.standard_normal((300, 64))
    Xn /= np.linalg.norm(Xn, axis=1, keepdims=True)
    Zn = rng.standard_normal((12, 64))
    Zn /= np.linalg.norm(Zn, axis=1, keepdims=True)
    sl = rng.integers(0, 3, size=12)
    sl[:3] = [0, 1, 2]
    got = R.assign(Xn, Zn, sl)
    want = MG.assign_margins(torch.from_numpy(Xn), torch.from_numpy(Zn), torch.from_numpy(sl)).numpy()
    assert np.abs(got["margin"] - want).max() <= 2.0 ** -25        # the oracle computes in fp64 here but stores float32: half an ulp below 1
    assert (got["margin"] >= 0).all() and (got["rival"] >= 0).all()
    assert (sl[got["rival"]] != sl[got["closest"]]).all()
    # ties: two seeds at the same place -> the lowest index wins both as best and as rival; the swap puts the largest label on 0
    e = np.eye(64)
    Zt = np.stack([e[0], e[0], e[1], e[1]])
    r = R.assign(np.stack([e[0], e[1], e[1], (e[0] + e[1]) / np.sqrt(2)]), Zt, [0, 0, 1, 1])
    assert r["closest"].tolist() == [0, 2, 2, 0] and r["rival"].tolist() == [2, 0, 0, 2]
    assert r["labels"].tolist() == [0, 1, 1, 0] and r["second"].tolist() == [1, 0, 0, 1]      # 2 : 2, the first maximum is 0: no swap
    assert r["margin"][3] == 0.0 and abs(r["margin"][0] - 0.5) < 1e-15
    r = R.assign(np.stack([e[1], e[1], e[0]]), Zt, [0, 0, 1, 1])
    assert r["labels"].tolist() == [0, 0, 1] and r["second"].tolist() == [1, 1, 0]           # label 1 is the largest: swapped
    one = R.assign(Xn[:5], Zn, np.full(12, 4))
    assert (one["margin"] == 1.0).all() and (one["rival"] == -1).all() and (one["second"] == -1).all()
    assert (one["labels"] == 4).all()       # num_unique = 1 counts label 0 only: nothing to swap


def test_reference_quantise_and_objects():
    c = np.array([np.nan, -1.0, -0.0, 0.0, 2.0 ** -17, 1 - 2.0 ** -17, 1.0, 7.5, np.inf, 0.02], np.float32)
    assert R.quantise(c).tolist() == [0, 0, 0, 0, 0, 65535, 65535, 65535, 65535, 1310]
    lab = np.array([[[1, 1, 1, 0, 128, -3, 127, 127, 5, 1]]])
    st = R.objects(lab, c[None, None], 1311)
    assert st[0, 1].tolist() == [4, 1310, 0, 4] and st[0, 127].tolist() == [2, 131070, 65535, 0]
    assert st[0, 0].tolist() == [1, 0, 0, 1] and st[0, 5].tolist() == [1, 65535, 65535, 0] and st[0, 2].tolist() == [0, 0, 0, 0]


def test_reference_paste_follows_the_order():
    S, H, W = 4, 6, 8
    labels_crop = np.zeros((2, S * S), np.int32)
    labels_crop[0, :] = 1
    labels_crop[1, :8] = 2          # the upper half of crop 1 is kept, the lower half is id 0 -> not mapped
    boxes = np.array([[0, 0, 5, 4], [2, 1, 7, 5]])
    idmap = np.zeros((2, 128), np.int32)
    idmap[0, 1], idmap[1, 2] = 1, 2
    plan = np.concatenate([[0, 1], idmap.reshape(-1)])
    vals = np.stack([np.full(S * S, 0.25, np.float32), np.arange(S * S, dtype=np.float32)])
    out = R.paste(vals, labels_crop, boxes, plan, 2, S, H, W, np.full((H, W), np.nan, np.float32))
    _, _, ident = R.paste_source(labels_crop, boxes, plan, 2, S, H, W)
    assert ident[0, 0] == 1 and ident[1, 2] == 2 and ident[4, 2] == 1 and ident[5, 7] == 0 and ident[5, 0] == 0
    assert np.array_equal(np.isnan(out), ident == 0)
    assert out[0, 0] == 0.25 and out[1, 2] == 0.0 and out[2, 7] == 3.0      # crop 1 paints over crop 0 where it keeps pixels
    plan_rev = np.concatenate([[1, 0], idmap.reshape(-1)])
    out_rev = R.paste(vals, labels_crop, boxes, plan_rev, 2, S, H, W, np.zeros((H, W), np.float32))
    assert out_rev[1, 2] == 0.25 and out_rev[2, 7] == 3.0
