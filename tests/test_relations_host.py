"""The numpy restatement of uoc_relations (tests/relations_reference.py) against hand-counted tables on frames of at
most 4x4, the generated scenes against what the GPU tests use them for, and the wrapper's argument checks.  No GPU."""
import numpy as np
import pytest

from tests import relations_reference as R


def table(entries):
    t = np.zeros((128, 128), np.int32)
    for (a, b), v in entries.items():
        t[a, b] = v
    return t


def sym(entries):
    return table({**entries, **{(b, a): v for (a, b), v in entries.items()}})


def test_hand_counted_2x2():
    # 1 2      depths 1.000 1.010      pairs (4): 1-2 touch (10 mm), 1-3 1 in front (200 mm), 2-0 border only (hole),
    # 3 0             1.200 0.000                 3-0 border only
    lab = np.array([[1, 2], [3, 0]])
    z = np.array([[1.0, 1.01], [1.2, 0.0]], np.float32)
    r = R.relations(lab, z, 4, 15, 1)
    assert np.array_equal(r["border"], sym({(1, 2): 1, (1, 3): 1, (0, 2): 1, (0, 3): 1}))
    assert np.array_equal(r["touch"], sym({(1, 2): 1}))
    assert np.array_equal(r["front"], table({(1, 3): 1}))
    assert r["pixels"][:4].tolist() == [0, 1, 1, 1] and r["edge"][:4].tolist() == [0, 1, 1, 1]
    assert r["border_sum"][:4].tolist() == [0, 2, 2, 2] and r["border_bg"][:4].tolist() == [0, 0, 1, 1]
    assert r["n_touch"][:4].tolist() == [0, 1, 1, 0] and r["n_above"][:4].tolist() == [0, 0, 0, 1]
    assert r["n_below"][:4].tolist() == [0, 1, 0, 0] and r["layer"][:4].tolist() == [0, 1, 1, 2]
    assert r["order"][:4].tolist() == [0, 1, 2, 3] and not r["free"].any()           # every pixel of a 2x2 frame is on the edge
    # connectivity 8 adds the diagonals 1-0 (hole: border only) and 2-3 (2 in front by 190 mm)
    r8 = R.relations(lab, z, 8, 15, 1)
    assert np.array_equal(r8["border"], sym({(1, 2): 1, (1, 3): 1, (0, 2): 1, (0, 3): 1, (0, 1): 1, (2, 3): 1}))
    assert np.array_equal(r8["touch"], sym({(1, 2): 1})) and np.array_equal(r8["front"], table({(1, 3): 1, (2, 3): 1}))
    assert r8["n_above"][3] == 2 and r8["layer"][:4].tolist() == [0, 1, 1, 2]
    # with min_pairs = 2 nothing is a relation any more; the tables do not change
    r2 = R.relations(lab, z, 8, 15, 2)
    assert np.array_equal(r2["front"], r8["front"]) and not r2["n_above"].any() and not r2["n_touch"].any()
    assert r2["layer"][:4].tolist() == [0, 1, 1, 1]


def test_hand_counted_4x4_with_background_in_front():
    # 0 0 0 0     the background ring is at 0.5 m, id 9 at 1.0 m.  Connectivity 4: each of the four pixels of the block
    # 0 9 9 0     has two background neighbours, 8 pairs, all front[0][9].  Connectivity 8: each has five background
    # 0 9 9 0     neighbours, three of them diagonal, 8 + 12 pairs.
    # 0 0 0 0
    lab = np.zeros((4, 4), int)
    lab[1:3, 1:3] = 9
    z = np.where(lab == 9, 1.0, 0.5).astype(np.float32)
    r = R.relations(lab, z, 4, 15, 8)
    assert np.array_equal(r["front"], table({(0, 9): 8})) and np.array_equal(r["border"], sym({(0, 9): 8}))
    assert not r["touch"].any()
    assert r["pixels"][9] == 4 and r["edge"][9] == 0 and r["hidden"][9] == 8 and r["border_bg"][9] == 8 and r["border_sum"][9] == 8
    assert r["n_above"][9] == 0 and r["layer"][9] == 1 and r["free"][9] == 0 and r["order"][9] == 1       # hidden >= min_pairs
    assert R.relations(lab, z, 4, 15, 9)["free"][9] == 1
    assert R.relations(lab, z, 8, 15, 8)["front"][0, 9] == 20


def test_depth_quantisation_and_label_rule():
    above = np.nextafter(np.float32(65.0), np.float32(np.inf))
    z = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, 65.0, above, 1e-9, 0.0625, 0.1875, 1.25, 1.2344], np.float32)   # 62.5 and 187.5 are ties
    assert R.depth_mm(z).tolist() == [-1, -1, -1, -1, -1, 65000, -1, 0, 62, 188, 1250, 1234]
    assert R.ids_of(np.array([0, 1, 127, 128, -1, 1000, 255])).tolist() == [0, 1, 127, 0, 0, 0, 0]


@pytest.mark.parametrize("H,W", [(24, 32), (61, 83), (97, 131), (224, 224), (480, 640)])
@pytest.mark.parametrize("seed", [1, 2])
def test_tabletop_scenes_contain_what_they_are_used_for(H, W, seed):
    lab, xyz = R.tabletop(H, W, seed)
    assert lab.dtype == np.int32 and xyz.dtype == np.float32 and xyz.shape == (3, H, W)
    holes = float((xyz[2] == 0).mean())
    assert 0.02 <= holes <= 0.09
    r = R.relations(lab, xyz[2], 8, 15, 4)
    occ = R.occlusion_matrix(r["front"].astype(np.int64), 4)
    assert occ[2, 1] and not occ[1, 2]                                       # the ellipse is painted over the rectangle
    assert r["touch"][3, 4] >= 4 and not occ[3, 4] and not occ[4, 3]         # side by side at one depth
    assert r["edge"][5] > 0 and r["free"][5] == 0                            # cut by the image edge
    assert r["layer"].max() >= 2 and r["free"].sum() >= 1
    assert (r["border_sum"] >= r["border_bg"]).all() and r["border"].sum() > r["touch"].sum() + r["front"].sum()   # holes


def test_engineered_cases_are_what_their_names_say():
    def run(name, **kw):
        c = R.ENGINEERED[name]()
        args = dict(connectivity=c["connectivity"], gap_mm=c["gap_mm"], min_pairs=c["min_pairs"])
        args.update(kw)
        return c, R.relations(c["lab"], c["xyz"][2], **args)

    for name in ("one_by_one", "one_id"):
        c, r = run(name)
        assert not r["border"].any() and r["layer"].max() == 1 and r["order"].max() == 1
    for name in ("pair_h", "pair_v"):
        c, r = run(name)
        assert r["border"].sum() == 2 and r["front"].sum() == 1 and sorted(r["layer"][1:3].tolist()) == [1, 2]
    _, r = run("chain5")
    assert r["layer"][1:6].tolist() == [1, 2, 3, 4, 5] and r["order"][1:6].tolist() == [1, 2, 3, 4, 5]
    assert r["free"][1:6].tolist() == [0, 0, 0, 0, 0] and r["n_below"][1:6].tolist() == [1, 1, 1, 1, 0]
    _, r = run("cycle")
    assert r["layer"][1:5].tolist() == [-1, -1, -1, -1] and r["n_above"][1:5].tolist() == [1, 1, 1, 1]
    assert r["front"][1, 2] == r["front"][2, 3] == r["front"][3, 1] == r["front"][1, 4] == 10
    _, r = run("tie")
    assert r["front"][1, 2] == r["front"][2, 1] == 4 and r["n_above"].sum() == 0 and r["layer"][1:3].tolist() == [1, 1]
    _, r = run("at_min_pairs")
    assert r["front"][1, 2] == 5 and r["front"][3, 4] == 4 and r["n_above"][2] == 1 and r["n_above"][4] == 0
    assert r["touch"][5, 6] == 5 and r["touch"][7, 8] == 4 and r["n_touch"][5:9].tolist() == [1, 1, 0, 0]
    _, r = run("at_gap")
    assert r["front"][1, 2] == 4 and r["touch"][1, 2] == 0 and r["touch"][3, 4] == 4 and r["front"][3, 4] == r["front"][4, 3] == 0
    c, r = run("bad_depth")
    assert r["border"][1, 2] > r["touch"][1, 2] + r["front"][1, 2] + r["front"][2, 1] > 0
    assert (R.depth_mm(c["xyz"][2]) == 65000).sum() == 2 and (R.depth_mm(c["xyz"][2]) == 0).sum() == 2
    c, r = run("bad_labels")
    assert r["pixels"].sum() == 4 + 3 and set(np.nonzero(r["border"])[0]) == {0, 1, 127}
    _, r = run("stripes127")
    assert r["layer"][1:].tolist() == list(range(1, 128)) and r["order"][1:].tolist() == list(range(1, 128))
    _, r = run("checkerboard")
    assert r["front"][1, 2] == r["border"][1, 2] == 2 * 16 * 15 and r["front"][2, 1] == 0
    lab, xyz = R.row_stripes(6, 5)
    assert R.relations(lab, xyz[2], 8, 15, 1)["front"][1, 2] == 5 * 5 + 2 * 5 * 4


def test_wrapper_argument_checks_need_no_gpu():
    import torch
    from unseenobjectclustering_amd import _native, relations
    lab, xyz = torch.zeros((4, 4), dtype=torch.int32), torch.ones((3, 4, 4))
    for bad in (dict(connectivity=6), dict(gap=0.0), dict(gap=65.6), dict(min_pairs=0)):
        with pytest.raises(ValueError):
            relations.relate(lab, xyz, **bad)
    with pytest.raises(_native.NativeError):
        relations.relate(lab, xyz)                                           # host tensors: there is no CPU fallback
    assert relations.OBJECT_FIELDS[0] == "pixels" and len(relations.OBJECT_FIELDS) == 11
    assert "uoc_relations" in _native.EXPORTED_SYMBOLS and "uoc_relations_workspace_bytes" in _native.EXPORTED_SYMBOLS

    class Fake:
        min_pairs = 2
        order = torch.tensor([[0, 3, 0, 1, 2]])
        front = torch.zeros((1, 5, 5), dtype=torch.int32)
        touch = torch.zeros((1, 5, 5), dtype=torch.int32)

    Fake.front[0, 3, 1], Fake.front[0, 4, 1], Fake.front[0, 1, 4], Fake.touch[0, 1, 3] = 2, 3, 3, 2
    assert relations.pick_order(Fake) == [3, 4, 1]
    assert relations.occluders(Fake, 0, 1) == [3] and relations.neighbours(Fake, 0, 1) == [3] and relations.neighbours(Fake, 0, 4) == []
