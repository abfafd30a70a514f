"""Where users meet the multi-plane stage: the opt-in --planes of tools/export_objects.py and planes=True of
objects.segment_objects.  The argument wiring and the arrays the tool adds are checked on the CPU (the tool's own
planes_arrays and the helpers of support.py on a synthetic result); the command line and segment_objects on the GPU (the
stage has no CPU path): tests/test_planes_gpu.py holds the stage against the reference."""
import types

import numpy as np
import pytest
import torch

from tests import planes_reference as P
from tests.tool_cases import BASE_KEYS, demo_sample, export, tool  # noqa: F401  (tool is a fixture)

PLANES_KEYS = {"plane_count", "plane_normal", "plane_d", "plane_inliers", "plane_cos0", "plane_offset0", "plane_extent",
               "plane_index", "stands_on", "plane_support"}


def synthetic(K=3):
    """A one-frame PlanesResult look-alike on the CPU: the table (plane 0), a wall, a board 0.25 above the table; id 5 on
    the table, id 9 on the board, id 7 below everything."""
    normal = torch.tensor([[[0.0, -0.8, -0.6], [1.0, 0.0, 0.0], [0.0, -0.8, -0.6]]])
    hm = torch.zeros(1, K, 128)
    cnt = torch.zeros(1, K, 128, dtype=torch.int32)
    for l, h0 in ((5, 0.05), (9, 0.30), (7, -0.10)):
        cnt[0, :, l] = 10
        hm[0, 0, l], hm[0, 1, l], hm[0, 2, l] = h0, 0.4, h0 - 0.25
    return types.SimpleNamespace(
        count=torch.tensor([K], dtype=torch.int32), normal=normal, d=torch.tensor([[0.55, 0.3, 0.30]]),
        inliers=torch.tensor([[500, 200, 100]], dtype=torch.int32), cos0=torch.tensor([[1.0, 0.0, 1.0]]),
        offset0=torch.tensor([[0.0, 0.1, 0.25]]), extent=torch.arange(12, dtype=torch.float32).reshape(1, K, 4),
        index=torch.full((1, 4, 6), -2, dtype=torch.int32), records=torch.zeros(1, K, 21, dtype=torch.int32),
        height_min=hm, obj_count=cnt)


def test_planes_arguments_and_arrays(tool):
    from unseenobjectclustering_amd import support
    base = ["--imgdir", "frames", "--out", "objs"]
    assert tool.parse_args(base).planes is None and tool.parse_args(base).planes_up is None
    assert tool.parse_args(base + ["--planes", "4"]).planes == 4
    args = tool.parse_args(base + ["--planes", "8", "--planes-up", "0", "-1", "0", "--placement", "0.05", "--normals"])
    assert args.planes == 8 and args.planes_up == [0.0, -1.0, 0.0]
    for bad in (["--planes", "0"], ["--planes", "9"], ["--planes"], ["--planes-up", "0", "-1", "0"], ["--planes", "2", "--plane"],
                ["--planes", "2", "--planes-up", "0", "0", "0"], ["--planes", "2", "--planes-up", "1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    syn = synthetic()
    assert support.planes_like(syn, 0)[0].tolist() == [True, False, True]
    assert support.planes_like(syn, (1.0, 0.0, 0.0))[0].tolist() == [False, True, False]
    on = support.standing_on(syn)[0]
    assert on.dtype == torch.int64 and on[5] == 0 and on[9] == 2 and on[7] == -1 and int((on >= 0).sum()) == 2
    assert support.standing_on(syn, (2.0, 0.0, 0.0))[0][[5, 9, 7]].tolist() == [1, 1, 1]
    assert support.choose_support(syn).tolist() == [0] and support.choose_support(syn, up=(0.0, -4.0, -3.0)).tolist() == [0]
    syn.obj_count[0, :, 5] = 0                                     # only id 9 stands on anything: the board wins
    assert support.choose_support(syn).tolist() == [2]
    syn.count[0] = 2                                               # ... unless it was not found
    assert support.choose_support(syn).tolist() == [0] and support.planes_like(syn, 0)[0].tolist() == [True, False, False]
    syn = synthetic()
    rec = tool.planes_arrays(syn, torch.tensor([9, 5, 7]))
    assert set(rec) == PLANES_KEYS == set(tool.PLANES_KEYS.values()) | {"stands_on", "plane_support"}
    assert rec["stands_on"].tolist() == [2, 0, -1] and int(rec["plane_support"]) == 0 and int(rec["plane_count"]) == 3
    assert rec["plane_normal"].shape == (3, 3) and rec["plane_extent"].shape == (3, 4) and rec["plane_index"].shape == (4, 6)
    assert rec["plane_inliers"].tolist() == [500, 200, 100] and rec["plane_index"].dtype == np.int32
    assert tool.planes_arrays(syn, torch.tensor([9, 5, 7]), up=[1.0, 0.0, 0.0])["stands_on"].tolist() == [1, 1, 1]
    assert tool.planes_arrays(syn, torch.zeros(0, dtype=torch.int64))["stands_on"].shape == (0,)


def _demo(golden_dir):
    from unseenobjectclustering_amd import networks, synth
    sample = demo_sample(golden_dir)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    return sample, networks.seg_resnet34_8s_embedding(2, 64, sd).eval(), networks.seg_resnet34_8s_embedding(2, 64, sd).eval()


@pytest.mark.gpu
def test_segment_objects_with_planes_end_to_end(device, golden_dir):
    from unseenobjectclustering_amd import objects as O, placement, support
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sample, net, net_crop = _demo(golden_dir)
    np.random.seed(3)
    out0, ref0, objs0, fit0, placed0 = O.segment_objects(sample, net, net_crop, placement=True)
    np.random.seed(3)
    out1, ref1, objs1, fit1, placed1, several = O.segment_objects(sample, net, net_crop, placement=True, planes=True,
                                                                   planes_args=dict(max_planes=3, up=None))
    assert torch.equal(out0, out1) and torch.equal(ref0, ref1) and torch.equal(objs0.centroid, objs1.centroid)
    assert isinstance(several, support.PlanesResult) and several.records.shape == (1, 3, 21)
    lab, xyz = ref1[0].numpy().astype(np.int32), sample["depth"][0].numpy()
    H, W = lab.shape
    want = P.fit(lab, xyz, 3, 256, 10, 20, P.default_min_inliers(H, W), 1)
    assert int(several.count[0]) == want["count"] >= 1 and np.array_equal(several.index[0].cpu().numpy(), want["index"])
    k = P.choose_support(want)
    assert torch.equal(fit1.records, several.records[:, k]) and fit1.height is None
    assert torch.equal(several.records[:, 0], fit0.records)                      # plane 0 is fit_plane's plane
    again = placement.free_space(torch.from_numpy(lab).to(device), sample["depth"][:1].to(device), several.plane(k))
    assert torch.equal(placed1.state, again.state) and torch.equal(placed1.dist2, again.dist2)
    if k == 0:
        assert torch.equal(placed1.state, placed0.state) and torch.equal(placed1.owner, placed0.owner)
    np.random.seed(3)
    only = O.segment_objects(sample, net, net_crop, planes=True, planes_args=dict(max_planes=2))
    assert len(only) == 4 and torch.equal(only[3].records[:, 0], fit0.records)


@pytest.mark.gpu
def test_export_objects_planes_cli(device, golden_dir, tmp_path):
    z = export(golden_dir, tmp_path / "planes", "--planes", "4", "--planes-up", "0", "-1", "-1", "--placement", "0.05")
    assert BASE_KEYS | PLANES_KEYS <= set(z.files) and "place_state" in z.files and "plane_found" not in z.files
    K = len(z["label"])
    H, W = z["label_map"].shape
    assert z["plane_normal"].shape == (4, 3) and z["plane_extent"].shape == (4, 4) and z["plane_index"].shape == (H, W)
    assert z["stands_on"].shape == (K,) and z["plane_index"].dtype == np.int32
    xyz = _demo(golden_dir)[0]["depth"][0].numpy()
    want = P.fit(z["label_map"], xyz, 4, 256, 10, 20, P.default_min_inliers(H, W), 1)
    assert int(z["plane_count"]) == want["count"] >= 1 and np.array_equal(z["plane_index"], want["index"])
    assert z["plane_inliers"].tolist() == [p["inliers"] for p in want["planes"]]
    up = (0.0, -1.0, -1.0)
    assert z["stands_on"].tolist() == [P.standing_on(want, up)[int(l)] for l in z["label"]]
    assert int(z["plane_support"]) == P.choose_support(want, up=up)
