"""Where users meet the motion stage: the opt-in --motion / --motion-angles / --motion-radius of tools/export_objects.py on
top of --track.  The argument wiring and the arrays the tool adds are checked on the CPU (the tool's own motion_arrays on a
result built from the reference); the command line on the GPU (the stage has no CPU path): tests/test_motion_gpu.py holds
the stage against the reference end to end."""
import numpy as np
import pytest
import torch

from tests import motion_reference as R
from tests.tool_cases import demo_frames, demo_sample, run_tool, tool  # noqa: F401  (tool is a fixture)

MOTION_KEYS = {"motion_ids", "motion_best", "motion_T"}


def test_motion_arguments_and_arrays(tool):
    from unseenobjectclustering_amd import motion, placement
    base = ["--imgdir", "frames", "--out", "objs"]
    a = tool.parse_args(base)
    assert a.motion is False and (a.motion_angles, a.motion_radius) == (32, 8)
    a = tool.parse_args(base + ["--track", "--motion", "--motion-angles", "64", "--motion-radius", "16", "--grid", "128"])
    assert a.motion and a.track and (a.motion_angles, a.motion_radius, a.grid) == (64, 16, 128)
    for bad in (["--motion"], ["--reid", "--motion"], ["--track", "--motion", "--motion-angles", "65"], ["--track", "--motion", "--motion-angles", "0"],
                ["--track", "--motion", "--motion-radius", "17"], ["--track", "--motion", "--motion-radius", "-1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert set(tool.MOTION_KEYS) == MOTION_KEYS
    ga, gb = R.l_pair(16, (4, 5), move=(2, -1), turn=1, a=5)
    pairs = [(5, 5), (9, 9)]
    out = R.motion(ga[0], ga[1], gb[0], gb[1], R.rotation_table(8), 2, pairs)
    planes = placement.pack_planes([0, 0, -1], 1.0, [0, 0, 1.0], [1, 0, 0], [0, -1, 0])
    res = motion.MotionResult(rot=torch.from_numpy(out["rot"][None]), best=torch.from_numpy(out["best"][None]), table=R.rotation_table(8),
                              pairs=np.array(pairs, np.int32), angles=8, radius=2, grid=16, cell_mm=10, planes=planes)
    rec = tool.motion_arrays(res)
    assert set(rec) == MOTION_KEYS and rec["motion_ids"].tolist() == [5, 9] and rec["motion_ids"].dtype == np.int32
    assert rec["motion_best"].shape == (2, 16) and rec["motion_best"].dtype == np.int32 and rec["motion_best"][:, 0].tolist() == [1, 2]
    assert rec["motion_best"][0, [1, 4]].tolist() == [2, 0]                       # a quarter turn of eight steps, every cell met
    T = rec["motion_T"]
    assert T.shape == (2, 4, 4) and T.dtype == np.float64 and np.isnan(T[1]).all()
    # u = x, v = -y, n = -z: a quarter turn from u towards v, about the pivot cell
    assert np.allclose(T[0][:3, :3], [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-9)
    f = dict(zip(R.BEST_FIELDS, rec["motion_best"][0].tolist()))
    pa = np.array([(f["pi"] + 0.5 - 8) * 0.01, -(f["pj"] + 0.5 - 8) * 0.01, 1.0])
    pb = np.array([(f["qi"] + f["si"] + 0.5 - 8) * 0.01, -(f["qj"] + f["sj"] + 0.5 - 8) * 0.01, 1.0])
    assert np.allclose(T[0] @ np.append(pa, 1.0), np.append(pb, 1.0), atol=1e-9)
    empty = tool.motion_arrays(None)
    assert set(empty) == MOTION_KEYS and [empty[k].shape for k in ("motion_ids", "motion_best", "motion_T")] == [(0,), (0, 16), (0, 4, 4)]


@pytest.mark.gpu
def test_export_objects_motion_cli(device, golden_dir, tmp_path):
    frames = demo_frames(golden_dir, tmp_path / "frames")        # the demo frame twice: nothing moves
    r = run_tool(frames, tmp_path / "out", "--max-points", "500", "--motion")
    assert r.returncode != 0 and "--motion needs --track" in r.stderr
    r = run_tool(frames, tmp_path / "out", "--max-points", "500", "--track", "--motion", "--motion-angles", "16", "--motion-radius", "4")
    assert r.returncode == 0, r.stdout + r.stderr
    first, second = np.load(tmp_path / "out" / "000002_objects.npz"), np.load(tmp_path / "out" / "000003_objects.npz")
    assert not MOTION_KEYS & set(first.files) and MOTION_KEYS <= set(second.files)
    ids, best, T = second["motion_ids"], second["motion_best"], second["motion_T"]
    assert len(ids) >= 1 and best.shape == (len(ids), 16) and T.shape == (len(ids), 4, 4)
    assert set(ids.tolist()) <= set(np.unique(first["label_map"]).tolist()) & set(np.unique(second["label_map"]).tolist())
    # the stage on the two exported label maps, with the tool's settings, against the reference
    import json
    from unseenobjectclustering_amd import motion, placement, support
    xyz = demo_sample(golden_dir)["depth"][0].to(device)
    la, lb = (torch.from_numpy(z["label_map"]).to(device) for z in (first, second))
    fitted = support.fit_plane(la, xyz)
    pa, pb = placement.free_space(la, xyz, fitted), placement.free_space(lb, xyz, fitted)
    grids = [getattr(p, k)[0].cpu().numpy() for p in (pa, pb) for k in ("state", "owner")]
    want = R.motion(*grids, R.rotation_table(16), 4, [(int(a), int(a)) for a in ids], pa.frame[0].cpu().numpy(), pb.frame[0].cpu().numpy())
    assert np.array_equal(best, want["best"])
    assert (best[:, 0] == 1).any()
    for p in np.nonzero(best[:, 0] == 1)[0]:
        assert np.allclose(T[p][3], [0, 0, 0, 1]) and abs(np.linalg.det(T[p][:3, :3]) - 1) < 1e-9
