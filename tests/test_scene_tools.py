"""Where users meet the scene memory: the opt-in --memory AGE of tools/export_objects.py on top of --placement.  The
argument wiring, the arrays the tool adds and the drop mask it builds from --motion are checked on the CPU (the tool's
own functions on results built from the reference); the command line on the GPU (the stage has no CPU path):
tests/test_scene_gpu.py holds the stage against the reference."""
import numpy as np
import pytest
import torch

from tests import scene_reference as R
from tests.tool_cases import demo_frames, demo_sample, run_tool, tool  # noqa: F401  (tool is a fixture)

MEMORY_KEYS = {"memory_state", "memory_owner", "memory_age", "memory_change", "memory_ids", "memory_info"}


def test_memory_arguments_and_arrays(tool):
    from unseenobjectclustering_amd import motion, scene
    base = ["--imgdir", "frames", "--out", "objs"]
    assert tool.parse_args(base).memory is None and tool.parse_args(base + ["--placement", "0.05"]).memory is None
    a = tool.parse_args(base + ["--placement", "0.05", "--memory", "12", "--grid", "128"])
    assert (a.memory, a.grid, a.placement) == (12, 128, 0.05)
    assert tool.parse_args(base + ["--placement", "0.05", "--memory", "0"]).memory == 0
    for bad in (["--memory", "5"], ["--placement", "0.05", "--memory", "-1"], ["--placement", "0.05", "--memory", "32768"],
                ["--placement", "0.05", "--memory"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert set(tool.MEMORY_KEYS) == MEMORY_KEYS
    frames = R.hand_sequences()["change_codes"][0]
    st = R.new_state(1, 8)
    for s, o, _, rec in frames[:2]:
        out = R.step(st, s[None], o[None], rec[None], None, 5, 1)
    res = scene.SceneResult(**{k: torch.from_numpy(v) for k, v in out.items()})
    rec = tool.memory_arrays(res)
    assert set(rec) == MEMORY_KEYS and all(v.dtype == np.int32 for v in rec.values())
    assert [rec[k].shape for k in sorted(MEMORY_KEYS)] == [(8, 8), (8, 8), (128, 8), (8,), (8, 8), (8, 8)]
    assert rec["memory_info"].tolist() == [1, 2, 58, 2, 0, 3, 1, 2] and rec["memory_change"][1, :4].tolist() == [2, 0, 3, 3]
    assert rec["memory_ids"][3].tolist() == [6, 1, 1, 1, 1, 0, 2, 0] and rec["memory_age"][0, 4] == 1
    # the ids --motion reports as moved become the drop mask, on whatever device the result lives
    best = np.zeros((1, 3, 16), np.int32)
    best[0, 0, :5], best[0, 0, 12:15] = (1, 0, 0, 0, 0), (0, 0, 0)             # stayed
    best[0, 1, :5], best[0, 1, 12:15] = (1, 0, 0, 0, 3), (2, 0, 40)            # two cells of 10 mm
    best[0, 2, :2] = (2, -1)                                                  # not evaluated
    moved = motion.MotionResult(best=torch.from_numpy(best), angles=32, cell_mm=10, pairs=np.array([[4, 4], [31, 31], [90, 90]], np.int32))
    mask = tool.moved_ids_mask(moved, torch.device("cpu"))
    assert mask.shape == (1, 128) and mask.dtype == torch.bool and torch.nonzero(mask[0]).flatten().tolist() == [31]
    assert not bool(tool.moved_ids_mask(None, torch.device("cpu")).any())
    assert np.array_equal(scene._pack_drop(mask, 1, torch.device("cpu")).numpy(), scene.drop_mask([31], 1))


@pytest.mark.gpu
def test_export_objects_memory_cli(device, golden_dir, tmp_path):
    frames = demo_frames(golden_dir, tmp_path / "frames")        # the demo frame twice
    r = run_tool(frames, tmp_path / "bad", "--max-points", "500", "--memory", "5")
    assert r.returncode != 0 and "--memory needs --placement" in r.stderr
    for out, extra in (("plain", []), ("mem", ["--memory", "5"])):
        r = run_tool(frames, tmp_path / out, "--max-points", "500", "--placement", "0.05", "--grid", "128", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
    from unseenobjectclustering_amd import placement, support
    xyz = demo_sample(golden_dir)["depth"][0].to(device)
    fitted, ref = None, R.new_state(1, 128)
    for t, stem in enumerate(("000002", "000003")):
        plain, mem = np.load(tmp_path / "plain" / f"{stem}_objects.npz"), np.load(tmp_path / "mem" / f"{stem}_objects.npz")
        assert not MEMORY_KEYS & set(plain.files) and set(mem.files) == set(plain.files) | MEMORY_KEYS
        for k in plain.files:                                      # without the option, and beside it: what the tool wrote before
            assert plain[k].dtype == mem[k].dtype and plain[k].tobytes() == mem[k].tobytes(), k
        # the stage on the exported label map, in the plane of the first frame as the tool keeps it, against the reference
        labels = torch.from_numpy(mem["label_map"]).to(device)
        fitted = support.fit_plane(labels, xyz) if fitted is None else fitted
        placed = placement.free_space(labels, xyz, fitted, grid=128)
        want = R.step(ref, placed.state.cpu().numpy(), placed.owner.cpu().numpy(), placed.frame.cpu().numpy(), None, 5, 1)
        for k in ("state", "owner", "age", "change", "ids", "info"):
            assert mem["memory_" + k].dtype == np.int32 and np.array_equal(mem["memory_" + k], want[k][0]), (stem, k)
        assert mem["memory_info"][:2].tolist() == [1, t + 1] and mem["memory_state"].shape == (128, 128)
        if t == 0:
            assert np.array_equal(mem["memory_state"], mem["place_state"]) and not mem["memory_change"].any()
            assert np.array_equal(mem["memory_age"], np.where(mem["place_state"] != 0, 0, -1)) and mem["memory_info"][2] > 100
