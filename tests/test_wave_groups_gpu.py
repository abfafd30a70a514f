"""The wave-group loop (for_each_wave_key, csrc/common.h) and the id rule (csrc/labelmap.h) at the shapes where they can go
wrong, for the stages that read a label map, each against its own reference under tests/ as in its own GPU file:

  5 x 13    65 pixels: a whole wave, then a wave with one active lane whose ballot's first group is lane 0 alone
            (tracking takes its one-pixel-per-lane path here: 65 is no multiple of 4)
  2 x 64    a wave with 64 distinct keys (ids 1..64, or 127 in place of 64) and a wave with none: the second row holds
            only 0, -1, 128, 129, INT_MIN and INT_MAX.  For the confidence summary label 0 is a row, so that wave has one key
  4 x 64    tracking's int4 path with the label changing every pixel: a lane's four pixels are four different pairs
  96 x 96   relations: 9216 pixels are two pair blocks of 8192, and the pixel of raster index 8191 differs from its right
            and lower neighbours, which belong to the second block

Integer results are compared with np.array_equal, objects' float statistics by that file's own bounds."""
import faulthandler
import sys

import numpy as np
import pytest
import torch

from tests import components_reference as CR
from tests import confidence_reference as FR
from tests import relations_reference as RR
from tests.test_objects_gpu import check_against_reference
from tests.test_tracking_gpu import assert_state, run_reference
from unseenobjectclustering_amd import components, relations, tracking
from unseenobjectclustering_amd import confidence as CF
from unseenobjectclustering_amd import objects as O

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
OUTSIDE = np.array([0, -1, 128, 129, I32.min, I32.max], np.int32)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def wave_and_a_lane():
    """[5,13]: ids 3 and 9 in the first 64 pixels, an out-of-range value among them, and pixel 64 the only one of id 77."""
    lab = np.where(np.arange(65) % 5 < 3, 3, 9).astype(np.int32)
    lab[[7, 30]] = [128, -1]
    lab[64] = 77
    return lab.reshape(5, 13)


def sixty_four_keys(top):
    """[2,64]: ids 1..63 and `top` in the first row, nothing but OUTSIDE in the second."""
    lab = np.stack([np.arange(1, 65, dtype=np.int32), OUTSIDE[np.arange(64) % 6]])
    lab[0, 63] = top
    return lab


MAPS = {"5x13": wave_and_a_lane(), "2x64": sixty_four_keys(64), "2x64_127": sixty_four_keys(127)}


def depth(lab, seed=5):
    """A valid, slowly varying z with steps between the ids, a few invalid values: [H,W] float32."""
    rng = np.random.default_rng(seed)
    ids = np.where((lab >= 1) & (lab < 128), lab, 0)
    z = (0.8 + 0.013 * (ids % 7) + 0.0005 * rng.standard_normal(lab.shape)).astype(np.float32)
    z.reshape(-1)[::17] = [0.0, np.nan, -1.0, np.inf][seed % 4]
    return z


def dev(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def test_the_maps_are_what_they_claim():
    flat = MAPS["5x13"].reshape(-1)
    assert flat.size == 65 and (flat[:64] != 77).all() and flat[64] == 77
    for name, top in (("2x64", 64), ("2x64_127", 127)):
        m = MAPS[name]
        assert len(set(m[0].tolist())) == 64 and m[0].min() == 1 and m[0].max() == top
        assert set(m[1].tolist()) == set(OUTSIDE.tolist()) and not ((m[1] >= 1) & (m[1] <= 127)).any()


@pytest.mark.parametrize("name", list(MAPS))
def test_objects(device, name):
    lab = MAPS[name][None]
    z = depth(lab[0])
    xyz = RR.xyz_of(z)[None]
    objs = O.extract_objects(dev(device, lab), dev(device, xyz), min_points=0)
    K, _ = check_against_reference(objs, lab, xyz)
    assert K == len(np.unique(lab[(lab >= 1) & (lab <= 127)]))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(MAPS))
def test_relations(device, name, conn):
    lab = MAPS[name]
    xyz = RR.xyz_of(depth(lab))
    for gap_mm, min_pairs in ((15, 1), (5, 2)):
        res = relations.relate(dev(device, lab), dev(device, xyz), connectivity=conn, gap=gap_mm / 1000.0, min_pairs=min_pairs)
        want = RR.relations(lab, xyz[2], conn, gap_mm, min_pairs)
        for k in RR.TABLES + RR.FIELDS:
            assert np.array_equal(getattr(res, k)[0].cpu().numpy(), want[k]), (name, conn, gap_mm, k)
    if name != "5x13":
        assert want["pixels"][1:64].tolist() == [1] * 63 and want["pixels"][0] == 0


@pytest.mark.parametrize("conn", [4, 8])
def test_relations_across_a_chunk_end(device, conn):
    lab = np.ones((96, 96), np.int32)
    lab[85, :32] = 2                                    # raster index 8191 = (85, 31) is the last pixel of id 2 in its row
    lab[86:, 40:] = 3
    flat = lab.reshape(-1)
    assert flat[8191] == 2 and flat[8192] == 1 and flat[8191 + 96] == 1 and flat[8191 + 97] == 1 and 96 * 96 > 8192
    z = (0.9 - 0.02 * (lab == 2) + 0.03 * (lab == 3)).astype(np.float32)
    z[85, 31] = 0.86                                    # the pixel at the chunk's end is in front by 40 mm
    xyz = RR.xyz_of(z)
    for gap_mm, min_pairs in ((15, 1), (30, 1), (50, 4)):
        res = relations.relate(dev(device, lab), dev(device, xyz), connectivity=conn, gap=gap_mm / 1000.0, min_pairs=min_pairs)
        want = RR.relations(lab, xyz[2], conn, gap_mm, min_pairs)
        for k in RR.TABLES + RR.FIELDS:
            assert np.array_equal(getattr(res, k)[0].cpu().numpy(), want[k]), (conn, gap_mm, k)
    assert want["border"][1, 2] == 32 + 32 + 1 + (126 if conn == 8 else 0)     # above, below, the right end; the diagonals


@pytest.mark.parametrize("name", list(MAPS))
def test_confidence(device, name):
    lab = MAPS[name][None]
    rng = np.random.default_rng(11)
    conf = rng.random(lab.shape).astype(np.float32)
    conf.reshape(-1)[::9] = [1.5, np.nan, -0.25, 0.0, 1.0, 0.01][len(name) % 6]
    for weak_q in (0, 1311, 65535):
        stats = CF.object_stats(dev(device, lab), dev(device, conf), weak_q)
        want = FR.objects(lab, conf, weak_q)
        assert np.array_equal(stats.cpu().numpy(), want), (name, weak_q)
    zeros = int((lab == 0).sum())
    assert want[0, 0, 0] == zeros and (zeros > 0) == (name != "5x13")           # label 0 is a row of this table
    assert want[0, :, 0].sum() == int(((lab >= 0) & (lab <= 127)).sum())         # and nothing else out of range is


@pytest.mark.parametrize("name", list(MAPS))
def test_components(device, name):
    lab = MAPS[name][None]
    for conn in (4, 8):
        for mode in ("all", "largest"):
            for min_area in (1, 2):
                out, table, counts = components.split_components(dev(device, lab), connectivity=conn, min_area=min_area, mode=mode)
                want = CR.split_batch(lab, conn, min_area, mode)
                for got, w in zip((out, table, counts), want):
                    assert np.array_equal(got.cpu().numpy(), w), (name, conn, mode, min_area)


def sequence(name):
    """Three steps of one stream: the map, its ids shifted, the map again with two ids swapped."""
    lab = MAPS[name]
    ids = (lab >= 1) & (lab <= 127)
    moved = np.where(ids, lab % 127 + 1, lab).astype(np.int32)
    swapped = np.where(lab == 3, 9, np.where(lab == 9, 3, lab)).astype(np.int32)
    return np.stack([lab, np.roll(moved, 1, axis=1), swapped])


def every_pixel_another_label():
    """[3,4,64]: the label changes from pixel to pixel, and from step to step against the memory map, so the four pixels
    of a lane's int4 hold four different (memory, label) pairs."""
    i = np.arange(256, dtype=np.int64).reshape(4, 64)
    frames = np.stack([i % 127 + 1, (i * 3 + 5) % 127 + 1, (i * 7 + 11) % 126 + 1]).astype(np.int32)
    frames[1, 2, 5:9] = OUTSIDE[:4]
    return frames


@pytest.mark.parametrize("name", list(MAPS) + ["4x64"])
def test_tracking(device, name):
    frames = every_pixel_another_label() if name == "4x64" else sequence(name)
    n = frames[0].size
    assert (n % 4 == 0) == (name != "5x13")                                   # 5x13: one pixel per lane; the others: int4
    if name == "4x64":
        quads = frames.reshape(3, -1, 4)
        assert all(len(set(q.tolist())) == 4 for q in quads[0]) and all(len(set(q.tolist())) >= 3 for q in quads[1])
    for min_iou, max_age in ((0.1, 2), (0.5, 0)):
        steps, _ = run_reference(frames, min_iou, max_age)
        tr = tracking.Tracker(min_iou=min_iou, max_age=max_age)
        for t in range(frames.shape[0]):
            d = dev(device, frames[t])
            assert d.data_ptr() % 16 == 0
            out = tr.update(d)
            assert np.array_equal(out.cpu().numpy(), steps[t][0].astype(np.int32)), (name, min_iou, t)
            assert_state(tr, steps[t], 0, (name, min_iou, t))
