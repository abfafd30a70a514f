"""uoc_cc_split / split_components on the GPU against the plain-integer reference (tests/components_reference.py), bit for
bit: the step has no float arithmetic, so every comparison of out, table and counts is torch.equal / np.array_equal.

The maps are generated in the reference module (seeded) and tests/test_components_host.py asserts on the CPU that they
contain what they are used for here (components across tile borders, more than 127 components, areas at min_area and
one below, an area tie, ids outside 1..127).

Every GPU test runs under a watchdog (faulthandler.dump_traceback_later(..., exit=True)): a hang ends the process instead
of letting later tests start more GPU work; nothing is retried."""
import faulthandler
import functools
import sys

import numpy as np
import pytest
import torch

from tests import components_reference as R
from unseenobjectclustering_amd import _native, components, tracking
from unseenobjectclustering_amd import objects as O

pytestmark = pytest.mark.gpu

SIZES = [(480, 640), (224, 224), (37, 53), (1, 64), (64, 1), (1, 1)]
MIN_AREAS = (1, 2, 50)
MODES = ("all", "largest")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def tabletop(H, W):
    return R.tabletop(1, H, W, frames=2)


@functools.lru_cache(maxsize=None)
def engineered(name, H, W):
    return R.ENGINEERED[name](H, W)


@functools.lru_cache(maxsize=None)
def reference(key, connectivity, min_area, mode):
    """key = ("tabletop", H, W) or (engineered name, H, W): the reference of the whole batch, computed once."""
    maps = tabletop(*key[1:]) if key[0] == "tabletop" else engineered(*key)[None]
    return R.split_batch(maps, connectivity, min_area, mode)


def assert_split(dev_maps, want, connectivity, min_area, mode, where):
    out, table, counts = components.split_components(dev_maps, connectivity=connectivity, min_area=min_area, mode=mode)
    assert out.dtype == table.dtype == counts.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), want[2]), where
    assert np.array_equal(table.cpu().numpy(), want[1]), where
    assert np.array_equal(out.cpu().numpy(), want[0]), where
    return out, table, counts


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SIZES)
def test_tabletop_maps_match_reference(device, H, W, connectivity):
    maps = tabletop(H, W)
    dev_maps = torch.from_numpy(maps).to(device)
    for mode in MODES:
        for min_area in MIN_AREAS:
            want = reference(("tabletop", H, W), connectivity, min_area, mode)
            assert (want[2][:, 0] == want[2][:, 1:].sum(axis=1)).all()
            assert_split(dev_maps, want, connectivity, min_area, mode, (mode, min_area))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", [(37, 53), (224, 224)])
@pytest.mark.parametrize("name", sorted(R.ENGINEERED))
def test_engineered_shapes_match_reference(device, name, H, W, connectivity):
    dev_map = torch.from_numpy(engineered(name, H, W)).to(device)[None]
    for mode in MODES:
        for min_area in MIN_AREAS:
            want = reference((name, H, W), connectivity, min_area, mode)
            assert_split(dev_map, want, connectivity, min_area, mode, (mode, min_area))


@pytest.mark.parametrize("H,W", [(37, 53), (224, 224)])
def test_frames_in_a_batch_equal_frames_alone(device, H, W):
    frames = np.stack([tabletop(H, W)[0], engineered("checkerboard", H, W), engineered("serpentine", H, W),
                       tabletop(H, W)[1], engineered("area_edges", H, W)])
    dev = torch.from_numpy(frames).to(device)
    for connectivity, min_area, mode in ((8, 1, "all"), (4, 1, "all"), (8, 50, "largest"), (4, 2, "largest")):
        out, table, counts = components.split_components(dev, connectivity=connectivity, min_area=min_area, mode=mode)
        assert out.shape == dev.shape and table.shape == (5, 128, 4) and counts.shape == (5, 4)
        for b in range(5):
            o1, t1, c1 = components.split_components(dev[b], connectivity=connectivity, min_area=min_area, mode=mode)
            assert torch.equal(out[b], o1) and torch.equal(table[b], t1[0]) and torch.equal(counts[b], c1[0]), (b, mode)
        want = R.split_batch(frames, connectivity, min_area, mode)
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(table.cpu().numpy(), want[1])
        assert np.array_equal(counts.cpu().numpy(), want[2])


def test_label_dtypes_and_shapes(device):
    img = tabletop(37, 53)[0]
    want = R.split(img, 8, 2, "all")
    base = torch.from_numpy(img).to(device)
    for conv in (lambda x: x, lambda x: x.long(), lambda x: x.float(), lambda x: x[None], lambda x: x[None].float()):
        lab = conv(base)
        out, table, counts = components.split_components(lab, connectivity=8, min_area=2, mode="all")
        assert out.shape == lab.shape and out.dtype == torch.int32
        assert table.shape == (1, 128, 4) and counts.shape == (1, 4)
        assert np.array_equal(out.reshape(37, 53).cpu().numpy(), want[0])
        assert np.array_equal(table[0].cpu().numpy(), want[1]) and np.array_equal(counts[0].cpu().numpy(), want[2])
    odd = base[:, 1:]                                             # a view that is not contiguous: 37x52, rows 53 apart
    out, _, _ = components.split_components(odd, connectivity=4, min_area=1, mode="largest")
    assert np.array_equal(out.cpu().numpy(), R.split(img[:, 1:], 4, 1, "largest")[0])
    with pytest.raises(_native.NativeError):
        components.split_components(base[None, None])
    with pytest.raises(ValueError):
        components.split_components(base, connectivity=6)
    with pytest.raises(ValueError):
        components.split_components(base, min_area=0)
    with pytest.raises(ValueError):
        components.split_components(base, mode="biggest")
    rec = components.component_table(table, counts)
    kept = int(want[2][2])
    assert rec["label"].tolist() == list(range(1, kept + 1)) and rec["kept"] == kept and rec["found"] == int(want[2][0])
    assert np.array_equal(rec["area"], want[1][1:kept + 1, 1]) and np.array_equal(rec["root"], want[1][1:kept + 1, 2])
    assert np.array_equal(rec["src"], want[1][1:kept + 1, 0]) and np.array_equal(rec["siblings"], want[1][1:kept + 1, 3])


def test_composition_with_segmentation_objects_and_tracking(device):
    from unseenobjectclustering_amd import networks, synth
    from unseenobjectclustering_amd.fcn.config import cfg
    cfg.device = device
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.calibrated_state_dict().items()}
    net = networks.seg_resnet34_8s_embedding(2, 64, sd).eval()
    fr = synth.palette_frame(1, 240, 320, 3)
    sample = dict(image_color=torch.from_numpy(fr["image_color"]), depth=torch.from_numpy(fr["depth"]))
    np.random.seed(3)
    out_label, refined, _ = O.segment_objects(sample, net, net, min_points=0)
    final = (refined if refined is not None else out_label)[0].to(device).to(torch.int32)
    xyz = sample["depth"].to(device)
    # CPU: an id of the frame that is one component of at least 50 pixels, and two far-away background pixels with a
    # valid depth to plant its speckle on
    host = final.cpu().numpy()
    z = fr["depth"][0, 2]
    _, comps = R.components(host, 8)
    single = [src for _, area, src in comps if area >= 50 and sum(1 for c in comps if c[2] == src) == 1]
    assert single, "the demo frame has no id that is one component of 50 pixels"
    target = single[0]
    ys, xs = np.nonzero(host == target)
    far = (host == 0) & np.isfinite(z) & (z > 0)
    far[max(ys.min() - 5, 0):ys.max() + 6, max(xs.min() - 5, 0):xs.max() + 6] = False
    cand = np.argwhere(far)
    assert len(cand) >= 2
    speckled = final.clone()
    for y, x in (cand[0], cand[-1]):
        speckled[int(y), int(x)] = target

    def aabb(label_map):
        objs = O.extract_objects(label_map, xyz, min_points=0)
        k = objs.label.cpu().tolist().index(target)
        return objs.aabb_min[k].cpu(), objs.aabb_max[k].cpu(), int(objs.pixels[k])

    clean_min, clean_max, clean_pixels = aabb(final)
    raw_min, raw_max, raw_pixels = aabb(speckled)
    assert raw_pixels == clean_pixels + 2
    assert (raw_max - raw_min > clean_max - clean_min).any()                    # the speckle stretches the raw box
    out, table, counts = components.split_components(speckled, connectivity=8, min_area=50, mode="largest")
    split_min, split_max, split_pixels = aabb(out)
    assert torch.equal(split_min, clean_min) and torch.equal(split_max, clean_max) and split_pixels == clean_pixels
    rec = components.component_table(table, counts)
    k = rec["label"].tolist().index(target)
    assert rec["area"][k] == clean_pixels and rec["siblings"][k] == 3 and rec["src"][k] == target
    want = R.split(speckled.cpu().numpy(), 8, 50, "largest")
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(table[0].cpu().numpy(), want[1])
    # ... and the split map goes on through the tracker
    tr = tracking.Tracker()
    tracked = tr.update(out)
    assert tracked.dtype == torch.int32 and int(tracked.min()) >= 0 and int(tracked.max()) <= 127
    assert torch.equal(tracked > 0, out > 0)
    assert len(tr.tracks()["slot"]) == rec["kept"]
