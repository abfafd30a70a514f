"""The network's CPU references (tests/network_reference.py) checked on the CPU: the layer-wise evaluation has the network's
structure and fold, the hostile BatchNorm weights are usable and make a wrong eps visible, and the stored yardsticks of
tests/test_network_fp64_gpu.py are what the emulation gives.  No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import conv_reference as CR
from tests import network_reference as NR

STRUCTURE_CASES = [f"{m} 9x15 B=2" for m in NR.MODES] + ["RGBD_ADD 8x8 B=1", "RGBD_ADD 37x53 B=2"]


@functools.lru_cache(maxsize=None)
def layerwise_fp64_error(name):
    sd, img, depth, ref = NR.case_reference(name)
    assert ref.dtype == torch.float64
    return CR.max_err(NR.layerwise(sd, img, depth, NR.CASES[name]["mode"], torch.float64), ref)


@pytest.mark.parametrize("name", STRUCTURE_CASES)
def test_layerwise_fp64_equals_oracle_fp64(name):
    """Fold in double, Winograd algebra in double, two-pass early stem, buffer-free layer table: the same function as the
    oracle's unfolded BatchNorm network, up to fp64 rounding."""
    err = layerwise_fp64_error(name)
    print(f"{name}: |layer-wise fp64 - oracle fp64| {err:.3e}")
    assert err < 1e-12


@pytest.mark.parametrize("name", NR.HOSTILE_CASES)
def test_hostile_bn_reference_is_usable(name):
    sd, img, depth, ref = NR.case_reference(name)
    assert torch.isfinite(ref).all()
    assert (ref.norm(dim=1) - 1).abs().max().item() < 1e-12
    assert layerwise_fp64_error(name) < 1e-12
    assert 0 < NR.stored_yardstick(name) < 1e-5


def test_hostile_bn_touches_every_batchnorm():
    base = NR.state_dict("RGBD_ADD")
    sd = NR.hostile_bn(base, NR.WSEED)
    assert set(sd) == set(base) and all(sd[k].dtype == base[k].dtype and sd[k].shape == base[k].shape for k in base)
    seen = set()
    for key in (k for k in sd if k.endswith(".running_var")):
        pfx = key[:-len("running_var")]
        changed = np.flatnonzero(sd[key] != base[key])
        C = sd[key].shape[0]
        assert C // 7 <= len(changed) <= C // 7 + 1, (key, len(changed))
        assert set(np.unique(sd[key][changed]).tolist()) <= set(np.float32(NR.HOSTILE_VARS).tolist())
        seen |= set(sd[key][changed].tolist())
        scale = sd[pfx + "weight"].astype(np.float64) / np.sqrt(sd[key].astype(np.float64) + 1e-5)
        assert np.abs(scale).max() < 2.2, key                    # the folded scale stays O(1): untouched channels 1.5 / sqrt(0.5)
        assert np.abs(scale[changed]).max() < 1.5 + 1e-6, key    # ... and the hostile ones |g0| < 1.5
        assert np.allclose(np.abs(scale[changed]), base[pfx + "weight"][changed], rtol=1e-6)
        assert (scale[changed] < 0).any() or C < 128
        assert (sd[pfx + "weight"] == 0).sum() >= 1
        assert 1.0 < np.abs(sd[pfx + "running_mean"][changed]).max() <= 3.0
        assert all(np.array_equal(sd[pfx + s], base[pfx + s]) for s in ("bias", "num_batches_tracked"))
    assert seen == set(np.float32(NR.HOSTILE_VARS).tolist())
    assert all(np.array_equal(sd[k], base[k]) for k in sd if sd[k].ndim == 4 or k.endswith("fc.bias"))


@pytest.mark.parametrize("name", NR.HOSTILE_CASES)
def test_eps_slip_is_more_than_100_yardsticks_away(name):
    """The oracle in fp64 with BN_EPS = 1e-3 instead of 1e-5 on the hostile weights: the embedding moves by more than
    100 x the case's yardstick, so a bar of 4 yardsticks sees a fold with that eps."""
    sd, img, depth, ref = NR.case_reference(name)
    moved = CR.max_err(NR.reference(sd, img, depth, NR.CASES[name]["mode"], eps=NR.EPS_SLIP), ref)
    yard = NR.stored_yardstick(name)
    print(f"{name}: eps 1e-3 moves the reference by {moved:.3e} = {moved / yard:.0f} yardsticks")
    assert moved > 100 * yard
    assert NR.BO.BN_EPS == 1e-5                                  # the experiment leaves the oracle as it was


def test_every_gpu_case_has_a_stored_yardstick():
    assert set(NR._stored()) == set(NR.CASES)
    for name in NR.CASES:
        assert 0 < NR.stored_yardstick(name) < 1e-5, name


@pytest.mark.parametrize("name", ["RGBD_ADD 8x8 B=1", "RGBD_ADD 16x8 B=1"])
def test_stored_yardsticks_agree_with_recomputation(name):
    """The two smallest cases, recomputed: within 1 % of tests/golden/network_yardsticks.json."""
    got, stored = NR.case_yardstick(name), NR.stored_yardstick(name)
    print(f"{name}: recomputed {got:.6e}, stored {stored:.6e}")
    assert abs(got - stored) <= 0.01 * stored


def test_winograd_rule_on_the_backbone():
    """Every 3x3 stride-1 layer of ResNet34 from 64 channels up, and no other: not the strided layer2.0.conv1, no 1x1."""
    from tests.backbone_layers import backbone_layers
    layers = backbone_layers(37, 53)
    wino = [l for l in layers if NR.runs_winograd(l[2], l[3], l[4], l[5])]
    assert len(layers) == 36 and len(wino) == 31
    assert all(K == 3 and s == 1 for (_, _, _, _, K, s, _) in wino)
    assert [l for l in layers if l[4] == 3 and l not in wino] == [(10, 14, 64, 128, 3, 2, 1)]
    assert not NR.runs_winograd(32, 64, 3, 1) and not NR.runs_winograd(64, 192, 3, 1) and not NR.runs_winograd(80, 64, 3, 1)
