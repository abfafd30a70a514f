"""GPU parity of the evaluation kernels (uoc_eval_pair_stats through utils/evaluation.py): every integer table
bit-exact against the CPU oracle, the overlap metrics equal to the reference's goldens, and test_segnet's
metric bookkeeping."""
import os

import numpy as np
import pytest
import torch

from oracle import evaluation_oracle as EO
from tests import evaluation_cases as EC
from tests import evaluation_reference as ER
from tests.golden.cases import EVAL_CASES, eval_pair
from unseenobjectclustering_amd import synth
from unseenobjectclustering_amd.fcn import test_dataset as TD
from unseenobjectclustering_amd.fcn.config import cfg
from unseenobjectclustering_amd.utils import evaluation as EV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_tables_match_oracle(device, name):
    pred, gt = eval_pair(EVAL_CASES[name])
    got = EV.pair_stats(torch.from_numpy(pred).to(device), gt)          # device tensor and numpy both accepted
    want = EO.pair_tables(pred, gt)
    for k in ("cont", "bnd_pred", "bnd_gt", "prec_tp", "rec_tp"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", list(EC.CASES))
def test_engineered_cases_match_reference(device, name):
    """tests/evaluation_cases.py (what each case contains: tests/test_evaluation_cases_host.py): labels from 64 up, four
    labels in one 2x2 neighbourhood, radii 0..32, maps of one row / column / pixel, one table cell hit by every pixel."""
    pred, gt, bound_th = EC.CASES[name]()
    want = ER.pair_tables(pred, gt, ER.radius_of(pred.shape, bound_th))
    got = EV.pair_stats(torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device), bound_th=bound_th)
    for k in ("cont", "bnd_pred", "bnd_gt", "prec_tp", "rec_tp"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_metrics_match_reference_golden(device, golden_dir, name):
    g = np.load(os.path.join(golden_dir, "evaluation.npz"))
    pred, gt = eval_pair(EVAL_CASES[name])
    m = EV.multilabel_metrics(pred.astype(np.float32), gt)               # float label maps like test_segnet passes
    for k, w in zip([str(k) for k in g["metrics/keys"]], g[f"metrics/{name}"]):
        assert float(m[k]) == w, (k, float(m[k]), w)
    o = EV.metrics_from_tables(EO.pair_tables(pred, gt))
    for k in ("Boundary F-measure", "Boundary Precision", "Boundary Recall"):
        assert float(m[k]) == float(o[k])


def test_border_and_label_range(device):
    """Masks touching every image border (seg2bmap's last-row / last-column rules) and the label-range check."""
    rng = np.random.default_rng(3)
    gt = rng.integers(0, 5, size=(37, 53)).astype(np.int64)
    pred = np.roll(gt, 1, axis=1)
    got, want = EV.pair_stats(pred, gt), EO.pair_tables(pred, gt)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    with pytest.raises(ValueError):
        EV.pair_stats(np.full((8, 8), 200), np.zeros((8, 8)))


def test_test_segnet_reports_metrics(device, tmp_path, capsys):
    """test_segnet with ground-truth labels: per-frame metrics of the stage-1 and the refined maps, averaged."""
    cfg.device = device

    class Loader(list):
        class dataset:
            name = "osd_object_test"

    class Net:
        def __init__(self, field):
            self.field = field

        def eval(self):
            return self

        def __call__(self, img, label, depth):
            return self.field(img.shape[0]).to(device)

    def field(seed, H, W, k):
        X, _ = synth.embedding_field(seed, H, W, 64, k, 0.05)
        return torch.from_numpy(X).view(H, W, 64).permute(2, 0, 1)[None].contiguous()
    samples = Loader()
    for s in (71, 72):
        fr = synth.rgbd_frame(s, 120, 160, 2)
        samples.append(dict(image_color=torch.from_numpy(fr["image_color"]), depth=torch.from_numpy(fr["depth"]),
                            label=torch.from_numpy(fr["label"].astype(np.float32))[None], filename="f%d" % s))
    net = Net(lambda B: field(71, 120, 160, 4))
    crop = Net(lambda B: torch.cat([field(800 + k, 224, 224, 2) for k in range(B)]))
    np.random.seed(3)
    res = TD.test_segnet(samples, net, str(tmp_path), crop)
    assert len(res) == 2 and all("metrics" in r and "metrics_refined" in r for r in res)
    out = capsys.readouterr().out
    assert "Objects F-measure" in out and "Refined" in out
    for r, smp in zip(res, samples):
        gt = smp["label"][0].numpy()
        m = EV.metrics_from_tables(EO.pair_tables(r["labels"], gt))
        assert float(m["Objects F-measure"]) == float(r["metrics"]["Objects F-measure"])
        m = EV.metrics_from_tables(EO.pair_tables(r["labels_refined"], gt))
        assert float(m["Boundary F-measure"]) == float(r["metrics_refined"]["Boundary F-measure"])
