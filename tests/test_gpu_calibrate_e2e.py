"""-m gpu: post-hoc calibration end to end at 64 x 64 on 64 synthetic samples, with the models tests/test_gpu_tta.py builds:
utils.calibrate.calibrate_model -> the sidecar -> utils/tester.py and JointPipeline.

Classifier: logits made over-confident (x 4) get T > 1 and a lower NLL; the tester with the sidecar reports the same accuracy and
confusion matrix and, on the validation loader, the fit's NLL within calibrate_ref.temp_nll_bound.  Segmenter: the Dice the tester
reports at t* is the sweep's mean Dice at t*.  The tester forms 100 * Dice per image and adds them on the host, the sweep adds Dice
and the test multiplies once: each side's mean of n terms <= 1 (<= 100) errs by at most fold_bound(n) (x 100), so they are held to
200 fold_bound(n).  JointPipeline: masks are sigmoid > t*, the confidence is mi355_cls_decide's on the scaled logits; without
``calibration`` every output is the bytes it was."""
import numpy as np
import pytest
import torch

import calibrate_ref as CR
from mi355 import nn as mnn
from mi355.lib import lib
from test_gpu_tester_ci import _loaders
from test_gpu_tta import DEV, _models

pytestmark = pytest.mark.gpu


class Overconfident(torch.nn.Module):
    """the classifier with its logits times four"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x) * 4.0


def _cls_case():
    """(the over-confident classifier, a loader whose labels follow its predictions three times out of four, logits, labels)"""
    cm, _, _ = _models()
    over = Overconfident(cm).eval()
    batches = [b[0] for b in _loaders()[0]]
    with torch.no_grad():
        logits = torch.cat([over(x).float() for x in batches])
    rng = np.random.RandomState(7)
    pred = logits.argmax(1).cpu().numpy()
    labels = np.where(rng.rand(len(pred)) < 0.75, pred, rng.randint(0, 3, len(pred))).astype(np.int64)
    loader = tuple((x, torch.from_numpy(labels[16 * i:16 * i + 16])) for i, x in enumerate(batches))
    return over, loader, logits.cpu().numpy(), labels


def test_classifier_temperature_through_the_tester(tmp_path, capsys):
    from utils import tester
    from utils.calibrate import Calibration, calibrate_model, find_sidecar
    over, loader, logits, labels = _cls_case()
    cal = calibrate_model(over, loader, DEV, seg=False)
    print(cal.describe())
    assert cal.kind == "classification" and cal.samples == 64 and cal.status == 0 and cal.temperature > 1.0 and cal.after <= cal.before
    ok, below, above = CR.sign_change(logits, labels, 1.0 / cal.temperature)
    assert ok, (below, above)
    cal.save(Calibration.path(tmp_path, "ResNet18"))
    loaded = find_sidecar(str(tmp_path), "ResNet18", "classification_models")
    assert loaded == cal
    with pytest.raises(FileNotFoundError, match="VGG16_calibration.json"):
        find_sidecar(str(tmp_path), "VGG16", "classification_models")
    capsys.readouterr()
    plain = tester.evaluate_classification_model(over, loader, DEV, "ResNet18", auc=True)
    plain_text = capsys.readouterr().out
    got = tester.evaluate_classification_model(over, loader, DEV, "ResNet18", auc=True, calibration=loaded)
    text = capsys.readouterr().out
    assert got["accuracy"] == plain["accuracy"] and np.array_equal(got["confusion_matrix"], plain["confusion_matrix"])
    assert set(got) == set(plain) | {"temperature"} and got["temperature"] == cal.temperature
    at = CR.nll_terms(logits, labels, 1.0 / cal.temperature)
    bound = CR.temp_nll_bound(64, 3, at["nll_max"], at["zmax"])
    print(f"NLL: tester {got['nll']!r}, fit {cal.after!r}, restated {at['nll']!r}, bound {bound:.3e}; before {plain['nll']!r} / {cal.before!r}")
    assert abs(got["nll"] - cal.after) <= bound and abs(got["nll"] - at["nll"]) <= bound
    assert abs(plain["nll"] - cal.before) <= bound and got["nll"] < plain["nll"]
    extra = [line for line in text.splitlines() if line not in plain_text.splitlines()]
    assert sum("Calibration: temperature T" in line for line in extra) == 1
    with pytest.raises(ValueError, match="tta"):
        tester.evaluate_classification_model(over, loader, DEV, "ResNet18", auc=True, tta="hflip", calibration=loaded)


def test_segmenter_threshold_through_the_tester(capsys):
    from utils import tester
    from utils.calibrate import calibrate_model
    _, sm, _ = _models()
    loader = _loaders()[1]
    cal = calibrate_model(sm, loader, DEV, seg=True)
    print(cal.describe())
    assert cal.kind == "segmentation" and cal.samples == 64 and cal.after >= cal.before and 0.0 < cal.threshold < 1.0
    assert cal.threshold in CR.DEFAULT_THRESHOLDS.astype(np.float64)
    capsys.readouterr()
    plain = tester.evaluate_segmentation_model(sm, loader, DEV, "AttentionUNet", surface=True)
    plain_text = capsys.readouterr().out
    got = tester.evaluate_segmentation_model_ci(sm, loader, DEV, "AttentionUNet", surface=True, calibration=cal)
    text = capsys.readouterr().out
    tol = 200 * CR.fold_bound(64)
    print(f"Dice: tester {got['dice']!r} at t* = {cal.threshold}, sweep {cal.after * 100!r}; at 0.5 {plain['dice']!r}, sweep {cal.before * 100!r}")
    assert abs(got["dice"] - cal.after * 100) <= tol and abs(plain["dice"] - cal.before * 100) <= tol
    assert got["dice"] >= plain["dice"] and set(got) == set(plain) | {"threshold"} and got["threshold"] == cal.threshold
    extra = [line for line in text.splitlines() if line not in plain_text.splitlines()]
    assert sum(line.startswith("Calibration:") for line in extra) == 1


def test_trainer_calibrates_the_best_checkpoint(tmp_path, capsys):
    from models.segmentation_models.AttentionUNet import AttentionUNet
    from utils import tester, trainer
    from utils.calibrate import Calibration, calibrate_model
    _, sm, _ = _models()
    torch.save(sm.state_dict(), tmp_path / "AttentionUNet_best_loss.pt")
    fresh = AttentionUNet()
    fresh.compute_dtype = torch.float32
    loader = _loaders()[1][:2]
    cal = trainer.calibrate_checkpoint(fresh, loader, DEV, "AttentionUNet", str(tmp_path), True)
    out = capsys.readouterr().out
    assert cal.samples == 32 and Calibration.load(Calibration.path(str(tmp_path), "AttentionUNet")) == cal
    assert cal == calibrate_model(sm, loader, DEV, seg=True)          # the reloaded checkpoint is the model
    assert out.count("[calibration] AttentionUNet: threshold t* =") == 1 and "AttentionUNet_calibration.json" in out
    with pytest.raises(ValueError, match="kind"):
        tester.evaluate_classification_model(sm, _loaders()[0], DEV, "ResNet18", calibration=cal)


def test_pipeline_with_and_without_calibration():
    from utils.calibrate import Calibration, dice_sweep
    from utils.pipeline import CLASSES, JointPipeline
    cm, sm, x = _models()
    plain = JointPipeline(cm, sm, device=DEV, bucket=4).predict(x)
    none = JointPipeline(cm, sm, device=DEV, bucket=4, calibration=None).predict(x)
    assert set(plain) == set(none) and all(torch.equal(plain[k], none[k]) for k in plain)
    t_star = float(np.float32(80 / 256))
    cals = (Calibration("classification", temperature=2.5), Calibration("segmentation", threshold=t_star))
    r = JointPipeline(cm, sm, device=DEV, bucket=4, calibration=cals).predict(x)
    B = x.shape[0]
    with torch.no_grad():
        logits = cm(x).float().contiguous()
    scaled = mnn._logits_scale(logits, torch.tensor([1.0 / 2.5], dtype=torch.float64, device=DEV))
    pred = torch.empty(B, dtype=torch.int32, device=DEV)
    conf = torch.empty(B, dtype=torch.float32, device=DEV)
    kept = torch.empty(B + 4, dtype=torch.int32, device=DEV)
    n_kept = torch.empty(1, dtype=torch.int32, device=DEV)
    lib.mi355_cls_decide(scaled, B, 3, CLASSES.index("COVID"), pred, conf, kept, n_kept)
    assert torch.equal(r["pred"], pred) and torch.equal(r["pred"], plain["pred"]) and torch.equal(r["confidence"], conf)
    assert bool((r["confidence"] <= plain["confidence"]).all()) and bool((r["confidence"] < plain["confidence"]).any())          # T > 1 softens the rows
    n = int(n_kept)
    assert 0 < n < B
    rows = kept[:n].long()
    idx = torch.cat([rows, rows[:1].expand(-n % 4)])
    with torch.no_grad():
        z = sm(x[idx].contiguous()).float().reshape(len(idx), -1)[:n]
    on = r["masks"][rows].reshape(n, -1) != 0
    p = torch.sigmoid(z.double())
    clear = (p - t_star).abs() > 1e-6
    assert torch.equal(on[clear], (p > t_star)[clear]) and bool(((r["masks"] == 0) | (r["masks"] == 255)).all())
    acc = dice_sweep(z, torch.zeros_like(z), thresholds=[t_star], is_logit=True)          # the same expression, counted by the sweep
    assert torch.equal(on.sum(1).to(torch.int32), acc["fp"][:, 0])
    assert not torch.equal(r["masks"], plain["masks"])
    others = torch.ones(B, dtype=torch.bool, device=DEV)
    others[rows] = False
    assert not bool(r["masks"][others].any())
    with pytest.raises(ValueError, match="calibration"):
        JointPipeline(cm, sm, device=DEV, bucket=4, calibration=(cals[1], cals[0]))
