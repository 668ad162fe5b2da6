"""-m gpu: the ``auc=`` option of utils/tester.py end to end at 64 x 64, on the models and the batch tests/test_gpu_tta.py builds for
the same tester functions.  The new keys are the restatement tests/ranking_ref.py applied to the models' read-back outputs: integers
(and the ROC-AUCs, one division of them) exactly, the floating-point means within 1e-9.  Without the option the result dictionary and
the printed text are what they are with it, less the new keys and lines.  (The segmentation loop with ``auc`` is
evaluate_segmentation_model: test_segmentation_model keeps the argument list that tests/test_surface_cpu.py pins.)"""
import functools

import numpy as np
import pytest
import torch

import ranking_ref as R
from test_gpu_tta import DEV, _models

pytestmark = pytest.mark.gpu
CLS_KEYS = {"accuracy", "precision", "recall", "f1", "precision_per_class", "recall_per_class", "f1_per_class", "confusion_matrix"}
CLS_NEW = {"auroc", "average_precision", "auc_classes", "auroc_per_class", "ap_per_class", "ece", "brier", "nll"}
SEG_KEYS = {"iou", "dice", "pixel_accuracy", "precision", "recall", "f1"}
SEG_NEW = {"pixel_auroc", "pixel_ap", "auc_samples"}


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) if isinstance(a, (np.ndarray, float)) else a == b


@functools.lru_cache(maxsize=None)
def _cls_loader():
    _, _, x = _models()
    labels = torch.arange(16) % 3
    return ((x[:8].contiguous(), labels[:8]), (x[8:].contiguous(), labels[8:]))


@functools.lru_cache(maxsize=None)
def _seg_loader():
    _, _, x = _models()
    g = torch.Generator().manual_seed(9)
    second = (torch.rand(2, 1, 64, 64, generator=g) < 0.4).float()
    second[1] = 0                                        # an all-background mask: no ROC-AUC, no average precision
    return ((x[0:4].contiguous(), (torch.rand(4, 1, 64, 64, generator=g) < 0.4).float()), (x[4:6].contiguous(), second))


def _check_cls(got, scores, labels, is_prob):
    ref = R.calibration_ref(scores, labels, 15, is_prob)
    assert ref["top2_gap"] >= 1e-6 and ref["edge_distance"] >= 1e-6          # conditions on the read-back outputs
    ranked = R.rank_ref(ref["scores_t"], labels=labels)
    gaps = np.diff(np.sort(ref["scores_t"].astype(np.float64), 1), axis=1)
    assert is_prob or (gaps > 4 * np.spacing(np.float32(1))).all()          # no two scores of a class within the fp32 rounding of the softmax
    auroc, ap = np.array([r["auroc"] for r in ranked]), np.array([r["ap"] for r in ranked])
    assert not np.isnan(auroc).any()
    assert np.array_equal(got["auroc_per_class"], auroc) and got["auc_classes"] == 3
    assert np.abs(got["ap_per_class"] - ap).max() <= 1e-9
    assert abs(got["auroc"] - auroc.mean()) <= 1e-9 and abs(got["average_precision"] - ap.mean()) <= 1e-9
    assert abs(got["ece"] - ref["ece"]) <= 1e-9 and abs(got["brier"] - ref["brier"]) <= 1e-9 and abs(got["nll"] - ref["nll"]) <= 1e-9
    assert 0.0 <= got["auroc"] <= 1.0 and 0.0 <= got["average_precision"] <= 1.0


def test_classification_with_auc(capsys):
    from utils import tester
    cm, _, _ = _models()
    loader = _cls_loader()
    labels = np.concatenate([y.numpy() for _, y in loader])
    got = tester.test_classification_model(cm, loader, DEV, "ResNet18", auc=True)
    text = capsys.readouterr().out
    assert set(got) == CLS_KEYS | CLS_NEW
    with torch.no_grad():
        z = np.concatenate([cm(images).float().cpu().numpy() for images, _ in loader])
    _check_cls(got, z, labels, False)
    assert text.count("AUROC / AP: ") == 1 and text.count("ECE (15 bins) / Brier / NLL: ") == 1
    assert f"AUROC / AP: {got['auroc']:.4f} / {got['average_precision']:.4f}" in text
    assert f"ECE (15 bins) / Brier / NLL: {got['ece']:.4f} / {got['brier']:.4f} / {got['nll']:.4f}" in text
    assert text.count("\n  AUROC:     ") == 3 and text.count("\n  AP:        ") == 3
    assert text.index("F1 Score:  ") < text.index("AUROC / AP: ") < text.index("ECE (15 bins)") < text.index("Per-Class Metrics:")
    # without the option: today's keys, values and text
    plain = tester.test_classification_model(cm, loader, DEV, "ResNet18")
    plain_text = capsys.readouterr().out
    assert set(plain) == CLS_KEYS and all(_same(plain[k], got[k]) for k in CLS_KEYS)
    assert "AUROC" not in plain_text and "ECE" not in plain_text
    new_lines = [l for l in text.splitlines() if l.startswith(("AUROC / AP: ", "ECE (15 bins) / Brier / NLL: ", "  AUROC:     ", "  AP:        "))]
    assert len(new_lines) == 8 and [l for l in text.splitlines() if l not in new_lines] == plain_text.splitlines()
    ten = tester.test_classification_model(cm, loader, DEV, "ResNet18", auc=True, calibration_bins=10)
    assert "ECE (10 bins) / Brier / NLL: " in capsys.readouterr().out and ten["nll"] == got["nll"] and ten["auroc"] == got["auroc"]
    assert abs(ten["ece"] - R.calibration_ref(z, labels, 10)["ece"]) <= 1e-9


def test_classification_with_auc_and_tta_ranks_the_merged_probabilities(capsys):
    from utils import tester
    from utils.tta import TTAClassifier
    cm, _, _ = _models()
    loader = _cls_loader()
    labels = np.concatenate([y.numpy() for _, y in loader])
    got = tester.test_classification_model(cm, loader, DEV, "ResNet18", tta="hflip", auc=True)
    assert set(got) == CLS_KEYS | CLS_NEW | {"tta_views", "tta_agreement"}
    probs = np.concatenate([TTAClassifier(cm, "hflip")(images)["probs"].float().cpu().numpy() for images, _ in loader])
    _check_cls(got, probs, labels, True)
    text = capsys.readouterr().out
    assert text.index("TTA agreement:") < text.index("AUROC / AP: ")


def _check_seg(got, scores, masks, n_defined):
    auroc, ap = [], []
    for z, m in zip(scores, masks):
        for r in R.rank_ref(z.reshape(len(z), -1), target=m.reshape(len(m), -1)):
            auroc.append(r["auroc"])
            ap.append(r["ap"])
    auroc, ap = np.array(auroc), np.array(ap)
    assert int((~np.isnan(auroc)).sum()) == n_defined == got["auc_samples"]
    assert abs(got["pixel_auroc"] - np.nanmean(auroc)) <= 1e-9 and abs(got["pixel_ap"] - np.nanmean(ap)) <= 1e-9
    assert 0.0 <= got["pixel_auroc"] <= 1.0 and 0.0 <= got["pixel_ap"] <= 1.0


def test_segmentation_with_auc(capsys):
    from utils import tester
    _, sm, _ = _models()
    loader = _seg_loader()
    got = tester.evaluate_segmentation_model(sm, loader, DEV, "AttentionUNet", auc=True)
    text = capsys.readouterr().out
    assert set(got) == SEG_KEYS | SEG_NEW
    with torch.no_grad():
        z = [sm(images).float().cpu().numpy() for images, _ in loader]
    _check_seg(got, z, [m.numpy() for _, m in loader], 5)          # the all-background mask is counted out
    line = f"Pixel AUROC / AP:  {got['pixel_auroc']:.4f} / {got['pixel_ap']:.4f} (5 of 6 samples)"
    assert text.count(line) == 1 and text.index("F1 Score:") < text.index(line)
    plain = tester.test_segmentation_model(sm, loader, DEV, "AttentionUNet")
    plain_text = capsys.readouterr().out
    assert set(plain) == SEG_KEYS and all(plain[k] == got[k] for k in SEG_KEYS)
    assert "AUROC" not in plain_text and [l for l in text.splitlines() if l != line] == plain_text.splitlines()
    both = tester.evaluate_segmentation_model(sm, loader, DEV, "AttentionUNet", surface=True, auc=True)
    out = capsys.readouterr().out
    assert set(both) == SEG_KEYS | SEG_NEW | set(tester.SURFACE_KEYS) | {"surface_samples"} and both["pixel_auroc"] == got["pixel_auroc"]
    assert out.index("Surface Dice @2px:") < out.index("Pixel AUROC / AP:")


@pytest.mark.parametrize("merge", ["prob", "logit"])
def test_segmentation_with_auc_and_tta_ranks_the_merged_map(merge, capsys):
    from utils import tester
    from utils.tta import TTASegmenter
    _, sm, _ = _models()
    loader = _seg_loader()
    got = tester.evaluate_segmentation_model(TTASegmenter(sm, "hflip", merge=merge), loader, DEV, "AttentionUNet", auc=True)
    assert set(got) == SEG_KEYS | SEG_NEW | {"tta_unanimous", "tta_views"}
    merged = [TTASegmenter(sm, "hflip", merge=merge)(images)["mean"].float().cpu().numpy() for images, _ in loader]
    if merge == "prob":
        assert all(0.0 <= m.min() and m.max() <= 1.0 for m in merged)
    _check_seg(got, merged, [m.numpy() for _, m in loader], 5)
    text = capsys.readouterr().out
    assert text.index("Pixel AUROC / AP:") < text.index("TTA unanimous:")


def test_csv_rows_hold_scalars_only(tmp_path, capsys):
    pd = pytest.importorskip("pandas")
    from utils import tester
    cm, sm, _ = _models()
    results = {"ResNet18": tester.test_classification_model(cm, _cls_loader(), DEV, "ResNet18", auc=True),
               "AttentionUNet": tester.evaluate_segmentation_model(sm, _seg_loader(), DEV, "AttentionUNet", auc=True)}
    tester.print_summary(results)
    text = capsys.readouterr().out
    assert "CLASSIFICATION MODELS, RANKING AND CALIBRATION" in text and "SEGMENTATION MODELS, PIXEL RANKING" in text
    tester.save_results_to_csv(results, str(tmp_path / "c.csv"), str(tmp_path / "s.csv"))
    c, s = pd.read_csv(tmp_path / "c.csv"), pd.read_csv(tmp_path / "s.csv")
    assert list(c.columns) == ["Model", "accuracy", "precision", "recall", "f1", "auroc", "auc_classes", "average_precision", "ece", "brier", "nll"]
    assert list(s.columns) == ["Model"] + ["iou", "dice", "pixel_accuracy", "precision", "recall", "f1", "pixel_auroc", "auc_samples", "pixel_ap"]
    for frame in (c, s):
        assert all(np.issubdtype(frame[k].dtype, np.number) for k in frame.columns if k != "Model")
    assert abs(c["auroc"][0] - results["ResNet18"]["auroc"]) < 1e-12 and s["auc_samples"][0] == 5
