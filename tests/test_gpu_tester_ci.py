"""-m gpu: the bootstrap option of utils/tester.py end to end at 64 x 64 on 64 synthetic samples, with the models tests/test_gpu_tta.py
builds for the same tester functions.  Without ``ci`` both loops return the keys and print the text they always did; with it every
interval brackets the mean of its replicates, the point estimates taken from the identity resample are the plain results (to the bit
where the figure is formed from integers — the classifiers'; within (n + 4) 2^-53 relative for the segmenters' means of per-image
doubles, which the host adds in another order), a seed names its numbers, and two copies of a model differ by exactly nothing."""
import functools
import math
import re

import numpy as np
import pytest
import torch

from test_gpu_tta import DEV, _models

pytestmark = pytest.mark.gpu
N, R = 64, 64
U = 2.0 ** -53
CLS_CI = ("accuracy", "precision", "recall", "f1", "auroc", "average_precision")
SEG_CI = ("iou", "dice", "pixel_accuracy", "precision", "recall", "f1", "hausdorff", "hd95", "assd", "surface_dice", "pixel_auroc", "pixel_ap")
BRACKET = re.compile(r" \[[-+0-9.]+, [-+0-9.]+\]")


@functools.lru_cache(maxsize=None)
def _loaders():
    g = torch.Generator().manual_seed(17)
    x = torch.randn(N, 3, 64, 64, generator=g).to(DEV)
    labels = torch.arange(N) % 3
    masks = (torch.rand(N, 1, 64, 64, generator=g) < 0.4).float()
    masks[5] = 0                                         # an all-background mask: no surface distances, no ROC-AUC
    cls = tuple((x[i:i + 16].contiguous(), labels[i:i + 16]) for i in range(0, N, 16))
    seg = tuple((x[i:i + 16].contiguous(), masks[i:i + 16]) for i in range(0, N, 16))
    return cls, seg


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (np.ndarray, float, tuple)):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b


def _without_ci(text, ci):
    """the text with every ' [lo, hi]', the DeLong note and the footer taken out"""
    text = re.sub(r" \(DeLong \[[0-9.]+, [0-9.]+\]\)", "", text)
    return BRACKET.sub("", text).replace(ci.footer() + "\n", "")


def test_classification_without_ci_is_unchanged(capsys):
    from utils import tester
    cm, _, _ = _models()
    loader = _loaders()[0]
    for kw in ({}, {"auc": True}):
        plain = tester.test_classification_model(cm, loader, DEV, "ResNet18", **kw)
        plain_text = capsys.readouterr().out
        for off in (None, 0):
            got = tester.evaluate_classification_model(cm, loader, DEV, "ResNet18", ci=off, **kw)
            assert capsys.readouterr().out == plain_text and _same(got, plain)
        assert "Bootstrap" not in plain_text and " [" not in plain_text and not any("ci" in k.split("_") for k in plain)


def test_segmentation_without_ci_is_unchanged(capsys):
    from utils import tester
    _, sm, _ = _models()
    loader = _loaders()[1]
    plain = tester.evaluate_segmentation_model(sm, loader, DEV, "AttentionUNet", surface=True, auc=True)
    plain_text = capsys.readouterr().out
    got = tester.evaluate_segmentation_model_ci(sm, loader, DEV, "AttentionUNet", surface=True, auc=True, ci=None)
    assert capsys.readouterr().out == plain_text and _same(got, plain)
    assert _same(tester.test_segmentation_model(sm, loader, DEV, "AttentionUNet", surface=True),
                 tester.evaluate_segmentation_model_ci(sm, loader, DEV, "AttentionUNet", surface=True, ci=0))
    assert "Bootstrap" not in plain_text and " [" not in plain_text


def _brackets(detail, keys):
    for k in keys:
        e = detail[k]
        assert e["valid"] >= 1 and e["lo"] <= e["mean"] <= e["hi"], (k, e)
        assert e["se"] >= 0.0 or e["valid"] < 2, (k, e)


def test_classification_with_ci(capsys):
    from utils import tester
    cm, _, _ = _models()
    loader = _loaders()[0]
    plain = tester.test_classification_model(cm, loader, DEV, "ResNet18", auc=True)
    plain_text = capsys.readouterr().out
    ci = tester.CI(R, 0.95, 3)
    got = tester.evaluate_classification_model(cm, loader, DEV, "ResNet18", auc=True, ci=ci)
    text = capsys.readouterr().out
    new = {f"{k}_ci" for k in CLS_CI} | {f"{k}_se" for k in CLS_CI} | {"auroc_ci_per_class", "auroc_se_per_class", "auroc_delong_ci_per_class",
                                                                      "ci_detail", "ci_replicates", "ci_level", "ci_seed"}
    assert set(got) == set(plain) | new and all(_same(got[k], plain[k]) for k in plain)
    d = got["ci_detail"]
    assert set(d) == set(CLS_CI) | {f"auroc_class{c}" for c in range(3)}
    _brackets(d, d)
    for k in CLS_CI:                                      # row 0 is the plain figure, to the bit
        assert d[k]["point"] == plain[k], (k, d[k]["point"], plain[k])
        assert got[f"{k}_ci"] == (d[k]["lo"], d[k]["hi"]) and got[f"{k}_se"] == d[k]["se"]
    for c in range(3):
        assert d[f"auroc_class{c}"]["point"] == plain["auroc_per_class"][c]
        assert tuple(got["auroc_ci_per_class"][c]) == (d[f"auroc_class{c}"]["lo"], d[f"auroc_class{c}"]["hi"])
        lo, hi = got["auroc_delong_ci_per_class"][c]
        assert 0.0 <= lo <= plain["auroc_per_class"][c] <= hi <= 1.0
    assert (got["ci_replicates"], got["ci_level"], got["ci_seed"]) == (R, 0.95, 3)
    assert _without_ci(text, ci) == plain_text and text.count(ci.footer()) == 1
    assert len(BRACKET.findall(text.replace("(DeLong [", "(DeLong["))) == 4 + 2 + 3 and text.count("(DeLong [") == 3
    assert f"Accuracy:  {got['accuracy']:.2f}% [{got['accuracy_ci'][0]:.2f}, {got['accuracy_ci'][1]:.2f}]" in text
    again = tester.evaluate_classification_model(cm, loader, DEV, "ResNet18", auc=True, ci=(R, 0.95, 3))
    assert _same(again, got)                             # the seed names the numbers
    other = tester.evaluate_classification_model(cm, loader, DEV, "ResNet18", auc=True, ci=tester.CI(R, 0.95, 4))
    assert any(other[f"{k}_ci"] != got[f"{k}_ci"] for k in CLS_CI)
    wide = tester.evaluate_classification_model(cm, loader, DEV, "ResNet18", ci=tester.CI(R, 0.5, 3))
    base = {"accuracy", "precision", "recall", "f1", "precision_per_class", "recall_per_class", "f1_per_class", "confusion_matrix"}
    assert set(wide) == base | {f"{k}_{s}" for k in CLS_CI[:4] for s in ("ci", "se")} | {"ci_detail", "ci_replicates", "ci_level", "ci_seed"}
    for k in CLS_CI[:4]:                                  # the same resamples: the 50 % interval lies inside the 95 % one
        assert got[f"{k}_ci"][0] <= wide[f"{k}_ci"][0] <= wide[f"{k}_ci"][1] <= got[f"{k}_ci"][1] and wide[f"{k}_se"] == got[f"{k}_se"]


def test_segmentation_with_ci(capsys):
    from utils import tester
    _, sm, _ = _models()
    loader = _loaders()[1]
    plain = tester.evaluate_segmentation_model(sm, loader, DEV, "AttentionUNet", surface=True, auc=True)
    plain_text = capsys.readouterr().out
    ci = tester.CI(R, 0.95, 3)
    got = tester.evaluate_segmentation_model_ci(sm, loader, DEV, "AttentionUNet", surface=True, auc=True, ci=ci)
    text = capsys.readouterr().out
    new = {f"{k}_{s}" for k in SEG_CI for s in ("ci", "se")} | {"ci_detail", "ci_replicates", "ci_level", "ci_seed"}
    assert set(got) == set(plain) | new and all(_same(got[k], plain[k]) for k in plain)
    d = got["ci_detail"]
    assert set(d) == set(SEG_CI)
    _brackets(d, SEG_CI)
    assert plain["surface_samples"] < N and plain["auc_samples"] < N          # asserted of the input: an undefined sample is counted out
    for k in SEG_CI:                                      # the same values in another order of additions: (n + 4) u relative (all >= 0)
        assert abs(d[k]["point"] - plain[k]) <= (N + 4) * U * abs(plain[k]), (k, d[k]["point"], plain[k])
        assert d[k]["valid"] == R
    assert _without_ci(text, ci) == plain_text and text.count(ci.footer()) == 1 and len(BRACKET.findall(text)) == len(SEG_CI)
    again = tester.evaluate_segmentation_model_ci(sm, loader, DEV, "AttentionUNet", surface=True, auc=True, ci=tester.CI(R, 0.95, 3))
    assert _same(again, got)
    only = tester.evaluate_segmentation_model_ci(sm, loader, DEV, "AttentionUNet", ci=R)
    assert set(only["ci_detail"]) == set(SEG_CI[:6]) and only["ci_seed"] == 0


def test_copies_of_a_model_are_identical(capsys):
    from utils import tester
    from utils.tta import TTAClassifier
    cm, sm, _ = _models()
    cls_loader, seg_loader = _loaders()
    ci = tester.CI(R, 0.95, 1)
    results = {"ResNet18": tester.evaluate_classification_model(cm, cls_loader, DEV, "ResNet18", auc=True, ci=ci),
               "ResNet50": tester.evaluate_classification_model(cm, cls_loader, DEV, "ResNet50", auc=True, ci=ci),
               "AttentionUNet": tester.evaluate_segmentation_model_ci(sm, seg_loader, DEV, "AttentionUNet", ci=ci),
               "R2Unet": tester.evaluate_segmentation_model_ci(sm, seg_loader, DEV, "R2Unet", ci=ci)}
    capsys.readouterr()
    rows = tester.print_paired_tests(results, ci)
    text = capsys.readouterr().out
    c = rows[("ResNet50", "ResNet18")]
    assert c["d_accuracy"] == 0.0 and c["d_accuracy_ci"] == (0.0, 0.0) and c["d_auroc"] == 0.0 and c["d_auroc_ci"] == (0.0, 0.0)
    assert c["mcnemar"]["p"] == 1.0 and c["mcnemar"]["b"] == c["mcnemar"]["c"] == 0
    assert all(math.isnan(t["z"]) and t["auc_a"] == t["auc_b"] for t in c["delong"]) and text.count("identical") == 3
    s = rows[("R2Unet", "AttentionUNet")]
    assert s["d_dice"] == 0.0 and s["d_dice_ci"] == (0.0, 0.0)
    assert "against ResNet18" in text and "against AttentionUNet" in text and text.count(ci.footer()) == 1
    # a model that does differ: the same classifier under test-time augmentation, on the same resamples
    results["ResNet50"] = tester.evaluate_classification_model(TTAClassifier(cm, "hflip"), cls_loader, DEV, "ResNet50", auc=True, ci=ci)
    capsys.readouterr()
    rows = tester.print_paired_tests(results, ci)
    (pair, row), = [(k, v) for k, v in rows.items() if "ResNet50" in k and "ResNet18" in k]
    sign = 1.0 if pair[0] == "ResNet50" else -1.0
    assert abs(row["d_accuracy"] - sign * (results["ResNet50"]["accuracy"] - results["ResNet18"]["accuracy"])) <= 1e-9
    assert row["d_accuracy_ci"][0] <= row["d_accuracy_ci"][1] and 0.0 <= row["mcnemar"]["p"] <= 1.0
    a, b = ci.kept[pair[0]], ci.kept[pair[1]]
    ok_a, ok_b = (a["pred"] == a["labels"]).cpu().numpy(), (b["pred"] == b["labels"]).cpu().numpy()
    assert (row["mcnemar"]["b"], row["mcnemar"]["c"]) == (int((ok_a & ~ok_b).sum()), int((~ok_a & ok_b).sum()))
    assert tester.print_paired_tests(results, None) == {}


def test_all_models_hands_one_set_of_resamples_to_every_model(tmp_path, capsys):
    from torch.utils.data import DataLoader, TensorDataset
    from oracle import train as otrain
    from utils import tester
    from utils.helpers import get_class_model, get_seg_model
    seg_dir, cls_dir = tmp_path / "seg", tmp_path / "cls"
    seg_dir.mkdir()
    cls_dir.mkdir()
    torch.manual_seed(11)
    torch.save(get_seg_model("AttentionUNet").state_dict(), seg_dir / "AttentionUNet_best_loss.pt")
    torch.save(get_class_model("ResNet18")[0].state_dict(), cls_dir / "ResNet18_best_acc.pt")
    xs, ms = zip(*[otrain.synthetic_batch(4, 32, seed=s) for s in (1, 2)])
    seg_dl = DataLoader(TensorDataset(torch.cat(xs), torch.cat(ms)), batch_size=4)
    cls_dl = DataLoader(TensorDataset(torch.cat(xs), torch.tensor([0, 1, 2, 1, 0, 2, 1, 0])), batch_size=4)
    kw = dict(cls_loader=cls_dl, seg_loader=seg_dl, cls_weights_dir=str(cls_dir), seg_weights_dir=str(seg_dir))
    plain = tester.test_all_models("cuda", 4, **kw)
    plain_text = capsys.readouterr().out
    ci = tester.CI(8, 0.9, 2)
    res = tester.test_all_models("cuda", 4, ci=ci, **kw)
    text = capsys.readouterr().out
    assert set(res) == set(plain) == set(ci.kept) == {"ResNet18", "AttentionUNet"}
    assert all(_same(res[m][k], plain[m][k]) for m in plain for k in plain[m])
    assert res["ResNet18"]["ci_replicates"] == res["AttentionUNet"]["ci_replicates"] == 8 and "accuracy_ci" in res["ResNet18"]
    assert "dice_ci" in res["AttentionUNet"] and text.count(ci.footer()) == 2 and _without_ci(text, ci) == plain_text
    assert ci.kept["ResNet18"]["accuracy"].shape == (9,) and ci.kept["AttentionUNet"]["dice"].shape == (9,)
    assert _same(tester.test_all_models("cuda", 4, ci=0, **kw), plain)
    tester.print_summary(res)


def test_csv_has_the_interval_columns_only_with_ci(tmp_path, capsys):
    import pandas as pd
    from utils import tester
    cm, sm, _ = _models()
    cls_loader, seg_loader = _loaders()
    plain = {"ResNet18": tester.test_classification_model(cm, cls_loader, DEV, "ResNet18"),
             "AttentionUNet": tester.test_segmentation_model(sm, seg_loader, DEV, "AttentionUNet")}
    tester.save_results_to_csv(plain, str(tmp_path / "c0.csv"), str(tmp_path / "s0.csv"))
    assert list(pd.read_csv(tmp_path / "c0.csv").columns) == ["Model", "accuracy", "precision", "recall", "f1"]
    assert list(pd.read_csv(tmp_path / "s0.csv").columns) == ["Model", "iou", "dice", "pixel_accuracy", "precision", "recall", "f1"]
    ci = tester.CI(R)
    with_ci = {"ResNet18": tester.evaluate_classification_model(cm, cls_loader, DEV, "ResNet18", ci=ci),
               "AttentionUNet": tester.evaluate_segmentation_model_ci(sm, seg_loader, DEV, "AttentionUNet", ci=ci)}
    tester.save_results_to_csv(with_ci, str(tmp_path / "c1.csv"), str(tmp_path / "s1.csv"))
    c, s = pd.read_csv(tmp_path / "c1.csv"), pd.read_csv(tmp_path / "s1.csv")
    extra = lambda keys: [f"{k}_{x}" for k in keys for x in ("lo", "hi", "se")] + ["ci_replicates", "ci_level", "ci_seed"]      # noqa: E731
    assert list(c.columns) == ["Model", "accuracy", "precision", "recall", "f1"] + extra(CLS_CI[:4])
    assert list(s.columns) == ["Model", "iou", "dice", "pixel_accuracy", "precision", "recall", "f1"] + extra(SEG_CI[:6])
    for frame in (c, s):
        assert all(np.issubdtype(frame[k].dtype, np.number) for k in frame.columns if k != "Model")
    assert abs(c["accuracy_lo"][0] - with_ci["ResNet18"]["accuracy_ci"][0]) < 1e-9
    assert abs(s["dice_hi"][0] - with_ci["AttentionUNet"]["dice_ci"][1]) < 1e-9
