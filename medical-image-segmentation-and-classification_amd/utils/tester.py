"""Evaluation metrics and loops of the MI355X path — same names and return values as the
reference's utils/tester.py (segmentation metrics :92-193, classification metrics :49-88, eval
loops :197-312).  Per-sample counters come from one HIP reduction per batch instead of ~9 host
syncs per sample.  On request (``surface=True`` / ``--surface``) the segmentation loop also reports
the boundary metrics the reference lacks: Hausdorff distance, HD95, ASSD and surface Dice
(csrc/surface.hip; DESIGN.md, "Surface-distance metrics"), and (``auc=True`` / ``--auc``) both loops report the threshold-free figures:
ROC-AUC and average precision — per class for the classifiers, per image over the pixels for the segmenters
(``evaluate_segmentation_model``) — and the classifiers' calibration (ECE, Brier score, NLL), from csrc/ranking.hip ("Ranking metrics and calibration")."""
import math
import os

import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # `python utils/tester.py` (tester.py:22-24 does the same)
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from mi355.lib import lib  # noqa: E402

CLASSES = ["COVID", "Healthy", "Non-COVID"]
DATA_ROOT = "dataset"
WEIGHTS_ROOT = "weights"
CLS_WEIGHTS_DIR = os.path.join(WEIGHTS_ROOT, "classification_models")
SEG_WEIGHTS_DIR = os.path.join(WEIGHTS_ROOT, "segmentation_models")
IMG_SIZE = 256
_E = 1e-7


def _counts(pred, target, threshold, is_logit=False):
    """[B,4] float64 numpy: tp, predicted-positive, target-positive, equal — per sample."""
    B = pred.shape[0]
    per = pred[0].numel()
    if pred.is_cuda:
        cnt = torch.empty(B, 4, dtype=torch.float32, device=pred.device)
        lib.mi355_seg_counts(pred.float().contiguous(), target.float().contiguous(), cnt, B, per, 1 if is_logit else 0,
                             float(threshold))
        return cnt.double().cpu().numpy(), per
    p = (torch.sigmoid(pred) if is_logit else pred) > threshold
    t = target > threshold
    f = lambda z: z.reshape(B, -1).sum(1).double()
    return torch.stack([f(p & t), f(p), f(t), f(p == t)], 1).numpy(), per


def _metrics_from_counts(c, per):
    tp, pp, tt, eq = c
    fp, fn, union = pp - tp, tt - tp, pp + tt - tp
    prec = (tp + _E) / (tp + fp + _E)
    rec = (tp + _E) / (tp + fn + _E)
    return {"iou": (tp + _E) / (union + _E) * 100, "dice": (2.0 * tp + _E) / (pp + tt + _E) * 100,
            "pixel_accuracy": eq / per * 100, "precision": prec * 100, "recall": rec * 100,
            "f1": 2 * (prec * rec) / (prec + rec + _E) * 100}


def _single(pred, target, threshold):
    c, per = _counts(pred.reshape(1, -1), target.reshape(1, -1), threshold)
    return _metrics_from_counts(c[0], per)


def calculate_iou(pred, target, threshold=0.5):
    return _single(pred, target, threshold)["iou"] / 100


def calculate_dice(pred, target, threshold=0.5):
    return _single(pred, target, threshold)["dice"] / 100


def calculate_pixel_accuracy(pred, target, threshold=0.5):
    return _single(pred, target, threshold)["pixel_accuracy"] / 100


def calculate_segmentation_metrics(pred, target, threshold=0.5):
    return _single(pred, target, threshold)


# ---- surface-distance metrics (nothing in the reference; definition in DESIGN.md and tests/surface_ref.py) ----------------
SURFACE_KEYS = ("hausdorff", "hd95", "assd", "surface_dice")


def _surface_values(out_i, out_d, spacing, q, xp):
    """The four per-sample metrics from mi355_surface_distances' raw output, in float64, on numpy arrays (xp = np) or torch
    tensors (xp = torch: device arithmetic, nothing is read back).  out_i [B, 8] = n_P, n_T, max d2_PT, max d2_TP, d2[lo], d2[hi],
    #{d2_PT <= tol2}, #{d2_TP <= tol2}; out_d [B, 2] = sum d_PT, sum d_TP.  Both borders empty: 0, 0, 0, 1; one empty: NaN."""
    f = (lambda a: a.astype(np.float64)) if xp is np else (lambda a: a.double())
    n_p, n_t, m_pt, m_tp, lo2, hi2, w_pt, w_tp = (f(out_i[:, k]) for k in range(8))
    s_pt, s_tp = f(out_d[:, 0]), f(out_d[:, 1])
    n = n_p + n_t
    one = lambda a: xp.clip(a, 1.0, None)
    r = xp.remainder(q * xp.clip(n - 1.0, 0.0, None), 100.0) / 100.0       # integers below 2^53: exact
    res = {"hausdorff": spacing * xp.sqrt(xp.maximum(m_pt, m_tp)),
           "hd95": spacing * ((1.0 - r) * xp.sqrt(lo2) + r * xp.sqrt(hi2)),
           "assd": spacing * 0.5 * (s_pt / one(n_p) + s_tp / one(n_t)),
           "surface_dice": (w_pt + w_tp) / one(n) + f(n == 0)}
    undefined = (n_p == 0) != (n_t == 0)
    nan = xp.full_like(n, float("nan"))
    return {k: xp.where(undefined, nan, v) for k, v in res.items()}


def _surface_from_raw(out_i, out_d, spacing=1.0, q=95):
    """numpy: raw arrays of mi355_surface_distances -> {"hausdorff", "hd95", "assd", "surface_dice"}, float64 arrays [B]."""
    return _surface_values(np.asarray(out_i).reshape(-1, 8), np.asarray(out_d).reshape(-1, 2), float(spacing), int(q), np)


def _surface_tol2(tolerance, spacing):
    """d * spacing <= tolerance as an integer bound on d^2 (the relative 1e-12 keeps ratios like 0.3 / 0.1 on the integer meant)"""
    if not (spacing > 0 and tolerance >= 0):
        raise ValueError(f"surface metrics: spacing must be positive and tolerance non-negative ({spacing}, {tolerance})")
    return int(min(math.floor((tolerance / spacing) ** 2 * (1.0 + 1e-12)), 2 ** 31 - 1))


def _surface_raw(pred, target, is_logit, threshold, percentile, tol2):
    """Launch mi355_surface_distances on [B,1,H,W] / [B,H,W] maps -> (out_i int32 [B, 8], out_d float64 [B, 2]) on the device."""
    if pred.dim() == 4:
        if pred.shape[1] != 1:
            raise ValueError(f"surface metrics are defined for one-channel masks, got C={pred.shape[1]}")
        pred = pred[:, 0]
    if target.dim() == 4:
        if target.shape[1] != 1:
            raise ValueError(f"surface metrics are defined for one-channel masks, got C={target.shape[1]} (target)")
        target = target[:, 0]
    if pred.dim() != 3 or pred.shape != target.shape:
        raise ValueError(f"surface metrics: [B,1,H,W] or [B,H,W] maps of one shape expected, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if int(percentile) != percentile or not 0 <= percentile <= 100:
        raise ValueError(f"surface metrics: percentile must be an integer in 0..100, got {percentile}")
    if not pred.is_cuda:
        pred = pred.cuda()
    target = target.to(pred.device)
    B, H, W = pred.shape
    n = lib.raw("mi355_surface_ws_ints")(B, H, W)
    if n < 0:
        raise RuntimeError(f"mi355_surface_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    ws = torch.empty(n, dtype=torch.int32, device=pred.device)
    out_i = torch.empty(B, 8, dtype=torch.int32, device=pred.device)
    out_d = torch.empty(B, 2, dtype=torch.float64, device=pred.device)
    lib.mi355_surface_distances(pred.float().contiguous(), target.float().contiguous(), B, H, W, 1 if is_logit else 0, float(threshold),
                                int(percentile), tol2, ws, n, out_i, out_d)
    return out_i, out_d


def surface_metrics_batch(pred, target, is_logit=False, threshold=0.5, spacing=1.0, percentile=95, tolerance=2.0):
    """Per-sample Hausdorff distance, its percentile (HD95 by default), average symmetric surface distance (in units of
    ``spacing``) and surface Dice at ``tolerance`` (same unit) of [B,1,H,W] / [B,H,W] maps, H, W <= 1024: float64 device tensors
    [B] (NaN where exactly one of the two masks has no border), plus the raw output under "out_i" / "out_d".  Four launches and
    a few element-wise ops on the current stream; nothing synchronises with the host — reading the values back is the caller's."""
    out_i, out_d = _surface_raw(pred, target, is_logit, threshold, percentile, _surface_tol2(tolerance, spacing))
    res = _surface_values(out_i, out_d, float(spacing), int(percentile), torch)
    res["out_i"], res["out_d"] = out_i, out_d
    return res


def calculate_surface_metrics(pred, target, threshold=0.5, spacing=1.0, percentile=95, tolerance=2.0):
    """One sample ([H,W] or [1,H,W] probabilities, like calculate_segmentation_metrics) -> dict of four floats."""
    H, W = pred.shape[-2:]
    res = surface_metrics_batch(pred.reshape(1, H, W), target.reshape(1, H, W), False, threshold, spacing, percentile, tolerance)
    return {k: float(res[k][0]) for k in SURFACE_KEYS}


def calculate_classification_metrics(all_preds, all_labels):
    """Accuracy and support-weighted precision/recall/F1 (+ per class, confusion matrix), the
    quantities sklearn's *_score(average="weighted", zero_division=0) return (tester.py:49-88)."""
    p = np.asarray(all_preds).astype(np.int64)
    y = np.asarray(all_labels).astype(np.int64)
    labels = np.unique(np.concatenate([p, y]))
    k = len(labels)
    idx = {int(l): i for i, l in enumerate(labels)}
    cm = np.zeros((k, k), dtype=np.int64)
    for a, b in zip(y, p):
        cm[idx[int(a)], idx[int(b)]] += 1
    tp = np.diag(cm).astype(np.float64)
    pred_pos, support = cm.sum(0).astype(np.float64), cm.sum(1).astype(np.float64)
    prec = np.divide(tp, pred_pos, out=np.zeros(k), where=pred_pos > 0)
    rec = np.divide(tp, support, out=np.zeros(k), where=support > 0)
    f1 = np.divide(2 * prec * rec, prec + rec, out=np.zeros(k), where=(prec + rec) > 0)
    w = support / support.sum()
    return {"accuracy": float((p == y).mean()) * 100, "precision": float((prec * w).sum()) * 100,
            "recall": float((rec * w).sum()) * 100, "f1": float((f1 * w).sum()) * 100,
            "precision_per_class": prec * 100, "recall_per_class": rec * 100, "f1_per_class": f1 * 100,
            "confusion_matrix": cm}


def _nanmean(values):
    """-> (mean of the values that are not NaN, or NaN; how many entered it)"""
    v = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(v)
    return (float(v[ok].mean()) if ok.any() else float("nan")), int(ok.sum())


# ---- bootstrap intervals and paired tests (nothing in the reference; utils/resample.py, DESIGN.md "Resampling statistics") ----------
class CI:
    """The bootstrap settings of a tester run: ``replicates`` resamples of the test set (1 .. 8192), percentile intervals at ``level``,
    the generator's ``seed``.  Both loops accept it (or the bare number of replicates) as ``ci=``.  One object handed to several
    models makes their resamples the same, and ``kept[model_name]`` then holds what ``print_paired_tests`` compares: per-sample
    predictions, labels and class scores or Dice values, and the replicates of accuracy / macro AUROC / Dice — all device tensors."""

    def __init__(self, replicates, level=0.95, seed=0):
        if int(replicates) != replicates or not 1 <= replicates <= 8192:
            raise ValueError(f"ci: the number of bootstrap replicates must be an integer in 1..8192, got {replicates}")
        if not 0.0 < level < 1.0:
            raise ValueError(f"ci: 0 < level < 1 expected, got {level}")
        self.replicates, self.level, self.seed, self.kept = int(replicates), float(level), int(seed), {}

    def footer(self):
        return f"Bootstrap: {self.replicates} replicates, {self.level * 100:g}% percentile intervals, seed {self.seed}"


def _check_ci(ci):
    """None / 0 -> None, a CI -> itself, R or (R, level, seed) -> CI"""
    if ci is None or isinstance(ci, CI):
        return ci
    if isinstance(ci, (tuple, list)):
        return CI(*ci)
    return None if ci == 0 else CI(ci)


def _nanmean_rows(x):
    """float64 device tensor [R1, C] -> [R1]: the mean over the defined entries of a row, added in column order.  _nanmean's
    numpy mean adds in that order too while there are fewer than 8 terms (pairwise above that): row 0 equals its result to the bit for
    the project's three classes, within (C + 1) 2^-53 relative for more than seven."""
    ok = ~torch.isnan(x)
    total, count = torch.zeros_like(x[:, 0]), torch.zeros_like(x[:, 0])
    for c in range(x.shape[1]):
        total = total + torch.where(ok[:, c], x[:, c], torch.zeros_like(total))
        count = count + ok[:, c].double()
    return total / count


def _intervals(names, reps, ci, extra=None):
    """replicates [R1, K] on the device -> {name: {"point", "mean", "se", "lo", "hi", "valid"}} of floats: one launch, one read-back.
    ``extra`` (a float64 device tensor [E]) rides along in that read-back: -> (the dictionary, float64 numpy [E])."""
    from utils import resample
    iv = resample.interval(reps, ci.level)
    keys = ("point", "mean", "se", "lo", "hi", "valid")
    flat = torch.cat([iv[k] for k in keys] + ([extra.double().reshape(-1)] if extra is not None else [])).cpu().numpy()
    K = len(names)
    detail = {name: {k: float(flat[j * K + i]) for j, k in enumerate(keys)} for i, name in enumerate(names)}
    return detail if extra is None else (detail, flat[len(keys) * K:].copy())


def _ci_text(detail, key, fmt, scale=1.0):
    """' [lo, hi]' in the metric's own format, or '' without intervals"""
    if detail is None or key not in detail:
        return ""
    return f" [{detail[key]['lo'] * scale:{fmt}}, {detail[key]['hi'] * scale:{fmt}}]"


def test_classification_model(model, test_loader, device, model_name, tta=None, auc=False, calibration_bins=15):
    """The classification eval loop with the argument list its callers know: evaluate_classification_model without bootstrap intervals,
    which documents every option."""
    return evaluate_classification_model(model, test_loader, device, model_name, tta=tta, auc=auc, calibration_bins=calibration_bins)


def evaluate_classification_model(model, test_loader, device, model_name, tta=None, auc=False, calibration_bins=15, ci=None,
                                  calibration=None):
    """``tta`` (a preset name or a list of views, utils/tta.py; or pass ``utils.tta.TTAClassifier(model, views)`` as the model): the
    predictions are the argmax of the views' mean softmax, and the result gains ``tta_agreement`` (%, the mean share of views whose
    own argmax is the prediction) and ``tta_views``.
    ``auc=True``: the logits (with ``tta`` the views' mean softmax) stay on the device across the loop; one calibration call and one
    ranking call after it (utils/ranking.py, one segment per class, one-vs-rest) add ``auroc`` and ``average_precision`` (fractions in
    [0, 1]: the macro mean over the classes where they are defined — a class with no sample, or for auroc with every sample, is left
    out), ``auc_classes`` (how many classes entered the auroc mean), ``auroc_per_class``, ``ap_per_class`` and the calibration figures
    ``ece`` (over ``calibration_bins`` confidence bins), ``brier`` and ``nll``.
    ``ci`` (a ``CI``, or the number of bootstrap replicates): the predictions, labels and scores that are on the device anyway are
    resampled there (utils/resample.py: one weights call, one confusion call, with ``auc`` one ranking and one DeLong call, one
    interval call, one read-back).  The result gains ``<key>_ci`` = (lo, hi) and ``<key>_se`` for accuracy, precision, recall, f1
    and, with ``auc``, auroc and average_precision; ``auroc_ci_per_class`` / ``auroc_se_per_class``; ``auroc_delong_ci_per_class``
    (auc -+ z sqrt(DeLong's variance), clipped to [0, 1]); ``ci_detail`` ({name: point, mean, se, lo, hi, valid}: ``point`` is the
    same code on the identity resample) and ``ci_replicates`` / ``ci_level`` / ``ci_seed``; every printed figure its `` [lo, hi]``.
    ``calibration`` (a ``utils.calibrate.Calibration`` of kind "classification", trainer.py --calibrate): with ``auc`` the logits are
    divided by its temperature (csrc/calibrate.hip) before the softmax that feeds the calibration and ranking figures, so ``ece``,
    ``brier`` and ``nll`` are the calibrated model's — ``nll`` evaluated in double on the unrounded scaled logits, the figure the fit
    minimised; the argmax, and with it the accuracy and the confusion matrix, is unchanged.  The result gains ``temperature`` and one
    line is printed.  Not together with ``tta``, whose scores are mean probabilities: ValueError."""
    from utils.tta import TTAClassifier
    ci = _check_ci(ci)
    if calibration is not None and calibration.kind != "classification":
        raise ValueError(f"a classifier's calibration is expected, got one of kind {calibration.kind!r}")
    if calibration is not None and (tta is not None or isinstance(model, TTAClassifier)):
        raise ValueError("a temperature scales logits: calibration together with tta (mean probabilities) is not supported")
    model.eval()
    preds, labels, agree, kept_scores = [], [], [], []
    print(f"\n{'=' * 60}\nTesting Classification Model: {model_name}\n{'=' * 60}")
    if isinstance(model, TTAClassifier):
        tta = cls_tta = model
    elif tta is not None:
        cls_tta = TTAClassifier(model, tta)
    with torch.no_grad():
        for images, y in test_loader:
            if tta is None:
                out = model(images.to(device))
                preds.append(torch.max(out, 1)[1])
                if auc:
                    kept_scores.append(out.float())
            else:
                r = cls_tta(images.to(device))
                preds.append(r["pred"])
                agree.append(r["agreement"])
                if auc:
                    kept_scores.append(r["probs"].float())
            labels.append(y.to(device))
    preds_dev, labels_dev = torch.cat(preds), torch.cat(labels)
    preds_host, labels_host = preds_dev.cpu().numpy(), labels_dev.cpu().numpy()
    m = calculate_classification_metrics(preds_host, labels_host)
    if tta is not None:
        m["tta_views"] = len(cls_tta.views)
        m["tta_agreement"] = float(torch.cat(agree).double().mean().cpu()) / m["tta_views"] * 100
    if auc:
        from utils.ranking import calibration as calibration_figures, rank_metrics
        y = torch.cat(labels).to(torch.int32)
        scores = torch.cat(kept_scores)
        if calibration is not None:
            from utils.calibrate import apply_temperature, nll_at
            nll_cal = nll_at(scores, y, calibration)
            scores = apply_temperature(scores, calibration)
        cal = calibration_figures(scores, y, bins=calibration_bins, is_prob=tta is not None)
        rk = rank_metrics(cal["scores_t"], labels=y)
        m["auroc_per_class"] = rk["auroc"].cpu().numpy()
        m["ap_per_class"] = rk["average_precision"].cpu().numpy()
        m["auroc"], m["auc_classes"] = _nanmean(m["auroc_per_class"])
        m["average_precision"] = _nanmean(m["ap_per_class"])[0]
        m["ece"], m["brier"], m["nll"] = float(cal["ece"].cpu()), float(cal["brier"].cpu()), float(cal["nll"].cpu())
        if calibration is not None:
            m["nll"] = float(nll_cal.cpu())
    if calibration is not None:
        m["temperature"] = float(calibration.temperature)
    d = None
    if ci is not None:
        from statistics import NormalDist
        from utils import resample
        p_dev, y_dev = preds_dev.to(torch.int32), labels_dev.to(torch.int32)
        # without scores the class ids are taken as they are: the largest one seen, from the arrays the metrics above read back
        classes = cal["scores_t"].shape[0] if auc else int(max(preds_host.max(), labels_host.max())) + 1
        counts = resample.bootstrap_counts(p_dev.shape[0], ci.replicates, ci.seed, device=p_dev.device)
        cls = resample.classification_from_confusion(resample.boot_confusion(p_dev, y_dev, classes, counts)[0])
        names = ["accuracy", "precision", "recall", "f1"]
        cols = [cls[k] for k in names]
        kept = {"pred": p_dev, "labels": y_dev, "accuracy": cls["accuracy"], "scores_t": None, "auroc": None}
        if auc:
            rk_b = resample.boot_rank_metrics(cal["scores_t"], counts, labels=y_dev)
            macro = _nanmean_rows(rk_b["auroc"])
            names += ["auroc", "average_precision"] + [f"auroc_class{c}" for c in range(classes)]
            cols += [macro, _nanmean_rows(rk_b["average_precision"])] + list(rk_b["auroc"].unbind(1))
            var = resample.delong(cal["scores_t"], y_dev)["var"][0]
            kept.update(scores_t=cal["scores_t"], auroc=macro)
            d, var = _intervals(names, torch.stack(cols, 1), ci, extra=var)       # DeLong's variances ride along in the one read-back
        else:
            d = _intervals(names, torch.stack(cols, 1), ci)
        for k in names[:6]:
            m[f"{k}_ci"], m[f"{k}_se"] = (d[k]["lo"], d[k]["hi"]), d[k]["se"]
        if auc:
            per = [d[f"auroc_class{c}"] for c in range(classes)]
            m["auroc_ci_per_class"] = np.array([[e["lo"], e["hi"]] for e in per])
            m["auroc_se_per_class"] = np.array([e["se"] for e in per])
            half = NormalDist().inv_cdf(0.5 + ci.level / 2.0) * np.sqrt(var)
            m["auroc_delong_ci_per_class"] = np.stack([np.clip(m["auroc_per_class"] - half, 0.0, 1.0),
                                                       np.clip(m["auroc_per_class"] + half, 0.0, 1.0)], 1)
        m["ci_detail"], m["ci_replicates"], m["ci_level"], m["ci_seed"] = d, ci.replicates, ci.level, ci.seed
        ci.kept[model_name] = kept
    print(f"\n{model_name} Test Results:\n{'-' * 60}")
    print(f"Accuracy:  {m['accuracy']:.2f}%{_ci_text(d, 'accuracy', '.2f')}\nPrecision: {m['precision']:.2f}%{_ci_text(d, 'precision', '.2f')}\n"
          f"Recall:    {m['recall']:.2f}%{_ci_text(d, 'recall', '.2f')}\nF1 Score:  {m['f1']:.2f}%{_ci_text(d, 'f1', '.2f')}")
    if tta is not None:
        print(f"TTA agreement: {m['tta_agreement']:.2f}% of {m['tta_views']} views")
    if auc:
        print(f"AUROC / AP: {m['auroc']:.4f}{_ci_text(d, 'auroc', '.4f')} / {m['average_precision']:.4f}{_ci_text(d, 'average_precision', '.4f')}"
              f" (macro, one-vs-rest, {m['auc_classes']} classes)")
        print(f"ECE ({calibration_bins} bins) / Brier / NLL: {m['ece']:.4f} / {m['brier']:.4f} / {m['nll']:.4f}")
    if calibration is not None:
        print(f"Calibration: {calibration.describe()}")
    print("\nPer-Class Metrics:")
    for i, c in enumerate(CLASSES[:len(m["f1_per_class"])]):   # (the reference indexes all of CLASSES, tester.py:282-296, and dies when a class is absent)
        delong_text = ""
        if d is not None and auc and i < len(m["auroc_per_class"]):
            delong_text = f"{_ci_text(d, f'auroc_class{i}', '.4f')} (DeLong [{m['auroc_delong_ci_per_class'][i, 0]:.4f}, {m['auroc_delong_ci_per_class'][i, 1]:.4f}])"
        print(f"\n{c}:\n  Precision: {m['precision_per_class'][i]:.2f}%\n  Recall:    {m['recall_per_class'][i]:.2f}%\n"
              f"  F1 Score:  {m['f1_per_class'][i]:.2f}%"
              + (f"\n  AUROC:     {m['auroc_per_class'][i]:.4f}{delong_text}\n  AP:        {m['ap_per_class'][i]:.4f}"
                 if auc and i < len(m["auroc_per_class"]) else ""))
    print("\nConfusion Matrix:")
    print((" " * 25).join(f"{c:>12}" for c in CLASSES))      # the reference's header: names joined by 12 + 1 + 12 blanks (:299)
    for i, row in enumerate(m["confusion_matrix"][:len(CLASSES)]):
        print(f"{CLASSES[i]:<12}" + "".join(f"{v:>12}" for v in row))
    if ci is not None:
        print(ci.footer())
    print(f"{'=' * 60}\n")
    return m


def test_segmentation_model(model, test_loader, device, model_name, surface=False):
    """The segmentation eval loop with the reference's arguments (plus ``surface``): evaluate_segmentation_model without the ranking
    figures, which documents both."""
    return evaluate_segmentation_model(model, test_loader, device, model_name, surface=surface)


def evaluate_segmentation_model(model, test_loader, device, model_name, surface=False, auc=False):
    """The segmentation eval loop with ``auc``, under the argument list its callers know: evaluate_segmentation_model_ci without bootstrap
    intervals, which documents every option."""
    return evaluate_segmentation_model_ci(model, test_loader, device, model_name, surface=surface, auc=auc)


def evaluate_segmentation_model_ci(model, test_loader, device, model_name, surface=False, auc=False, ci=None, calibration=None):
    """``surface=True`` adds hausdorff, hd95, assd (pixels; mean over the samples where both masks have a border), surface_dice
    (%, tolerance 2 pixels) and surface_samples (how many samples entered those means) behind the six overlap metrics.
    Test-time augmentation: pass ``utils.tta.TTASegmenter(model, views, merge)`` as the model.  Every metric is then taken from the
    views' merged map — the mean probability (``merge="prob"``) or the mean logit (``"logit"``) — and the result gains
    ``tta_unanimous`` (%, the pixels on which every view that sees them votes alike; mean over the samples) and ``tta_views``.
    ``auc=True`` (this function only: test_segmentation_model keeps the argument list its callers know) adds ``pixel_auroc`` and
    ``pixel_ap`` (fractions in [0, 1]): ROC-AUC and average precision of each image's pixel scores against ``masks > 0.5``, one ranking call per batch (utils/ranking.py), averaged over the samples where they are defined —
    ``auc_samples`` of them: an image without a positive pixel (or without a negative one) has no ROC-AUC and is counted out.  The LOGITS
    are ranked: the sigmoid is monotone, so the order, the ties that matter and with them every figure are those of the probabilities
    in exact arithmetic, and nothing passes through expf.  With test-time augmentation the merged map is ranked — with
    ``merge="prob"`` the merged probabilities.
    Sliding-window inference: pass ``utils.sliding.SlidingWindowSegmenter(model, tile, overlap, weighting, merge)`` as the model (the
    loader's images are then larger than the tile).  Every metric is taken from the windows' blended map, and the result gains
    ``sw_tiles`` (windows per image) and ``sw_seam_spread`` (per sample the mean, over the pixels more than one window covers, of the
    largest minus the smallest value the windows give the pixel — logits, or probabilities for ``merge="prob"``; 0 for a sample
    without such pixels; averaged over the samples).
    ``ci`` (a ``CI``, or the number of bootstrap replicates): the per-sample values formed after the read-back — the six overlap
    metrics, with ``surface`` the four surface metrics, with ``auc`` the pixel ROC-AUC and average precision — go back to the device
    once as [M, n] doubles and their NaN-aware means are bootstrapped over the images (utils/resample.py).  The result gains
    ``<key>_ci`` = (lo, hi) and ``<key>_se`` for each of them, ``ci_detail`` ({key: point, mean, se, lo, hi, valid}; ``point`` is the
    same fold on the identity resample, equal to the plain figure up to the order of the additions) and ``ci_replicates`` /
    ``ci_level`` / ``ci_seed``; every printed figure its `` [lo, hi]``.
    ``calibration`` (a ``utils.calibrate.Calibration`` of kind "segmentation", trainer.py --calibrate): its threshold takes the place
    of 0.5 in the overlap counters and the surface metrics (the binary masks of the loaders are the same under either); the result
    gains ``threshold`` and one line is printed.  Hand a TTASegmenter / SlidingWindowSegmenter the same ``thr``."""
    from utils.sliding import SlidingWindowSegmenter
    from utils.tta import TTASegmenter
    ci = _check_ci(ci)
    model.eval()
    tta = seg_tta = model if isinstance(model, TTASegmenter) else None
    sw = model if isinstance(model, SlidingWindowSegmenter) else None
    if calibration is not None and calibration.kind != "segmentation":
        raise ValueError(f"a segmenter's calibration is expected, got one of kind {calibration.kind!r}")
    thr = 0.5 if calibration is None else float(np.float32(calibration.threshold))
    is_logit = True                               # the model's output; with tta the merged map, a probability unless merge="logit"
    if tta is not None:
        tta_merge = seg_tta.merge
        is_logit = tta_merge == "logit"
    if sw is not None:
        is_logit = sw.merge == "logit"
    seam, sw_tiles = [], 0
    tot = {k: 0.0 for k in ("iou", "dice", "pixel_accuracy", "precision", "recall", "f1")}
    n = 0
    print(f"\n{'=' * 60}\nTesting Segmentation Model: {model_name}\n{'=' * 60}")
    pending, unanimous, ranked = [], [], []
    if auc:
        from utils.ranking import rank_metrics
    with torch.no_grad():
        for images, masks in test_loader:
            if sw is not None:
                r = sw(images.to(device))
                out = r["mean"]
                over = r["cover"] > 1
                seam.append((r["spread"].double() * over).flatten(1).sum(1) / over.sum().clamp(min=1))
                gy, gx = sw.grid(images.shape[-2], images.shape[-1])
                sw_tiles = len(gy) * len(gx)
            elif tta is None:
                out = model(images.to(device))
            else:
                r = seg_tta(images.to(device))
                out = r["mean"]
                unanimous.append(((r["votes"] == 0) | (r["votes"] == r["valid"])).flatten(1).double().mean(1))
            if out.dim() == 3:
                out = out.unsqueeze(1)
            masks = masks.to(device)
            B, per = out.shape[0], out[0].numel()
            cnt = torch.empty(B, 4, dtype=torch.float32, device=out.device)
            lib.mi355_seg_counts(out.float().contiguous(), masks.float().contiguous(), cnt, B, per, 1 if is_logit else 0, thr)
            pending.append((cnt, per, _surface_raw(out, masks, is_logit, thr, 95, 4) if surface else None))
            if auc:
                rk = rank_metrics(out.float().reshape(B, per), target=masks.float().reshape(B, per), threshold=0.5)
                ranked.append((rk["auroc"], rk["average_precision"]))
    surf, rows = [], []
    if tta is not None:                           # read back with the counters below
        unanimous = torch.cat(unanimous).cpu().numpy()
    if sw is not None:
        seam = torch.cat(seam).cpu().numpy()
    for cnt, per, raw in pending:                 # single read-back after the loop
        for c in cnt.double().cpu().numpy():
            m = _metrics_from_counts(c, per)
            for k in tot:
                tot[k] += m[k]
            if ci is not None:
                rows.append([m[k] for k in tot])
            n += 1
        if raw is not None:
            surf.append(_surface_from_raw(raw[0].cpu().numpy(), raw[1].cpu().numpy(), 1.0, 95))
    avg = {k: v / n for k, v in tot.items()}
    if surface:
        per_sample = {k: np.concatenate([s[k] for s in surf]) for k in SURFACE_KEYS}
        ok = ~np.isnan(per_sample["hausdorff"])
        for k in SURFACE_KEYS:
            avg[k] = float(per_sample[k][ok].mean()) * (100.0 if k == "surface_dice" else 1.0) if ok.any() else float("nan")
        avg["surface_samples"] = int(ok.sum())
    if auc:                                       # read back with the counters above
        avg["pixel_auroc"], avg["auc_samples"] = _nanmean(torch.cat([a for a, _ in ranked]).cpu().numpy())
        avg["pixel_ap"] = _nanmean(torch.cat([p for _, p in ranked]).cpu().numpy())[0]
    d = None
    if ci is not None:
        from utils import resample
        names, values = list(tot), [np.asarray(rows, dtype=np.float64).T]
        if surface:                               # NaN where a sample has no surface distances: counted out of every replicate's mean
            names += list(SURFACE_KEYS)
            values.append(np.stack([per_sample[k] * (100.0 if k == "surface_dice" else 1.0) for k in SURFACE_KEYS]))
        per_dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(values))).to(device)
        if auc:
            names += ["pixel_auroc", "pixel_ap"]
            per_dev = torch.cat([per_dev, torch.cat([a for a, _ in ranked]).view(1, -1), torch.cat([p for _, p in ranked]).view(1, -1)])
        counts = resample.bootstrap_counts(n, ci.replicates, ci.seed, device=per_dev.device)
        reps = resample.boot_means(per_dev, counts)
        d = _intervals(names, reps, ci)
        for k in names:
            avg[f"{k}_ci"], avg[f"{k}_se"] = (d[k]["lo"], d[k]["hi"]), d[k]["se"]
        avg["ci_detail"], avg["ci_replicates"], avg["ci_level"], avg["ci_seed"] = d, ci.replicates, ci.level, ci.seed
        ci.kept[model_name] = {"dice_values": per_dev[names.index("dice")], "dice": reps[:, names.index("dice")]}
    if tta is not None:
        avg["tta_unanimous"] = float(unanimous.mean()) * 100
        avg["tta_views"] = len(seg_tta.views)
    if sw is not None:
        avg["sw_tiles"] = int(sw_tiles)
        avg["sw_seam_spread"] = float(seam.mean())
    if calibration is not None:
        avg["threshold"] = thr
    print(f"\n{model_name} Test Results:\n{'-' * 60}")
    b = lambda key, fmt=".2f": _ci_text(d, key, fmt)      # noqa: E731  ('' without ci)
    print(f"IoU (Jaccard):     {avg['iou']:.2f}%{b('iou')}\nDice Coefficient:  {avg['dice']:.2f}%{b('dice')}\n"
          f"Pixel Accuracy:    {avg['pixel_accuracy']:.2f}%{b('pixel_accuracy')}")
    print(f"Precision:         {avg['precision']:.2f}%{b('precision')}\nRecall:            {avg['recall']:.2f}%{b('recall')}\n"
          f"F1 Score:          {avg['f1']:.2f}%{b('f1')}"
          + (f"\nHausdorff:         {avg['hausdorff']:.2f} px{b('hausdorff')}\nHD95:              {avg['hd95']:.2f} px{b('hd95')}\n"
             f"ASSD:              {avg['assd']:.2f} px{b('assd')}\n"
             f"Surface Dice @2px: {avg['surface_dice']:.2f}%{b('surface_dice')} ({avg['surface_samples']} of {n} samples)" if surface else "")
          + (f"\nPixel AUROC / AP:  {avg['pixel_auroc']:.4f}{b('pixel_auroc', '.4f')} / {avg['pixel_ap']:.4f}{b('pixel_ap', '.4f')} "
             f"({avg['auc_samples']} of {n} samples)" if auc else "")
          + (f"\nTTA unanimous:     {avg['tta_unanimous']:.2f}% of the pixels ({avg['tta_views']} views, merged {tta_merge})" if tta is not None else "")
          + (f"\nSliding window:    {avg['sw_tiles']} tiles of {sw.tile} px per image (overlap {sw.overlap:g}, {sw.weighting} weights, merged "
             f"{sw.merge}), seam spread {avg['sw_seam_spread']:.4f}" if sw is not None else "")
          + (f"\nCalibration:       {calibration.describe()}" if calibration is not None else "")
          + (f"\n{ci.footer()}" if ci is not None else "")
          + f"\n{'=' * 60}\n")
    return avg


# ---- the whole-zoo driver and its reports (tester.py:513-876) -------------------------------------------------------
_CLS_FILES = {"ResNet18": "ResNet18_best_acc.pt", "ResNet50": "ResNet50_best_acc.pt", "VGG16": "VGG16_best_acc.pt",
              "VGG19": "VGG19_best_acc.pt", "CLIP": "CLIP_best_acc.pt"}
_SEG_FILES = {"ResNetUnet": "ResNetUnet_best_loss.pt", "AttentionUNet": "AttentionUNet_best_loss.pt",
              "R2Unet": "R2Unet_best_loss.pt", "R2AttUnet": "R2AttUnet_best_loss.pt", "CLIPSeg": "CLIPSeg_best_loss.pt"}
WEIGHTS_VARIANTS = ("raw", "ema", "swa")


def variant_files(files, variant):
    """_CLS_FILES / _SEG_FILES for a weights variant: "raw" is the table itself; "ema" / "swa" name the averaged checkpoints
    train(model, WithAveraging(train_dl, ...), ...) writes beside the raw ones ({name}_ema_best_acc.pt / {name}_ema_best_loss.pt, {name}_swa.pt)."""
    if variant not in WEIGHTS_VARIANTS:
        raise ValueError(f"weights_variant must be one of {WEIGHTS_VARIANTS}, got {variant!r}")
    if variant == "raw":
        return files
    if variant == "ema":
        return {m: f.replace("_best_", "_ema_best_") for m, f in files.items()}
    return {m: f.rsplit("_best_", 1)[0] + "_swa.pt" for m, f in files.items()}


def check_multiclass_options(seg_classes, surface=False, tta=None, sliding=None, auc=False, ci=None, calibration=None):
    """seg_classes > 1 (tester.py --seg-classes) next to an option that is defined for one foreground: ValueError naming it."""
    seg_classes = int(seg_classes)
    if not 1 <= seg_classes <= 16:
        raise ValueError(f"seg_classes must lie in [1, 16], got {seg_classes}")
    if seg_classes == 1:
        return seg_classes
    bad = [name for name, on in (("--surface", surface), ("--tta", tta is not None), ("--sw-tile", sliding is not None), ("--auc", auc),
                                 ("--ci", ci is not None and ci != 0), ("--calibration", calibration is not None)) if on]
    if bad:
        raise ValueError(f"--seg-classes {seg_classes}: {', '.join(bad)} {'is' if len(bad) == 1 else 'are'} defined for binary "
                         "segmentation only (one foreground) and not supported with more than one class")
    return seg_classes


def evaluate_multiclass_segmentation_model(model, test_loader, device, model_name, num_classes, ignore_index=255, class_names=None):
    """The segmentation eval loop for a K-channel model and class-index masks (uint8 [N, H, W]; ``ignore_index`` and every other
    label >= K are left out): one argmax / confusion launch per batch (utils/multiclass.py), one read-back after the loop.  Returns
    percentages like the binary loop: ``dice`` / ``iou`` (the means over the classes of the per-class means over the images — a
    class in neither mask of an image is NaN there and counted out), ``pixel_accuracy``, ``dice_per_class`` / ``iou_per_class``
    (lists in class order), and ``num_classes``, ``class_names``, ``samples``, ``confusion_matrix`` ([K][K] integers, label x
    prediction, summed over the images)."""
    from utils.multiclass import check_class_names, confusion_batch, metrics_from_confusion
    num_classes = int(num_classes)
    names = check_class_names(class_names, num_classes)
    model.eval()
    print(f"\n{'=' * 60}\nTesting Segmentation Model: {model_name} ({num_classes} classes)\n{'=' * 60}")
    pending = []
    with torch.no_grad():
        for images, masks in test_loader:
            out = model(images.to(device))
            if out.dim() < 4 or out.shape[1] != num_classes:
                raise ValueError(f"{model_name}: logits [N, {num_classes}, H, W] expected, got {tuple(out.shape)}")
            pending.append(confusion_batch(out, masks.to(device), ignore_index))
    if not pending:
        raise ValueError("the test loader is empty")
    conf = torch.cat(pending).cpu().numpy()           # single read-back after the loop
    result = multiclass_result(metrics_from_confusion(conf), names, conf.shape[0])
    for line in _multiclass_lines(result):
        print(line)
    return result


def multiclass_result(m, class_names, samples):
    """metrics_from_confusion's fractions -> the result dictionary of evaluate_multiclass_segmentation_model (percentages)."""
    return {"iou": 100.0 * m["mean_iou"], "dice": 100.0 * m["mean_dice"], "pixel_accuracy": 100.0 * m["pixel_accuracy"],
            "num_classes": len(class_names), "class_names": list(class_names), "samples": int(samples),
            "dice_per_class": [100.0 * float(v) for v in m["dice_per_class"]],
            "iou_per_class": [100.0 * float(v) for v in m["iou_per_class"]],
            "confusion_matrix": np.asarray(m["confusion_matrix"]).tolist()}


def _multiclass_lines(r):
    lines = [f"Mean IoU:       {r['iou']:.2f}%", f"Mean Dice:      {r['dice']:.2f}%", f"Pixel Accuracy: {r['pixel_accuracy']:.2f}%",
             f"{'Class':<20} {'IoU':<10} {'Dice':<10}"]
    lines += [f"{n:<20} {i:>8.2f}% {d:>8.2f}%" for n, i, d in zip(r["class_names"], r["iou_per_class"], r["dice_per_class"])]
    return lines


def test_all_models(device="cuda", batch_size=16, cls_loader=None, seg_loader=None, cls_weights_dir=None,
                    seg_weights_dir=None, clahe=None, tta=None, tta_merge="prob", sliding=None, size=None, ci=None, calibration=None,
                    seg_classes=1, seg_ignore_index=255, class_names=None, weights_variant="raw", auc=False, calibration_bins=15, surface=False):
    """Evaluate every checkpoint found under the weights directories (tester.py:513-735): same model names, file
    names, skip rules and result dictionary.  Like the reference (:531-555, :569-580, :651-666) the test loaders are built
    from ``DATA_ROOT/splits/test.csv`` with the validation transforms — here `utils.dataset` + `GpuBatchLoader` (native PNG
    decode, transforms on the GPU), batch_size for classification and batch_size // 2 for segmentation (:663); a caller may pass
    its own loaders instead, and when neither exists the reference's "dataset not found" branch is taken (:637-639, :729-731).
    The CLIP / CLIPSeg entries (hub models, out of scope: SURVEY.md section 8) are reported and skipped.  Checkpoints are the
    reference's own format: a plain `state_dict` saved by `train` (helpers.py:394-400).  ``surface=True`` adds the surface-distance
    metrics to every segmentation result (test_segmentation_model).  ``clahe=(clip, grid)``: the default loaders' transforms equalise
    the images (utils/clahe.py) — pass what the checkpoints were trained with (trainer.py --clahe-clip / --clahe-grid).  ``tta`` /
    ``tta_merge``: test-time augmentation for every model (test_classification_model(tta=...); the segmenters are handed to
    test_segmentation_model wrapped in utils.tta.TTASegmenter).  ``auc`` / ``calibration_bins``: ROC-AUC, average precision and
    calibration for every classifier (test_classification_model(auc=True)), per-image pixel ROC-AUC and average precision for every
    segmenter (evaluate_segmentation_model(auc=True)).  ``sliding=(tile, overlap, weighting)``: the segmenters are handed on wrapped in
    utils.sliding.SlidingWindowSegmenter (windows of ``tile`` pixels blended on the GPU; the classifiers are untouched), and ``size``
    (default IMG_SIZE, at least ``tile``) is the side the default SEGMENTATION loader resizes to (the classifiers keep IMG_SIZE) — the
    point of the option is a ``size`` above the training size with ``tile`` at the training size.  ``sliding`` together with ``tta``: ValueError.
    ``ci`` (a ``CI``, the number of bootstrap replicates, or (replicates, level, seed)): every figure of every model gets its
    bootstrap interval (the ``ci`` of the two loops).  All models share the seed, hence the resamples, and what ``print_paired_tests``
    needs stays on the device in ``ci.kept`` — pass a ``CI`` to have it afterwards.
    ``calibration`` (a directory): every model that is tested is given its sidecar ``{name}_calibration.json`` (utils/calibrate.py,
    written by trainer.py --calibrate) from that directory or its ``classification_models`` / ``segmentation_models`` sub-directory:
    the classifiers' temperature (with ``auc``: their ECE, Brier score and NLL are the calibrated ones; not together with ``tta``),
    the segmenters' threshold in place of 0.5 (also in the TTA and sliding-window folds).  A checkpoint without a sidecar:
    FileNotFoundError naming the file.
    ``seg_classes`` K > 1 (with ``seg_ignore_index``, ``class_names``): the segmenters are built with K-channel heads, the default
    segmentation loader yields class-index masks (SegmentationDataset(labels=True)) and every segmenter goes through
    evaluate_multiclass_segmentation_model; the binary-only options (check_multiclass_options) raise ValueError.
    ``weights_variant`` "ema" / "swa": the averaged checkpoints of train(model, WithAveraging(train_dl, ...), ...) are tested in place of the raw ones
    (variant_files); a model without such a file is skipped like any model without weights.  Pass it BY KEYWORD: it stands in front
    of ``auc`` / ``calibration_bins`` / ``surface`` in the parameter list (tests pin those three as its tail), so a positional call
    that reaches past ``class_names`` would shift; a value that is not one of the three names raises ValueError."""
    from utils.helpers import get_class_model, get_seg_model
    cls_files, seg_files = variant_files(_CLS_FILES, weights_variant), variant_files(_SEG_FILES, weights_variant)
    seg_classes = check_multiclass_options(seg_classes, surface, tta, sliding, auc, ci, calibration)
    ci = _check_ci(ci)
    size = IMG_SIZE if size is None else int(size)
    if size < 1:
        raise ValueError(f"size >= 1 required, got {size}")
    if sliding is not None:
        from utils.sliding import check_sliding
        if tta is not None:
            raise ValueError("sliding together with tta is not supported: pass one of the two")
        sliding = check_sliding(sliding)
        if size < sliding[0]:
            raise ValueError(f"sliding: size must be at least the tile ({sliding[0]}), got {size}")
    if tta is not None:
        from utils.tta import MERGES, check_views
        tta = check_views(tta)
        if tta_merge not in MERGES:
            raise ValueError(f"tta_merge must be one of {MERGES}, got {tta_merge!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("test_all_models: the MI355X path needs a GPU (the reference falls back to the CPU, tester.py:524)")
    device = torch.device(device)
    print(f"[INFO] Using device: {device}")
    cls_weights_dir = CLS_WEIGHTS_DIR if cls_weights_dir is None else cls_weights_dir
    seg_weights_dir = SEG_WEIGHTS_DIR if seg_weights_dir is None else seg_weights_dir
    results = {}
    cals = {}                                     # model name -> its Calibration (calibration is a directory)

    def run(files, wdir, loader, build, test, n_samples_label):
        print(f"\n[INFO] {n_samples_label} Test Dataset: {len(loader.dataset)} samples")
        for model_name, weight_file in files.items():
            weight_path = os.path.join(wdir, weight_file)
            if not os.path.exists(weight_path):
                print(f"\n[WARNING] Weights not found for {model_name}: {weight_path}")
                print(f"Skipping {model_name}...")
                continue
            if model_name in ("CLIP", "CLIPSeg"):
                print(f"\n[WARNING] {model_name} is a hub model outside the MI355X conv path; skipping {weight_path}")
                continue
            if calibration is not None:
                from utils.calibrate import find_sidecar
                # (an averaged checkpoint has a sidecar of its own, {name}_{variant}_calibration.json: trainer.py --calibrate)
                tag = model_name if weights_variant == "raw" else f"{model_name}_{weights_variant}"
                cals[model_name] = find_sidecar(calibration, tag, n_samples_label.lower() + "_models")
            try:
                model = build(model_name)
                model.load_state_dict(torch.load(weight_path, map_location=device))
                model = model.to(device)
                results[model_name] = test(model, loader, device, model_name)
                del model
                torch.cuda.empty_cache()
            except Exception as e:      # (the reference reports and moves on to the next model, :630-635)
                print(f"\n[ERROR] Failed to test {model_name}: {e}")
                import traceback
                traceback.print_exc()
                continue

    def default_loader(seg):
        """test split of DATA_ROOT through the GPU input pipeline, or None (split file / directory absent)"""
        try:
            from utils.dataset import ClassificationDataset, GpuBatchLoader, SegmentationDataset
            from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
            if seg:
                if seg_classes > 1:
                    ds = SegmentationDataset(DATA_ROOT, SegBatchTransform(size, train=False, device=device, clahe=clahe, labels=True),
                                             split="test", labels=True)
                else:
                    ds = SegmentationDataset(DATA_ROOT, SegBatchTransform(size, train=False, device=device, clahe=clahe), split="test")
                return GpuBatchLoader(ds, max(1, batch_size // 2), shuffle=False, device=device)
            ds = ClassificationDataset(DATA_ROOT, ClsBatchTransform(IMG_SIZE, train=False, device=device, clahe=clahe), split="test")
            return GpuBatchLoader(ds, batch_size, shuffle=False, device=device)
        except FileNotFoundError:
            return None

    if cls_loader is None:
        cls_loader = default_loader(False)
    if seg_loader is None:
        seg_loader = default_loader(True)
    if cls_loader is None:
        print(f"\n[WARNING] Classification test dataset not found: no loader given for {DATA_ROOT!r}")
        print("Skipping classification model testing...")
    else:
        cls_test = (lambda m, l, d, name: test_classification_model(m, l, d, name, tta=tta)) if tta is not None else test_classification_model
        if auc:
            cls_test = lambda m, l, d, name: test_classification_model(m, l, d, name, tta=tta, auc=True, calibration_bins=calibration_bins)  # noqa: E731
        if ci is not None:
            cls_test = lambda m, l, d, name: evaluate_classification_model(m, l, d, name, tta=tta, auc=auc, calibration_bins=calibration_bins, ci=ci)  # noqa: E731
        if calibration is not None:
            cls_test = lambda m, l, d, name: evaluate_classification_model(m, l, d, name, tta=tta, auc=auc, calibration_bins=calibration_bins, ci=ci, calibration=cals[name])  # noqa: E731
        run(cls_files, cls_weights_dir, cls_loader, lambda n: get_class_model(n)[0], cls_test, "Classification")
    if seg_loader is None:
        print(f"\n[WARNING] Segmentation test dataset not found: no loader given for {DATA_ROOT!r}")
        print("Skipping segmentation model testing...")
    elif len(seg_loader.dataset) == 0:
        print("\n[WARNING] Segmentation test dataset is empty. Skipping segmentation testing.")
    else:
        seg_test = (lambda m, l, d, name: test_segmentation_model(m, l, d, name, surface=True)) if surface else test_segmentation_model
        if tta is not None:
            from utils.tta import TTASegmenter
            seg_test = lambda m, l, d, name: test_segmentation_model(TTASegmenter(m, tta, tta_merge), l, d, name, surface=surface)  # noqa: E731
        if auc:
            wrap = (lambda m: TTASegmenter(m, tta, tta_merge)) if tta is not None else (lambda m: m)
            seg_test = lambda m, l, d, name: evaluate_segmentation_model(wrap(m), l, d, name, surface=surface, auc=True)  # noqa: E731
        if sliding is not None:                          # (tta is None here)
            from utils.sliding import SlidingWindowSegmenter
            sw_batch = max(1, batch_size // 2)
            sw_wrap = lambda m: SlidingWindowSegmenter(m, sliding[0], sliding[1], sliding[2], batch=sw_batch)  # noqa: E731
            seg_test = lambda m, l, d, name: evaluate_segmentation_model(sw_wrap(m), l, d, name, surface=surface, auc=auc)  # noqa: E731
        if ci is not None:
            if sliding is not None:
                seg_wrap = sw_wrap
            elif tta is not None:
                seg_wrap = lambda m: TTASegmenter(m, tta, tta_merge)  # noqa: E731
            else:
                seg_wrap = lambda m: m  # noqa: E731
            seg_test = lambda m, l, d, name: evaluate_segmentation_model_ci(seg_wrap(m), l, d, name, surface=surface, auc=auc, ci=ci)  # noqa: E731
        if calibration is not None:
            def seg_test(m, l, d, name):
                t = float(np.float32(cals[name].threshold))
                if sliding is not None:
                    m = SlidingWindowSegmenter(m, sliding[0], sliding[1], sliding[2], thr=t, batch=sw_batch)
                elif tta is not None:
                    m = TTASegmenter(m, tta, tta_merge, t)
                return evaluate_segmentation_model_ci(m, l, d, name, surface=surface, auc=auc, ci=ci, calibration=cals[name])
        seg_build = get_seg_model
        if seg_classes > 1:
            seg_build = lambda n: get_seg_model(n, classes=seg_classes)  # noqa: E731
            seg_test = lambda m, l, d, name: evaluate_multiclass_segmentation_model(m, l, d, name, seg_classes, seg_ignore_index, class_names)  # noqa: E731
        run(seg_files, seg_weights_dir, seg_loader, seg_build, seg_test, "Segmentation")
    return results


def print_summary(results):
    """The two result tables and the best model of each family (tester.py:738-805), same text."""
    if not results:
        print("\n[INFO] No test results to display.")
        return
    print("\n" + "=" * 80)
    print(" " * 25 + "TEST RESULTS SUMMARY")
    print("=" * 80)
    cls_models = [m for m in ["ResNet18", "ResNet50", "VGG16", "VGG19", "CLIP"] if m in results]
    if cls_models:
        print("\nCLASSIFICATION MODELS:")
        print("-" * 80)
        print(f"{'Model':<20} {'Accuracy':<12} {'Precision':<12} {'Recall':<12} {'F1 Score':<12}")
        print("-" * 80)
        for model in cls_models:
            m = results[model]
            print(f"{model:<20} {m['accuracy']:>10.2f}% {m['precision']:>10.2f}% {m['recall']:>10.2f}% {m['f1']:>10.2f}%")
        best = max(cls_models, key=lambda x: results[x]["accuracy"])
        print(f"\n\U0001F3C6 Best Classification Model: {best} (Accuracy: {results[best]['accuracy']:.2f}%)")
        rank_models = [m for m in cls_models if all(k in results[m] for k in ("auroc", "average_precision", "ece", "brier", "nll"))]
        if rank_models:                                     # (only after test_all_models(auc=True))
            print("\n\nCLASSIFICATION MODELS, RANKING AND CALIBRATION (macro one-vs-rest AUROC / AP):")
            print("-" * 80)
            print(f"{'Model':<20} {'AUROC':<10} {'AP':<10} {'ECE':<10} {'Brier':<10} {'NLL':<10}")
            print("-" * 80)
            for model in rank_models:
                m = results[model]
                print(f"{model:<20} {m['auroc']:>8.4f}   {m['average_precision']:>8.4f}   {m['ece']:>8.4f}   {m['brier']:>8.4f}   {m['nll']:>8.4f}")
    seg_all = [m for m in ["ResNetUnet", "AttentionUNet", "R2Unet", "R2AttUnet", "CLIPSeg"] if m in results]
    mc_models = [m for m in seg_all if "num_classes" in results[m]]      # (only after test_all_models(seg_classes=K > 1))
    seg_models = [m for m in seg_all if m not in mc_models]
    for line in multiclass_summary_lines(results, mc_models):
        print(line)
    if seg_models:
        print("\n\nSEGMENTATION MODELS:")
        print("-" * 80)
        print(f"{'Model':<20} {'IoU':<10} {'Dice':<10} {'Precision':<12} {'Recall':<12} {'F1 Score':<12}")
        print("-" * 80)
        for model in seg_models:
            m = results[model]
            print(f"{model:<20} {m['iou']:>8.2f}% {m['dice']:>8.2f}% {m['precision']:>10.2f}% {m['recall']:>10.2f}% {m['f1']:>10.2f}%")
        best = max(seg_models, key=lambda x: results[x]["dice"])
        print(f"\n\U0001F3C6 Best Segmentation Model: {best} (Dice: {results[best]['dice']:.2f}%)")
        surf_models = [m for m in seg_models if all(k in results[m] for k in SURFACE_KEYS)]
        if surf_models:                                     # (only after test_all_models(surface=True))
            print("\n\nSEGMENTATION MODELS, SURFACE DISTANCES (pixels; surface Dice at 2 px):")
            print("-" * 80)
            print(f"{'Model':<20} {'Hausdorff':<12} {'HD95':<12} {'ASSD':<12} {'Surface Dice':<14} {'Samples':<8}")
            print("-" * 80)
            for model in surf_models:
                m = results[model]
                print(f"{model:<20} {m['hausdorff']:>10.2f}   {m['hd95']:>10.2f}   {m['assd']:>10.2f}   {m['surface_dice']:>11.2f}%   "
                      f"{m.get('surface_samples', ''):>7}")
        rank_models = [m for m in seg_models if "pixel_auroc" in results[m] and "pixel_ap" in results[m]]
        if rank_models:                                     # (only after test_all_models(auc=True))
            print("\n\nSEGMENTATION MODELS, PIXEL RANKING (mean over the images):")
            print("-" * 80)
            print(f"{'Model':<20} {'Pixel AUROC':<14} {'Pixel AP':<12} {'Samples':<8}")
            print("-" * 80)
            for model in rank_models:
                m = results[model]
                print(f"{model:<20} {m['pixel_auroc']:>11.4f}   {m['pixel_ap']:>9.4f}   {m.get('auc_samples', ''):>7}")
    print("=" * 80 + "\n")


def multiclass_summary_lines(results, models):
    """The multi-class table of print_summary: one row of means per model, then each model's per-class IoU / Dice."""
    if not models:
        return []
    lines = ["\n\nSEGMENTATION MODELS, MULTI-CLASS (means over the classes):", "-" * 80,
             f"{'Model':<20} {'Classes':<8} {'mIoU':<10} {'mDice':<10} {'Pixel Acc':<12} {'Samples':<8}", "-" * 80]
    for model in models:
        m = results[model]
        lines.append(f"{model:<20} {m['num_classes']:>7} {m['iou']:>8.2f}% {m['dice']:>8.2f}% {m['pixel_accuracy']:>10.2f}% {m.get('samples', ''):>7}")
    best = max(models, key=lambda x: results[x]["dice"])
    lines.append(f"\n\U0001F3C6 Best Segmentation Model: {best} (Mean Dice: {results[best]['dice']:.2f}%)")
    for model in models:
        m = results[model]
        lines += [f"\n{model}, per class (IoU / Dice):"]
        lines += [f"  {n:<18} {i:>8.2f}% {d:>8.2f}%" for n, i, d in zip(m["class_names"], m["iou_per_class"], m["dice_per_class"])]
    return lines


def print_paired_tests(results, ci):
    """After ``test_all_models(ci=CI(...))`` (or the two loops with one ``CI``): every model against the best of its task ON THE SAME
    RESAMPLES, so the differences are paired.  Classifiers: the accuracy difference (percentage points) with its bootstrap interval
    and McNemar's exact p; with ``auc`` the macro-AUROC difference with its interval and DeLong's p per class ("identical" where the
    two rankings give a zero variance of the difference).  Segmenters: the Dice difference with its interval.  Returns the rows:
    {(model, best): {"d_accuracy", "d_accuracy_ci", "mcnemar", "d_auroc", "d_auroc_ci", "delong", "d_dice", "d_dice_ci"}}."""
    from utils import resample
    ci = _check_ci(ci)
    rows = {}
    if ci is None or not ci.kept:
        return rows
    fmt = lambda dd, f: f"{dd['point']:+{f}} [{dd['lo']:+{f}}, {dd['hi']:+{f}}]"      # noqa: E731
    cls_models = [m for m in results if m in ci.kept and "pred" in ci.kept[m]]
    seg_models = [m for m in results if m in ci.kept and "dice" in ci.kept[m]]
    print("\n" + "=" * 80 + "\n" + " " * 22 + "PAIRED COMPARISONS (same resamples)\n" + "=" * 80)
    if len(cls_models) > 1:
        best = max(cls_models, key=lambda x: results[x]["accuracy"])
        kb = ci.kept[best]
        print(f"\nCLASSIFICATION MODELS against {best}:\n" + "-" * 80)
        for name in cls_models:
            if name == best:
                continue
            k = ci.kept[name]
            diffs, names = [k["accuracy"] - kb["accuracy"]], ["d_accuracy"]
            both_auc = k["auroc"] is not None and kb["auroc"] is not None
            if both_auc:
                diffs.append(k["auroc"] - kb["auroc"])
                names.append("d_auroc")
            d = _intervals(names, torch.stack(diffs, 1), ci)
            mc = resample.mcnemar(k["pred"] == k["labels"], kb["pred"] == kb["labels"])
            row = {"d_accuracy": d["d_accuracy"]["point"], "d_accuracy_ci": (d["d_accuracy"]["lo"], d["d_accuracy"]["hi"]), "mcnemar": mc}
            print(f"{name:<16} accuracy {fmt(d['d_accuracy'], '.2f')} points, McNemar p = {mc['p']:.4g} ({mc['b']} / {mc['c']} discordant)")
            if both_auc:
                row.update(d_auroc=d["d_auroc"]["point"], d_auroc_ci=(d["d_auroc"]["lo"], d["d_auroc"]["hi"]),
                           delong=resample.delong_test(k["scores_t"], kb["scores_t"], k["labels"]))
                per = ", ".join(f"{CLASSES[c] if c < len(CLASSES) else c}: " + ("identical" if t["z"] != t["z"] else f"p = {t['p']:.4g}")
                                for c, t in enumerate(row["delong"]))
                print(f"{'':<16} macro AUROC {fmt(d['d_auroc'], '.4f')}; DeLong {per}")
            rows[(name, best)] = row
    if len(seg_models) > 1:
        best = max(seg_models, key=lambda x: results[x]["dice"])
        print(f"\nSEGMENTATION MODELS against {best}:\n" + "-" * 80)
        for name in seg_models:
            if name == best:
                continue
            d = _intervals(["d_dice"], (ci.kept[name]["dice"] - ci.kept[best]["dice"]).view(-1, 1), ci)["d_dice"]
            rows[(name, best)] = {"d_dice": d["point"], "d_dice_ci": (d["lo"], d["hi"])}
            print(f"{name:<16} Dice {fmt(d, '.2f')} points")
    print(ci.footer() + "\n" + "=" * 80 + "\n")
    return rows


def _csv_row(name, result):
    """scalars only; a ``<key>_ci`` pair becomes the columns ``<key>_lo`` and ``<key>_hi``, a multi-class result's per-class lists
    the columns ``dice_<class name>`` / ``iou_<class name>``"""
    row = {"Model": name}
    for k, v in result.items():
        if k.endswith("_ci") and isinstance(v, tuple):
            row[k[:-3] + "_lo"], row[k[:-3] + "_hi"] = v
        elif k in ("dice_per_class", "iou_per_class") and "class_names" in result:      # multi-class: one column per class
            for n, x in zip(result["class_names"], v):
                row[f"{k[:-10]}_{n}"] = x
        else:
            row[k] = v
    for k in ("confusion_matrix", "class_names", "precision_per_class", "recall_per_class", "f1_per_class", "auroc_per_class", "ap_per_class",
              "ci_detail", "auroc_ci_per_class", "auroc_se_per_class", "auroc_delong_ci_per_class"):
        row.pop(k, None)
    return row


def save_results_to_csv(results, cls_output_path="results/classification_test_results.csv",
                        seg_output_path="results/segmentation_test_results.csv"):
    """One CSV per family, a `Model` column followed by the scalar metrics in dictionary order (tester.py:808-876;
    written through pandas like the reference, so the float formatting is identical)."""
    if not results:
        print("\n[INFO] No results to save.")
        return
    import pandas as pd
    cls_models = [k for k in results.keys() if any(x in k for x in ["ResNet18", "ResNet50", "VGG", "CLIP"]) and "Seg" not in k]
    seg_models = [k for k in results.keys() if "Unet" in k or "UNet" in k or "CLIPSeg" in k]
    if cls_models:
        rows = [_csv_row(name, results[name]) for name in cls_models]
        pd.DataFrame(rows).to_csv(cls_output_path, index=False)
        print(f"\n[INFO] Classification results saved to: {cls_output_path}")
    else:
        print("\n[INFO] No classification results to save.")
    if seg_models:
        rows = [_csv_row(name, results[name]) for name in seg_models]
        pd.DataFrame(rows).to_csv(seg_output_path, index=False)
        print(f"[INFO] Segmentation results saved to: {seg_output_path}")
    else:
        print("\n[INFO] No segmentation results to save.")


def build_parser():
    import argparse
    _ap = argparse.ArgumentParser(description="Test every checkpoint under weights/ on the test split")
    _ap.add_argument("--surface", action="store_true", help="also report Hausdorff, HD95, ASSD and surface Dice of the segmentation models")
    _ap.add_argument("--clahe-clip", type=float, default=0.0,
                     help="CLAHE clip limit the checkpoints were trained with (trainer.py --clahe-clip); 0 = off")
    _ap.add_argument("--clahe-grid", type=int, default=8, help="CLAHE: tiles per side")
    _ap.add_argument("--tta", choices=("hflip", "rot", "full"), default=None,
                     help="test-time augmentation: predict on these views and score the merged prediction (utils/tta.py)")
    _ap.add_argument("--tta-merge", choices=("prob", "logit"), default="prob", help="TTA: average the probabilities or the logits")
    _ap.add_argument("--sw-tile", type=int, default=0,
                     help="sliding-window inference for the segmenters: the window side (the training size); 0 = off (utils/sliding.py)")
    _ap.add_argument("--sw-overlap", type=float, default=0.5, help="sliding window: the share of a window its neighbour overlaps (0 .. 0.75)")
    _ap.add_argument("--sw-weight", choices=("gaussian", "constant"), default="gaussian", help="sliding window: how overlapping windows are weighted")
    _ap.add_argument("--size", type=int, default=IMG_SIZE, help="the side the segmentation test images are resized to (with --sw-tile: at least the tile)")
    _ap.add_argument("--auc", action="store_true",
                     help="also report ROC-AUC and average precision (per class / per image over the pixels) and the classifiers' ECE, Brier score and NLL")
    _ap.add_argument("--calibration-bins", type=int, default=15, help="--auc: confidence bins of the expected calibration error")
    _ap.add_argument("--calibration", default=None, metavar="DIR",
                     help="apply the post-hoc calibration fitted by trainer.py --calibrate: DIR holds the {name}_calibration.json sidecars "
                          "(or the classification_models / segmentation_models directories that do)")
    _ap.add_argument("--ci", type=int, default=0,
                     help="bootstrap replicates (up to 8192) for a percentile interval on every figure and paired tests between the models; 0 = off")
    _ap.add_argument("--ci-level", type=float, default=0.95, help="--ci: the level of the intervals")
    _ap.add_argument("--ci-seed", type=int, default=0, help="--ci: the seed of the resamples (shared by every model)")
    _ap.add_argument("--seg-classes", type=int, default=1,
                     help="K > 1: the segmentation checkpoints have K-channel heads and the masks hold class indices (grey value = class, "
                          "255 = ignore): per-class and mean Dice / IoU, pixel accuracy and the confusion matrix (utils/multiclass.py)")
    _ap.add_argument("--seg-ignore-index", type=int, default=255, help="--seg-classes: the label left out of every count (-1: none)")
    _ap.add_argument("--class-names", default=None, help="--seg-classes: comma-separated names of the K classes, in class order")
    _ap.add_argument("--weights-variant", choices=WEIGHTS_VARIANTS, default="raw",
                     help="which checkpoint of every model to test: raw = {name}_best_*.pt; ema / swa = the averaged weights written by "
                          "trainer.py --ema-decay / --swa-start ({name}_ema_best_*.pt, {name}_swa.pt)")
    return _ap


def multiclass_kwargs(args):
    """tester.py --seg-classes K [--seg-ignore-index] [--class-names]: the keyword arguments of test_all_models ({} for K = 1),
    after the clear error for an option that is binary-only."""
    k = check_multiclass_options(args.seg_classes, args.surface, args.tta, (args.sw_tile or None) and (args.sw_tile,), args.auc,
                                 args.ci, args.calibration)
    if k == 1:
        return {}
    from utils.multiclass import check_class_names
    return {"seg_classes": k, "seg_ignore_index": args.seg_ignore_index, "class_names": check_class_names(args.class_names, k)}


if __name__ == "__main__":          # python utils/tester.py (tester.py:879-898): same banner, same three calls
    _args = build_parser().parse_args()
    _kw = multiclass_kwargs(_args)
    if _args.clahe_clip != 0:
        from utils.clahe import check_clahe
        _kw["clahe"] = check_clahe(_args.clahe_clip, _args.clahe_grid)
    print("\n" + "=" * 80)
    print(" " * 20 + "MODEL TESTING UTILITY")
    print("=" * 80)
    if _args.surface:
        _kw["surface"] = True
    if _args.tta is not None:
        _kw.update(tta=_args.tta, tta_merge=_args.tta_merge)
    if _args.auc:
        _kw.update(auc=True, calibration_bins=_args.calibration_bins)
    if _args.sw_tile != 0:
        if _args.tta is not None:
            raise ValueError("--tta together with --sw-tile is not supported: pass one of the two")
        _kw.update(sliding=(_args.sw_tile, _args.sw_overlap, _args.sw_weight))
    if _args.size != IMG_SIZE:
        _kw["size"] = _args.size
    if _args.ci != 0:
        _kw["ci"] = CI(_args.ci, _args.ci_level, _args.ci_seed)
    if _args.calibration is not None:
        _kw["calibration"] = _args.calibration
    if _args.weights_variant != "raw":
        _kw["weights_variant"] = _args.weights_variant
    results = test_all_models(device="cuda", batch_size=16, **_kw)
    print_summary(results)
    if _args.ci != 0:
        print_paired_tests(results, _kw["ci"])
    save_results_to_csv(results, cls_output_path="classification_test_results.csv", seg_output_path="segmentation_test_results.csv")
    print("\n[INFO] Testing complete!")
