"""Threshold-free evaluation on the device (csrc/ranking.hip): ROC-AUC, average precision, the ROC / precision-recall curves and the
calibration of a classifier (ECE, Brier score, NLL) — what utils/tester.py reports under ``auc=True``, exposed for other uses.

A *segment* is one ranking problem: one image's pixels, or one class of a classifier one-vs-rest.  Scores are ranked by the
deterministic segmented sort of csrc/segsort.hip; equal scores (-0.0 == +0.0) form one tie group, so ROC-AUC counts ties half and the
curves have one point per distinct score, as scikit-learn's do.  The integers (positives, negatives, twice the Mann-Whitney statistic,
distinct scores, the curves' tp / fp) are exact; ROC-AUC is formed from them in double.  NaN scores are not supported as an order.

``rank_metrics`` and ``calibration`` stay on the device: no host round trip, no synchronisation, the same bits on every run.
``binary_curve`` (and ``roc_curve`` / ``precision_recall_curve`` on top of it) returns numpy arrays sliced to each segment's number of
points: that is the one read-back here."""
import numpy as np
import torch

from mi355 import nn as mnn


def _prepare(scores, target, labels, what):
    """-> (scores fp32 [S, len], target fp32 [S, len] or None, labels int32 [len] or None), validated"""
    if (target is None) == (labels is None):
        raise ValueError(f"{what}: exactly one of target and labels is expected ({'both' if target is not None else 'neither'} given)")
    given = target if target is not None else labels
    if not (scores.is_cuda and given.is_cuda):
        raise ValueError(f"{what} is computed on the GPU: device tensors are expected (there is no CPU fallback)")
    if scores.dim() < 1 or scores.numel() == 0:
        raise ValueError(f"{what} expects scores [S, len] or [len], got {tuple(scores.shape)}")
    z = scores.float().contiguous()
    z = z.view(1, -1) if z.dim() == 1 else z.view(z.shape[0], -1)
    if target is not None:
        if target.numel() != z.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match scores size {tuple(scores.shape)}")
        return z, target.float().contiguous().view(z.shape), None
    if labels.dim() != 1 or labels.shape[0] != z.shape[1]:
        raise ValueError(f"labels [len] are shared by the segments of scores [S, len]: got {tuple(labels.shape)} for {tuple(scores.shape)}")
    return z, None, labels.to(torch.int32).contiguous()


def rank_metrics(scores, target=None, labels=None, threshold=0.5):
    """scores [S, len] (or [len], or [B, ...] flattened per sample) with the positives from exactly one of ``target`` (same size,
    positive where ``target > threshold``) and ``labels`` (integers [len] shared by the segments: segment s ranks class s against the
    rest) -> dict of device tensors [S]: ``pos``, ``neg``, ``u2`` (twice the Mann-Whitney statistic, ties half) and ``thresholds_n``
    (distinct scores) as int64, ``auroc`` = u2 / (2 pos neg) and ``average_precision`` (scikit-learn's step-wise sum) as float64, NaN
    where undefined (no positive; for auroc also no negative).  Nothing is read back."""
    z, t, y = _prepare(scores, target, labels, "rank_metrics")
    counts, ap, _ = mnn._rank_metrics(z, t, y, threshold)
    pos, neg, u2 = counts[:, 0], counts[:, 1], counts[:, 2]
    return {"pos": pos, "neg": neg, "u2": u2, "thresholds_n": counts[:, 3],
            "auroc": u2.double() / (2.0 * pos.double() * neg.double()), "average_precision": ap}


def binary_curve(scores, target=None, labels=None, threshold=0.5):
    """-> a list with, per segment, ``(thresholds, tp, fp)``: numpy arrays (fp32, int32, int32) of the segment's distinct scores in
    descending order and the true / false positives at ``score >= threshold`` — what scikit-learn's ``_binary_clf_curve`` returns
    (as ``fps, tps, thresholds``).  Reads the device arrays back, sliced to each segment's number of points."""
    z, t, y = _prepare(scores, target, labels, "binary_curve")
    _, _, (thr, tp, fp, npoints) = mnn._rank_metrics(z, t, y, threshold, curve=True)
    n = npoints.cpu().numpy()
    thr, tp, fp = thr.cpu().numpy(), tp.cpu().numpy(), fp.cpu().numpy()
    return [(thr[s, :n[s]].copy(), tp[s, :n[s]].copy(), fp[s, :n[s]].copy()) for s in range(len(n))]


def roc_from_points(thresholds, tp, fp):
    """(thresholds, tp, fp) of one segment -> (fpr, tpr, thresholds) as ``sklearn.metrics.roc_curve(drop_intermediate=False)`` returns
    them: a leading (0, 0) point with threshold inf; a rate is NaN where its class is absent."""
    tps = np.r_[0, tp].astype(np.float64)
    fps = np.r_[0, fp].astype(np.float64)
    thr = np.r_[np.inf, thresholds].astype(np.asarray(thresholds).dtype)
    fpr = fps / fps[-1] if fps[-1] > 0 else np.full(fps.shape, np.nan)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.full(tps.shape, np.nan)
    return fpr, tpr, thr


def pr_from_points(thresholds, tp, fp):
    """(thresholds, tp, fp) of one segment -> (precision, recall, thresholds) as ``sklearn.metrics.precision_recall_curve`` returns
    them: ascending thresholds, decreasing recall, the final (precision 1, recall 0) point; recall is 1 where there is no positive."""
    tps, fps = np.asarray(tp, dtype=np.float64), np.asarray(fp, dtype=np.float64)
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=ps != 0)
    recall = tps / tps[-1] if tps[-1] > 0 else np.ones_like(tps)
    return np.hstack((precision[::-1], 1.0)), np.hstack((recall[::-1], 0.0)), np.asarray(thresholds)[::-1].copy()


def roc_curve(scores, target=None, labels=None, threshold=0.5):
    """-> per segment ``(fpr, tpr, thresholds)`` with scikit-learn's conventions (roc_from_points)."""
    return [roc_from_points(*c) for c in binary_curve(scores, target=target, labels=labels, threshold=threshold)]


def precision_recall_curve(scores, target=None, labels=None, threshold=0.5):
    """-> per segment ``(precision, recall, thresholds)`` with scikit-learn's conventions (pr_from_points)."""
    return [pr_from_points(*c) for c in binary_curve(scores, target=target, labels=labels, threshold=threshold)]


def calibration(logits_or_probs, labels, bins=15, is_prob=False):
    """[N, C] logits (or probabilities, ``is_prob=True``) and integer labels [N] -> dict of device tensors: ``ece`` (expected calibration
    error over ``bins`` equal-width confidence bins (k / M, (k + 1) / M], Guo et al. 2017), ``brier`` (mean multi-class Brier score) and
    ``nll`` (mean negative log-likelihood) as 0-d float64; ``bin_count``, ``bin_correct`` (int64 [bins]) and ``bin_confidence`` (float64
    [bins], the SUM of the bin's confidences); ``scores_t`` (fp32 [C, N]: the probabilities, one row per class — what
    ``rank_metrics(scores_t, labels=labels)`` ranks).  The softmax is evaluated in double.  Nothing is read back."""
    if not (logits_or_probs.is_cuda and labels.is_cuda):
        raise ValueError("calibration is computed on the GPU: device tensors are expected (there is no CPU fallback)")
    if logits_or_probs.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits_or_probs.shape[0]:
        raise ValueError(f"calibration expects [N, C] scores and [N] labels, got {tuple(logits_or_probs.shape)} and {tuple(labels.shape)}")
    if int(bins) != bins or not 1 <= bins <= 1024:
        raise ValueError(f"calibration: bins must be an integer in 1..1024, got {bins}")
    x = logits_or_probs.float().contiguous()
    cnt, ok, conf, out, scores_t = mnn._cls_calibration(x, labels.to(torch.int32).contiguous(), int(bins), bool(is_prob))
    return {"ece": out[2], "brier": out[1], "nll": out[0], "bin_count": cnt, "bin_correct": ok, "bin_confidence": conf,
            "scores_t": scores_t}
