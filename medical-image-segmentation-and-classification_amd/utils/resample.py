"""Resampling statistics on the device (csrc/resample.hip): bootstrap confidence intervals for what utils/tester.py reports, DeLong's
variance of an AUROC and test between two, and McNemar's test — what ``tester.py --ci R`` prints, exposed for other uses.

A bootstrap replicate is a row of integer weights (how often each sample was drawn), never a copy of the data; ``bootstrap_counts``
draws R of them with a counter-based generator (Philox4x32-10), so a seed names the same resamples on every run, for every model and
for every metric: differences between two models evaluated with the same weights are paired.  Row 0 of the weights is all ones, so row
0 of everything computed from them is the point estimate.  The integers (weighted positives / negatives, twice the Mann-Whitney
statistic, confusion matrices, DeLong's components) are exact; the doubles are folded in a fixed order: the same bits on every run.

Everything stays on the device except ``delong_test`` and ``mcnemar``, which read back a handful of numbers to form a p-value."""
import math
from fractions import Fraction

import torch

from mi355 import nn as mnn
from utils.ranking import _prepare

MAX_REPLICATES = 8192


def _device_only(what, *tensors):
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise ValueError(f"{what} is computed on the GPU: device tensors are expected (there is no CPU fallback)")


def _check_counts(what, counts, n):
    _device_only(what, counts)
    if counts.dim() != 2 or counts.shape[0] < 2 or counts.shape[1] != n or counts.dtype != torch.int32:
        raise ValueError(f"{what}: counts must be int32 [replicates + 1, {n}] (bootstrap_counts), got {counts.dtype} {tuple(counts.shape)}")
    return counts.contiguous()


def bootstrap_counts(n, replicates, seed=0, device="cuda"):
    """-> int32 [replicates + 1, n] on ``device``: row 0 all ones, row r the multinomial counts of n draws with replacement."""
    if int(n) != n or n < 1 or int(replicates) != replicates or replicates < 1:
        raise ValueError(f"bootstrap_counts: n >= 1 and replicates >= 1 are expected, got n={n}, replicates={replicates}")
    if torch.device(device).type != "cuda":
        raise ValueError("bootstrap_counts is computed on the GPU: a cuda device is expected (there is no CPU fallback)")
    return mnn._boot_counts(int(n), int(replicates), int(seed), device)


def boot_rank_metrics(scores, counts, target=None, labels=None, threshold=0.5):
    """``utils.ranking.rank_metrics`` on every resample -> dict of device tensors [R1, S]: ``pos``, ``neg``, ``u2`` (int64, weighted),
    ``auroc`` = u2 / (2 pos neg) and ``average_precision`` (float64), NaN where a replicate leaves them undefined."""
    z, t, y = _prepare(scores, target, labels, "boot_rank_metrics")
    pnu, ap = mnn._boot_rank(z, t, y, threshold, _check_counts("boot_rank_metrics", counts, z.shape[1]))
    pos, neg, u2 = pnu[..., 0], pnu[..., 1], pnu[..., 2]
    return {"pos": pos, "neg": neg, "u2": u2, "auroc": u2.double() / (2.0 * pos.double() * neg.double()), "average_precision": ap}


def boot_confusion(pred, labels, classes, counts):
    """integer predictions and labels [n] in 0 .. classes - 1 -> int64 [R1, classes, classes] weighted confusion matrices (rows the
    truth, columns the prediction) and int64 [R1], the weight of samples skipped for an id outside that range."""
    _device_only("boot_confusion", pred, labels)
    if pred.dim() != 1 or pred.shape != labels.shape or pred.numel() == 0:
        raise ValueError(f"boot_confusion expects pred and labels [n], got {tuple(pred.shape)} and {tuple(labels.shape)}")
    if int(classes) != classes or not 1 <= classes <= 64:
        raise ValueError(f"boot_confusion: classes must be an integer in 1..64, got {classes}")
    c = _check_counts("boot_confusion", counts, pred.shape[0])
    return mnn._boot_confusion(pred.to(torch.int32).contiguous(), labels.to(torch.int32).contiguous(), int(classes), c)


def classification_from_confusion(cm):
    """int64 [..., C, C] confusion matrices -> dict of float64 device tensors [...]: ``accuracy`` and the support-weighted ``precision``,
    ``recall``, ``f1`` in percent, as ``utils.tester.calculate_classification_metrics`` forms them from the arrays: a class without
    support has weight 0, a zero denominator gives 0."""
    _device_only("classification_from_confusion", cm)
    tp = torch.diagonal(cm, dim1=-2, dim2=-1).double()
    pred_pos, support = cm.sum(-2).double(), cm.sum(-1).double()      # integer sums: exact
    total = cm.sum((-2, -1)).double().unsqueeze(-1)
    zero = torch.zeros_like(tp)
    prec = torch.where(pred_pos > 0, tp / pred_pos, zero)
    rec = torch.where(support > 0, tp / support, zero)
    f1 = torch.where(prec + rec > 0, 2 * prec * rec / (prec + rec), zero)
    w = support / total

    def fold(x):                                  # over the classes in class order, as numpy adds a handful of terms
        acc = x[..., 0]
        for c in range(1, x.shape[-1]):
            acc = acc + x[..., c]
        return acc

    accuracy = torch.diagonal(cm, dim1=-2, dim2=-1).sum(-1).double() / total[..., 0] * 100
    return {"accuracy": accuracy, "precision": fold(prec * w) * 100, "recall": fold(rec * w) * 100, "f1": fold(f1 * w) * 100}


def _boot_sums(values, counts):
    """per-sample values [M, n] (or [n]) -> (float64 [R1, M] weighted sums, int64 [R1, M] weights) over the values that are not NaN"""
    _device_only("boot_means", values)
    v = values.double().contiguous()
    v = v.view(1, -1) if v.dim() == 1 else v
    if v.dim() != 2 or v.numel() == 0:
        raise ValueError(f"boot_means expects values [M, n] or [n], got {tuple(values.shape)}")
    return mnn._boot_sums(v, _check_counts("boot_means", counts, v.shape[1]))


def boot_means(values, counts):
    """per-sample values [M, n] (or [n]) -> float64 [R1, M]: the NaN-aware mean of every row under every resample (NaN where a
    replicate drew no defined value)."""
    total, weight = _boot_sums(values, counts)
    return total / weight.double()


def interval(reps, level=0.95):
    """replicates float64 [R1, K] (or [R1]) with the point estimate in row 0 -> dict of float64 device tensors [K]: ``point``, ``mean``
    and ``se`` (ddof = 1) of the defined replicates, ``lo`` / ``hi`` (the percentile interval at ``level``: numpy's linear quantiles at
    (1 - level) / 2 and 1 - that) and ``valid``, how many replicates were not NaN."""
    _device_only("interval", reps)
    if not 0.0 < level < 1.0:
        raise ValueError(f"interval: 0 < level < 1 expected, got {level}")
    r = reps.double().contiguous()
    r = r.view(-1, 1) if r.dim() == 1 else r
    if r.dim() != 2 or r.shape[0] < 2 or r.shape[1] < 1 or r.shape[0] - 1 > MAX_REPLICATES:
        raise ValueError(f"interval expects replicates [R + 1, K] with 1 <= R <= {MAX_REPLICATES}, got {tuple(reps.shape)}")
    alpha = (1.0 - level) / 2.0
    out = mnn._boot_interval(r, alpha, 1.0 - alpha)
    return {k: out[:, i] for i, k in enumerate(("point", "mean", "se", "lo", "hi", "valid"))}


def _delong_prepare(scores, labels):
    _device_only("delong", scores, labels)
    z = scores.float().contiguous()
    z = z.unsqueeze(0) if z.dim() == 2 else z
    if z.dim() != 3 or z.numel() == 0 or labels.dim() != 1 or labels.shape[0] != z.shape[2]:
        raise ValueError(f"delong expects scores [M, C, n] (or [C, n]) and labels [n], got {tuple(scores.shape)} and {tuple(labels.shape)}")
    return z, labels.to(torch.int32).contiguous()


def delong(scores, labels):
    """scores [M, C, n] (model, class, sample; or [C, n] for one model) and integer labels [n], class c one-vs-rest -> dict of device
    tensors: ``auroc`` float64 [M, C], ``var`` float64 [M, C] (DeLong's variance of it), ``cov`` float64 [C, M, M], ``pos``, ``neg``,
    ``u2`` int64 [M, C] and ``v2`` int64 [M, C, n] (twice the structural components times the other class's size).  NaN where a class
    has fewer than two members or non-members."""
    z, y = _delong_prepare(scores, labels)
    v2, pnu, var, cov = mnn._delong(z, y)
    pos, neg, u2 = pnu[..., 0], pnu[..., 1], pnu[..., 2]
    return {"auroc": u2.double() / (2.0 * pos.double() * neg.double()), "var": var, "cov": cov, "pos": pos, "neg": neg, "u2": u2,
            "v2": v2}


def delong_test(scores_a, scores_b, labels):
    """two models' scores [C, n] on the same samples -> a list with, per class, a dict of floats ``auc_a``, ``auc_b``, ``z`` and the
    two-sided ``p`` = erfc(|z| / sqrt 2) of DeLong's test for equal AUROCs; z and p are NaN where the variance of the difference is
    zero (identical rankings) or undefined."""
    _device_only("delong_test", scores_a, scores_b, labels)
    if scores_a.shape != scores_b.shape or scores_a.dim() != 2:
        raise ValueError(f"delong_test expects two score tensors [C, n], got {tuple(scores_a.shape)} and {tuple(scores_b.shape)}")
    d = delong(torch.stack([scores_a.float(), scores_b.float()]), labels)
    auc, cov = d["auroc"].cpu().tolist(), d["cov"].cpu().tolist()
    out = []
    for c in range(scores_a.shape[0]):
        v = cov[c][0][0] + cov[c][1][1] - 2.0 * cov[c][0][1]
        z = (auc[0][c] - auc[1][c]) / math.sqrt(v) if v > 0.0 else float("nan")
        out.append({"auc_a": auc[0][c], "auc_b": auc[1][c], "z": z, "p": math.erfc(abs(z) / math.sqrt(2.0)) if z == z else float("nan")})
    return out


def _mcnemar_p(b, c):
    """the exact two-sided binomial p of b and c discordant pairs, min(1, 2 P(X <= min(b, c))) with X ~ Bin(b + c, 1 / 2), in integers"""
    n, k = b + c, min(b, c)
    if n == 0:
        return 1.0
    tail = sum(math.comb(n, i) for i in range(k + 1))
    return min(1.0, float(Fraction(2 * tail, 1 << n)))


def mcnemar(correct_a, correct_b):
    """two models' per-sample correctness (bool or 0 / 1, [n]) -> dict: ``table`` (2 x 2 ints, rows a wrong / right, columns b wrong /
    right), ``b`` (a right, b wrong), ``c`` (a wrong, b right) and the exact two-sided ``p``."""
    _device_only("mcnemar", correct_a, correct_b)
    n = correct_a.shape[0]
    ones = torch.ones(2, n, dtype=torch.int32, device=correct_a.device)      # row 0 of a weight table: the plain counts
    cm, _ = boot_confusion(correct_b.to(torch.int32), correct_a.to(torch.int32), 2, ones)
    t = cm[0].cpu().tolist()
    b, c = int(t[1][0]), int(t[0][1])
    return {"table": t, "b": b, "c": c, "p": _mcnemar_p(b, c)}
