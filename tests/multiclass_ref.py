"""numpy fp64 restatement of the multi-class segmentation path (csrc/mcseg.hip, utils/multiclass.py): softmax cross-entropy +
per-class soft Dice with its gradient, the argmax rule, the confusion matrix and the metrics read from it.  Pinned against torch
fp64 (F.cross_entropy and autograd through a one-hot Dice) and brute-force loops in tests/test_multiclass_cpu.py.

Logits z [N, C, ...], labels y integer [N, ...]; a pixel is valid when 0 <= y < C (every other label is ignored, ignore_index among
them); weight [C] or None."""
import numpy as np


def _flat(z, y):
    z = np.asarray(z, dtype=np.float64)
    N, C = z.shape[:2]
    z = z.reshape(N, C, -1)
    y = np.asarray(y).astype(np.int64).reshape(N, -1)
    assert y.shape[1] == z.shape[2], (y.shape, z.shape)
    return z, y, N, C


def loss_terms(z, y, weight=None, smooth=1.0, per_sample=False, include_background=True):
    """-> dict with p [N, C, HW], valid [N, HW], onehot [N, C, HW], w_pix [N, HW], wsum, ce, dice, and the Dice coefficients
    a, b [G, C] (G = N with per_sample, else 1), the class set mask inS [C] and its size."""
    z, y, N, C = _flat(z, y)
    w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    lse = np.log(s[:, 0]) + m[:, 0]
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    onehot = (np.arange(C)[None, :, None] == ys[:, None, :]) & valid[:, None, :]
    zy = np.take_along_axis(z, ys[:, None, :], axis=1)[:, 0]
    w_pix = np.where(valid, w[ys], 0.0)
    wsum = float(w_pix.sum())
    ce = float((w_pix * (lse - zy)).sum() / wsum) if wsum > 0 else 0.0
    pv = p * valid[:, None, :]
    ax = (2,) if per_sample else (0, 2)
    I = (pv * onehot).sum(axis=ax).reshape(-1, C)
    P = pv.sum(axis=ax).reshape(-1, C)
    T = onehot.sum(axis=ax).astype(np.float64).reshape(-1, C)
    den = P + T + smooth
    num = 2.0 * I + smooth
    inS = np.arange(C) >= (0 if include_background else 1)
    nS = int(inS.sum())
    dice = float(np.mean(1.0 - (num / den)[:, inS].mean(axis=1)))
    return dict(p=p, valid=valid, onehot=onehot, w_pix=w_pix, wsum=wsum, ce=ce, dice=dice, a=2.0 / den, b=num / den ** 2, inS=inS,
                nS=nS, N=N, C=C)


def mc_loss(z, y, weight=None, ce_weight=1.0, dice_weight=0.0, smooth=1.0, per_sample=False, include_background=True, gscale=1.0):
    """-> ((total, ce, dice), dz of z's shape): the loss terms and gscale * d(total)/dz, +0 at ignored pixels."""
    t = loss_terms(z, y, weight, smooth, per_sample, include_background)
    p, valid, onehot = t["p"], t["valid"], t["onehot"]
    G = t["a"].shape[0]
    g = -(t["a"][:, :, None] * onehot - t["b"][:, :, None]) * t["inS"][None, :, None] / (t["nS"] * G)      # [N, C, HW]
    gp = (g * p).sum(axis=1, keepdims=True)
    d_dice = p * (g - gp)
    d_ce = t["w_pix"][:, None, :] * (p - onehot) / t["wsum"] if t["wsum"] > 0 else np.zeros_like(p)
    dz = gscale * (ce_weight * d_ce + dice_weight * d_dice)
    dz = np.where(valid[:, None, :], dz, 0.0)
    total = ce_weight * t["ce"] + dice_weight * t["dice"]
    return (total, t["ce"], t["dice"]), dz.reshape(np.asarray(z).shape)


def grad_scale(z, y, weight=None, ce_weight=1.0, dice_weight=0.0, smooth=1.0, per_sample=False, include_background=True, gscale=1.0):
    """S of the gradient bound 2^-23 |ref| + 2^-40 S: |gscale| (ce_weight max w / sum w + dice_weight (max a_c + max b_c) / |S|)."""
    t = loss_terms(z, y, weight, smooth, per_sample, include_background)
    w = np.ones(t["C"]) if weight is None else np.asarray(weight, dtype=np.float64)
    ce = ce_weight * float(w.max()) / t["wsum"] if t["wsum"] > 0 else 0.0
    return abs(gscale) * (ce + dice_weight * (float(t["a"].max()) + float(t["b"].max())) / t["nS"])


def argmax_first(z):
    """[N, C, ...] -> uint8 [N, ...]: v > best in ascending c, from best = -inf and class 0 (ties: the lower class; a NaN never wins)."""
    z = np.asarray(z)
    best = np.full(z[:, 0].shape, -np.inf, dtype=z.dtype)
    pred = np.zeros(z[:, 0].shape, dtype=np.uint8)
    for c in range(z.shape[1]):
        with np.errstate(invalid="ignore"):
            gt = z[:, c] > best
        best = np.where(gt, z[:, c], best)
        pred = np.where(gt, np.uint8(c), pred)
    return pred


def confusion(z, y):
    """-> (conf int64 [N, C, C] with conf[n, y, pred] over the valid pixels, pred uint8 of y's shape)."""
    z = np.asarray(z)
    N, C = z.shape[:2]
    pred = argmax_first(z)
    yy = np.asarray(y).astype(np.int64).reshape(N, -1)
    pp = pred.reshape(N, -1).astype(np.int64)
    conf = np.zeros((N, C, C), dtype=np.int64)
    for n in range(N):
        v = (yy[n] >= 0) & (yy[n] < C)
        conf[n] = np.bincount(yy[n][v] * C + pp[n][v], minlength=C * C).reshape(C, C)
    return conf, pred.reshape(np.asarray(y).shape)


def _nanmean(a, axis=None):
    a = np.asarray(a, dtype=np.float64)
    ok = ~np.isnan(a)
    n = ok.sum(axis=axis)
    s = np.where(ok, a, 0.0).sum(axis=axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / np.maximum(n, 1), np.nan) if np.ndim(n) else (s / n if n > 0 else float("nan"))


def metrics(conf):
    """[N, C, C] -> dict: per image and class IoU = tp / (row + col - tp) and Dice = 2 tp / (row + col), NaN where the denominator
    is 0; class means = NaN-aware mean over images; mean_* = NaN-aware mean over classes of those; pixel accuracy = trace / total."""
    conf = np.asarray(conf, dtype=np.float64)
    tp = np.einsum("ncc->nc", conf)
    row, col = conf.sum(axis=2), conf.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(row + col - tp > 0, tp / (row + col - tp), np.nan)
        dice = np.where(row + col > 0, 2 * tp / (row + col), np.nan)
    iou_c, dice_c = _nanmean(iou, axis=0), _nanmean(dice, axis=0)
    total = conf.sum()
    return dict(iou=iou, dice=dice, iou_per_class=iou_c, dice_per_class=dice_c, mean_iou=float(_nanmean(iou_c)),
                mean_dice=float(_nanmean(dice_c)), pixel_acc=float(tp.sum() / total) if total > 0 else float("nan"))


def val_metric(conf):
    """mean over the classes with a non-zero union of tp / (row + col - tp), from the batch-summed confusion matrix (0 if none)."""
    c = np.asarray(conf, dtype=np.float64).sum(axis=0)
    tp = np.diag(c)
    un = c.sum(axis=1) + c.sum(axis=0) - tp
    ok = un > 0
    return float((tp[ok] / un[ok]).mean()) if ok.any() else 0.0
