"""Multi-class segmentation metrics (nothing in the reference, whose metrics know one foreground): the argmax / confusion-matrix
pass of csrc/mcseg.hip on the device and the figures read from its integer counts on the host.

``confusion_batch`` launches ``mi355_mcseg_confusion`` and does not synchronise; ``metrics_from_confusion`` takes the [N][C][C]
integers after the read-back.  Rules: a pixel counts when its label is in [0, C) (``ignore_index`` and every other label >= C are
left out); the prediction is the first maximum over the classes; per image and class IoU = tp / (row + col - tp) and
Dice = 2 tp / (row + col), NaN where the denominator is 0 — no 1e-7 term: a class absent from both masks is not a perfect score, it
is no score — and the means are NaN-aware, first over the images, then over the classes."""
import numpy as np
import torch

from mi355 import nn as mnn


def confusion_batch(logits, labels, ignore_index=255, return_pred=False):
    """logits [N, C, H, W] (any float dtype, on the device), labels uint8 / integer [N, H, W] or [N, 1, H, W] ->
    int32 device tensor [N, C, C] with conf[n, label, prediction]; with ``return_pred`` also the uint8 predictions [N, H, W]
    (written for every pixel, ignored ones included).  2 <= C <= 16."""
    if logits.dim() < 3:
        raise ValueError(f"logits [N, C, H, W] expected, got {tuple(logits.shape)}")
    C = logits.shape[1]
    if not 2 <= C <= 16:
        raise ValueError(f"2 <= C <= 16 classes expected, got {C}")
    ignore_index = -1 if ignore_index is None else int(ignore_index)
    if ignore_index != -1 and not C <= ignore_index <= 255:
        raise ValueError(f"ignore_index must be None / -1 or lie in [{C}, 255] (got {ignore_index})")
    r = mnn._mc_confusion(logits, labels, ignore_index, return_pred)
    if return_pred:
        conf, pred = r
        return conf, pred.view(logits.shape[0], *logits.shape[2:])
    return r


def metrics_from_confusion(conf):
    """integer array [N, C, C] (or [C, C]: one image) -> {"iou", "dice": [N, C] per image and class (NaN: class in neither mask),
    "iou_per_class", "dice_per_class": [C] NaN-aware means over the images, "mean_iou", "mean_dice": NaN-aware means over the
    classes of those, "pixel_accuracy": trace / total over all images, "confusion_matrix": the [C, C] sum} — fractions in [0, 1]."""
    from utils.tester import _nanmean
    conf = np.asarray(conf)
    if conf.ndim == 2:
        conf = conf[None]
    if conf.ndim != 3 or conf.shape[1] != conf.shape[2]:
        raise ValueError(f"a confusion array [N, C, C] expected, got {conf.shape}")
    c = conf.astype(np.float64)
    tp = np.einsum("ncc->nc", c)
    row, col = c.sum(axis=2), c.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(row + col - tp > 0, tp / (row + col - tp), np.nan)
        dice = np.where(row + col > 0, 2.0 * tp / (row + col), np.nan)
    C = conf.shape[1]
    iou_c = np.array([_nanmean(iou[:, k])[0] for k in range(C)])
    dice_c = np.array([_nanmean(dice[:, k])[0] for k in range(C)])
    total = c.sum()
    return {"iou": iou, "dice": dice, "iou_per_class": iou_c, "dice_per_class": dice_c, "mean_iou": _nanmean(iou_c)[0],
            "mean_dice": _nanmean(dice_c)[0], "pixel_accuracy": float(tp.sum() / total) if total > 0 else float("nan"),
            "confusion_matrix": conf.astype(np.int64).sum(axis=0)}


def check_class_names(class_names, num_classes):
    """None -> ["class0", ...]; a list or a comma-separated string of ``num_classes`` distinct names otherwise."""
    if class_names is None:
        return [f"class{k}" for k in range(num_classes)]
    names = [s.strip() for s in class_names.split(",")] if isinstance(class_names, str) else [str(s) for s in class_names]
    if len(names) != num_classes or len(set(names)) != num_classes or not all(names):
        raise ValueError(f"{num_classes} distinct class names expected, got {names}")
    return names
