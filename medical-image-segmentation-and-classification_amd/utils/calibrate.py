"""Post-hoc calibration (csrc/calibrate.hip; nothing in the reference): fitted on the validation set after training, applied at test
time.  A classifier gets ONE temperature T (Guo et al. 2017): its logits are divided by T before the softmax, which leaves the argmax —
accuracy, the confusion matrix — alone and moves the confidence, ECE, Brier score and NLL.  A segmenter gets the mask threshold t* with
the best mean per-image Dice over a list of candidates, in place of the constant 0.5.

``fit_temperature`` / ``apply_temperature`` and ``dice_sweep`` / ``pick_threshold`` stay on the device: no host round trip, no
synchronisation, the same bits on every run.  ``calibrate_model`` runs a model over a loader and reads back once, into a
``Calibration`` that is saved next to the checkpoint as ``{name}_calibration.json`` (trainer.py --calibrate) and loaded by
tester.py --calibration and ``JointPipeline(calibration=...)``."""
import json
import os
from dataclasses import asdict, dataclass

import numpy as np
import torch

from mi355 import nn as mnn

STATUS = ("converged", "lower clamp", "upper clamp", "flat", "iteration cap")
STATE_KEYS = ("beta", "temperature", "nll_before", "nll_after", "gradient", "curvature", "evaluations", "status")


def default_thresholds():
    """k / 256, k = 1 .. 255 in fp32: 0.5 is candidate 127, exactly"""
    return np.arange(1, 256, dtype=np.float32) / np.float32(256)


def _need_device(what, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise ValueError(f"{what} is computed on the GPU: device tensors are expected (there is no CPU fallback)")


def fit_temperature(logits, labels):
    """[N, C] logits and integer labels [N] (device tensors) -> dict of 0-d float64 device tensors: ``beta`` = 1 / T, ``temperature``,
    ``nll_before`` (mean NLL at T = 1), ``nll_after``, ``gradient`` and ``curvature`` (g', g'' of the mean NLL in beta, at beta),
    ``evaluations`` and ``status`` (0 converged, 1 / 2 stopped at beta = 2^-6 / 2^6, 3 flat, 4 iteration cap; STATUS names them), and
    ``state``, the float64 [8] they are views of.  A safeguarded Newton iteration on the device; nothing is read back."""
    _need_device("fit_temperature", logits, labels)
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError(f"fit_temperature expects [N, C] logits and [N] labels, got {tuple(logits.shape)} and {tuple(labels.shape)}")
    state = mnn._temperature_fit(logits.float().contiguous(), labels.to(torch.int32).contiguous())
    fit = {k: state[i] for i, k in enumerate(STATE_KEYS)}
    fit["state"] = state
    return fit


def apply_temperature(logits, fit_or_T):
    """logits * beta in double, rounded to fp32 once.  ``fit_or_T``: fit_temperature's dict (beta is read on the device), a
    ``Calibration`` or a temperature T."""
    _need_device("apply_temperature", logits)
    if logits.dim() != 2:
        raise ValueError(f"apply_temperature expects [N, C] logits, got {tuple(logits.shape)}")
    return mnn._logits_scale(logits.float().contiguous(), _beta_of(fit_or_T, logits.device))


def _beta_of(fit_or_T, device):
    """-> a float64 device tensor whose first element is beta = 1 / T"""
    if isinstance(fit_or_T, dict):
        return fit_or_T["state"]
    T = float(fit_or_T.temperature if isinstance(fit_or_T, Calibration) else fit_or_T)
    if not T > 0:
        raise ValueError(f"temperature: T > 0 required, got {T}")
    return torch.tensor([1.0 / T], dtype=torch.float64, device=device)


def nll_at(logits, labels, fit_or_T):
    """The mean NLL of softmax(logits / T) in double, on the logits as they are (apply_temperature rounds the scaled logits to fp32):
    the figure fit_temperature minimised -> 0-d float64 device tensor.  ``fit_or_T`` as for apply_temperature."""
    _need_device("nll_at", logits, labels)
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError(f"nll_at expects [N, C] logits and [N] labels, got {tuple(logits.shape)} and {tuple(labels.shape)}")
    return mnn._temperature_eval(logits.float().contiguous(), labels.to(torch.int32).contiguous(), _beta_of(fit_or_T, logits.device))[0]


def _check_thresholds(thresholds):
    thr = default_thresholds() if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= thr.size <= 1024 or np.isnan(thr).any() or (np.diff(thr) <= 0).any():
        raise ValueError("thresholds: 1 .. 1024 strictly ascending values expected")
    return thr


def dice_sweep(scores, target, thresholds=None, is_logit=False, acc=None, target_threshold=0.5):
    """scores [B, ...] (probabilities, or logits with ``is_logit``) and target of the same size, flattened per image, swept over the
    ascending candidates ``thresholds`` (default k / 256) -> ``acc``: dict of device tensors ``tp``, ``fp`` int32 [B, K] (this
    batch's positive / negative pixels with score > candidate), ``pos`` int32 [B], ``sums`` float64 [2, K] (the per-image Dice and
    IoU added up over every batch folded so far), ``n_images`` int64 [1] and ``thresholds`` fp32 [K].  Pass the returned ``acc`` to
    the next batch's call: a validation set accumulates in loader order.  Nothing is read back."""
    _need_device("dice_sweep", scores, target)
    if scores.dim() < 1 or scores.numel() == 0 or target.numel() != scores.numel():
        raise ValueError(f"dice_sweep expects scores [B, ...] and a target of the same size, got {tuple(scores.shape)} and {tuple(target.shape)}")
    z = scores.float().contiguous()
    z = z.view(1, -1) if z.dim() == 1 else z.view(z.shape[0], -1)
    t = target.float().contiguous().view(z.shape)
    if acc is None:
        cand = _check_thresholds(thresholds)
        acc = {"thresholds": torch.from_numpy(cand).to(z.device), "candidates": cand,      # (candidates: the host's copy)
               "sums": torch.zeros(2, cand.size, dtype=torch.float64, device=z.device),
               "n_images": torch.zeros(1, dtype=torch.int64, device=z.device)}
    elif thresholds is not None:
        raise ValueError("dice_sweep: the candidates are those of acc: pass thresholds with the first batch only")
    tp, fp, pos = mnn._thr_sweep(z, t, acc["thresholds"], is_logit, target_threshold)
    mnn._thr_sweep_fold(tp, fp, pos, acc["sums"], acc["n_images"])
    acc.update(tp=tp, fp=fp, pos=pos)
    return acc


def pick_threshold(acc, reference=0.5):
    """dice_sweep's ``acc`` -> dict of device tensors: ``index`` int32 [1] (the lowest candidate with the largest mean Dice),
    ``threshold`` fp32 [1], ``dice``, ``iou`` (0-d float64: the means at it), ``dice_ref``, ``iou_ref`` (at the candidate equal to
    ``reference``, NaN when there is none).  Nothing is read back."""
    thr = acc["thresholds"]
    hit = np.flatnonzero(acc["candidates"] == np.float32(reference)) if reference is not None else ()
    k_ref = int(hit[0]) if len(hit) else -1       # (the host's copy of the candidates: no read-back)
    out_d, out_k = mnn._thr_sweep_pick(acc["sums"], acc["n_images"], k_ref)
    return {"index": out_k, "threshold": thr[out_k.long()], "dice": out_d[0], "iou": out_d[1], "dice_ref": out_d[2], "iou_ref": out_d[3]}


@dataclass
class Calibration:
    """What ``calibrate_model`` found.  ``kind``: "classification" (``temperature``; ``before`` / ``after`` = the mean NLL at T = 1 /
    at T) or "segmentation" (``threshold``; the mean Dice at 0.5 / at the threshold, fractions).  ``status``: fit_temperature's (0 for
    a segmenter); ``samples``: the validation samples seen."""
    kind: str
    temperature: float = 1.0
    threshold: float = 0.5
    before: float = float("nan")
    after: float = float("nan")
    status: int = 0
    samples: int = 0

    @staticmethod
    def path(directory, name):
        return os.path.join(directory, f"{name}_calibration.json")

    def save(self, path):
        with open(path, "w") as f:
            json.dump(asdict(self), f, indent=1)
        return path

    @classmethod
    def load(cls, path):
        if not os.path.exists(path):
            raise FileNotFoundError(f"calibration sidecar not found: {path} (written by trainer.py --calibrate)")
        with open(path) as f:
            return cls(**json.load(f))

    def describe(self):
        if self.kind == "classification":
            return f"temperature T = {self.temperature:.4f} ({STATUS[self.status]}), NLL {self.before:.4f} -> {self.after:.4f} on {self.samples} validation samples"
        return f"threshold t* = {self.threshold:.4f}, mean Dice {self.before * 100:.2f}% at 0.5 -> {self.after * 100:.2f}% on {self.samples} validation samples"


def find_sidecar(directory, name, sub):
    """the ``Calibration`` of model ``name`` from ``directory`` or ``directory/sub``; FileNotFoundError naming the file otherwise"""
    first = Calibration.path(directory, name)
    nested = Calibration.path(os.path.join(directory, sub), name)
    return Calibration.load(nested if not os.path.exists(first) and os.path.exists(nested) else first)


@torch.no_grad()
def calibrate_model(model, val_dl, device, seg, thresholds=None):
    """Run ``model`` in eval mode over ``val_dl`` and fit its calibration on the device: a classifier's logits are kept and its
    temperature fitted once; a segmenter's batches are folded into the threshold sweep one by one.  One read-back at the end ->
    ``Calibration``.  Under data parallelism rank 0 fits and the other ranks return None."""
    from utils.distributed import dist_info
    if dist_info()[0] != 0:
        return None
    was_training = model.training
    model.eval()
    kept, labels, acc = [], [], None
    for images, y in val_dl:
        out = model(images.to(device))
        if seg:
            acc = dice_sweep(out, y.to(device), thresholds if acc is None else None, is_logit=True, acc=acc)
        else:
            kept.append(out.float())
            labels.append(y.to(device))
    model.train(was_training)
    if seg:
        if acc is None:
            raise ValueError("calibrate_model: the validation loader is empty")
        p = pick_threshold(acc)
        got = torch.stack([p["threshold"][0].double(), p["dice_ref"], p["dice"], acc["n_images"][0].double()]).cpu().numpy()
        return Calibration("segmentation", threshold=float(got[0]), before=float(got[1]), after=float(got[2]), samples=int(got[3]))
    if not kept:
        raise ValueError("calibrate_model: the validation loader is empty")
    state = fit_temperature(torch.cat(kept), torch.cat(labels))["state"].cpu().numpy()
    return Calibration("classification", temperature=float(state[1]), before=float(state[2]), after=float(state[3]),
                       status=int(state[7]), samples=sum(k.shape[0] for k in kept))
