"""Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) on the device (nothing in the reference, which trains on hard labels):
regularisers for classifiers trained on a few thousand images per class, applied to the normalised batch where it lies after the GPU
input pipeline (csrc/mix.hip, one streaming pass; the rule is written out in include/mi355conv.h).

Mixup blends every sample with a partner, ``lam * x + (1 - lam) * x[perm]`` with ``lam ~ Beta(alpha, alpha)``; CutMix pastes a box of the
partner into the sample and leaves the rest alone.  Either way the label becomes a distribution over the two classes — ``MixedTarget`` —
which ``mi355.nn.MixCrossEntropyLoss`` takes (mi355_ce_mix).  For segmentation (``seg=True``) only CutMix is offered: image AND mask get
the partner's box, so the masks stay in {0, 1}; a blended mask would break the thresholded losses.

The draws are made on the host from a generator of the ``BatchMix`` object's own (``numpy.random.default_rng(seed)``): nothing shared
with the transforms', the loader's or torch's generators is touched.  One small upload per batch, no read-back, no synchronisation.

``train()`` (utils/helpers.py) keeps the reference's parameter list, so the mixer reaches it on the training loader:
``train(model, MixedBatches(train_dl, batch_mix), val_dl, ...)``."""
from __future__ import annotations

import math

import numpy as np
import torch

from mi355.lib import lib


def cutmix_box(h, w, lam0, cy, cx):
    """The paper's box for a drawn ``lam0`` and centre: sides int(h r), int(w r) with r = sqrt(1 - lam0), clipped to the image ->
    (y0, x0, y1, x1), half-open."""
    r = math.sqrt(max(1.0 - float(lam0), 0.0))
    ch, cw = int(h * r), int(w * r)
    clip = lambda v, hi: min(max(v, 0), hi)
    return clip(cy - ch // 2, h), clip(cx - cw // 2, w), clip(cy + ch // 2, h), clip(cx + cw // 2, w)


def kernel_lam(lam, boxes):
    """The blend weight the kernel gets for a draw: the target weight for mixup (an empty box), 1 for CutMix (the box alone mixes)."""
    lam, boxes = np.asarray(lam, np.float32).reshape(-1), np.asarray(boxes, np.int64).reshape(-1, 4)
    empty = (boxes[:, 0] >= boxes[:, 2]) | (boxes[:, 1] >= boxes[:, 3])
    return np.where(empty, lam, np.float32(1.0)).astype(np.float32)


def mix_batch(x, perm, lam, boxes):
    """mi355_mix_batch_f32 on a float32 [N,C,H,W] GPU tensor -> a new tensor of x's shape: x[perm[n]] inside sample n's box
    (y0, x0, y1, x1), lam[n] * x[n] + (1 - lam[n]) * x[perm[n]] outside it.  perm, lam, boxes: host sequences or arrays of N, N and
    N x 4 entries, validated here (perm in [0, N), 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W), then uploaded in one copy."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"mix: a float32 [N,C,H,W] GPU tensor expected, got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', 'the host')}")
    if not x.is_contiguous():
        raise ValueError("mix: x must be contiguous")
    N, C, H, W = x.shape
    if N < 1 or C * H * W < 1:
        raise ValueError(f"mix: empty batch {tuple(x.shape)}")
    perm, lam, boxes = np.asarray(perm), np.asarray(lam, np.float32), np.asarray(boxes)
    if perm.shape != (N,) or lam.shape != (N,) or boxes.shape != (N, 4):
        raise ValueError(f"mix: perm, lam, boxes must hold {N}, {N} and {N} x 4 entries, got {perm.shape}, {lam.shape}, {boxes.shape}")
    if perm.dtype.kind not in "iu" or boxes.dtype.kind not in "iu":
        raise ValueError(f"mix: perm and boxes must be integers, got {perm.dtype}, {boxes.dtype}")
    if perm.min() < 0 or perm.max() >= N:
        raise ValueError(f"mix: perm entries must lie in [0, {N}), got {perm.tolist()}")
    y0, x0, y1, x1 = (boxes[:, k] for k in range(4))
    if not (np.all(0 <= y0) and np.all(y0 <= y1) and np.all(y1 <= H) and np.all(0 <= x0) and np.all(x0 <= x1) and np.all(x1 <= W)):
        raise ValueError(f"mix: boxes must satisfy 0 <= y0 <= y1 <= {H} and 0 <= x0 <= x1 <= {W}, got {boxes.tolist()}")
    if not np.all(np.isfinite(lam)):
        raise ValueError(f"mix: lam must be finite, got {lam.tolist()}")
    packed = np.concatenate([perm.astype(np.int32), lam.view(np.int32), boxes.astype(np.int32).reshape(-1)])
    d = torch.from_numpy(packed).to(x.device, non_blocking=True)          # [perm | lam bits | boxes]: one upload
    out = torch.empty_like(x)
    lib.mi355_mix_batch_f32(x, d[:N], d[N:2 * N], d[2 * N:], out, N, C, H, W)
    return out


class MixedTarget:
    """The label of a mixed batch: class ``ya`` with weight ``lam`` and class ``yb`` with weight ``1 - lam`` per sample.  Device tensors:
    int64 [N], int64 [N], float32 [N].  ``hard`` is the class with the larger weight (``ya`` on a tie), what training accuracy counts."""

    def __init__(self, ya, yb, lam):
        if not (ya.dim() == yb.dim() == lam.dim() == 1 and ya.shape == yb.shape == lam.shape):
            raise ValueError(f"MixedTarget: three [N] tensors expected, got {tuple(ya.shape)}, {tuple(yb.shape)}, {tuple(lam.shape)}")
        self.ya, self.yb, self.lam = ya.to(torch.int64), yb.to(torch.int64), lam.to(torch.float32)

    @property
    def hard(self):
        return torch.where(self.lam >= 0.5, self.ya, self.yb)

    def to(self, *args, **kwargs):
        return MixedTarget(self.ya.to(*args, **kwargs), self.yb.to(*args, **kwargs), self.lam.to(*args, **kwargs))

    def size(self, dim=None):
        return self.ya.size() if dim is None else self.ya.size(dim)

    def __len__(self):
        return self.ya.size(0)

    def __repr__(self):
        return f"MixedTarget(ya={self.ya.tolist()}, yb={self.yb.tolist()}, lam={self.lam.tolist()})"


class BatchMix:
    """``x, y = BatchMix(...)(x, y)`` on a normalised float32 [N,C,H,W] GPU batch.

    ``mixup_alpha`` / ``cutmix_alpha``: the Beta parameters, 0 = that scheme off (both 0: the object does nothing).  ``p``: probability
    that a batch is mixed at all (``per_sample=True``: each sample, with a scheme and a ``lam`` of its own); ``switch_p``: probability of
    CutMix when both schemes are on.  ``seg=True``: y is the mask batch and gets the same boxes; only CutMix is allowed.

    ``draw(n, h, w)`` -> (perm, lam, boxes), host arrays (int64 [n], float32 [n], int64 [n, 4] as (y0, x0, y1, x1)):
      an unmixed sample has perm = itself, lam = 1 and an empty box (all zeros); otherwise perm is a uniform random permutation and
      mixup: lam ~ Beta(alpha, alpha), an empty box;
      CutMix: ``cutmix_box`` of lam0 ~ Beta(alpha, alpha) and a uniform centre, and lam = 1 - box area / (h w), the share of the sample
      that is left — the weight of its label; the kernel blends with ``kernel_lam`` = 1.
    Classification returns ``(x_mixed, MixedTarget(y, y[perm], lam))``, segmentation ``(x_mixed, y_mixed)``.  ``params`` fixes the draw.
    With N == 1 or both alphas 0 the inputs come back as they are and nothing is launched or drawn."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, p=1.0, switch_p=0.5, per_sample=False, seed=0, seg=False):
        for nm, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if isinstance(v, bool) or not v >= 0 or v == float("inf"):
                raise ValueError(f"mix: {nm} must be a finite number >= 0 ({v})")
        for nm, v in (("p", p), ("switch_p", switch_p)):
            if isinstance(v, bool) or not 0 <= v <= 1:
                raise ValueError(f"mix: {nm} must lie in [0, 1] ({v})")
        if seg and mixup_alpha > 0:
            raise ValueError("mix: mixup is not offered for segmentation (a blended mask breaks the thresholded losses); use cutmix_alpha")
        self.mixup_alpha, self.cutmix_alpha, self.p, self.switch_p = float(mixup_alpha), float(cutmix_alpha), float(p), float(switch_p)
        self.per_sample, self.seed, self.seg = bool(per_sample), int(seed), bool(seg)
        self.rng = np.random.default_rng(self.seed)

    @property
    def active(self):
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0

    def _one(self, h, w):
        """one scheme and its parameters -> (target lam, box)"""
        rng = self.rng
        cut = self.cutmix_alpha > 0 and (self.mixup_alpha == 0 or rng.random() < self.switch_p)
        if not cut:
            return float(rng.beta(self.mixup_alpha, self.mixup_alpha)), (0, 0, 0, 0)
        lam0 = float(rng.beta(self.cutmix_alpha, self.cutmix_alpha))
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        y0, x0, y1, x1 = cutmix_box(h, w, lam0, cy, cx)
        if y0 == y1 or x0 == x1:
            return 1.0, (0, 0, 0, 0)
        return 1.0 - (y1 - y0) * (x1 - x0) / (h * w), (y0, x0, y1, x1)

    def draw(self, n, h, w):
        perm, lam, boxes = np.arange(n, dtype=np.int64), np.ones(n, np.float32), np.zeros((n, 4), np.int64)
        if not self.active or n < 2:
            return perm, lam, boxes
        rng = self.rng
        apply = rng.random(n) < self.p if self.per_sample else np.full(n, rng.random() < self.p)
        if not apply.any():
            return perm, lam, boxes
        drawn = rng.permutation(n)
        shared = None if self.per_sample else self._one(h, w)
        for i in np.flatnonzero(apply):
            l, b = self._one(h, w) if shared is None else shared
            perm[i], lam[i], boxes[i] = drawn[i], l, b
        return perm, lam, boxes

    def __call__(self, x, y, params=None):
        if not self.active or x.size(0) < 2:
            return x, y
        N, _, H, W = x.shape
        perm, lam, boxes = self.draw(N, H, W) if params is None else params
        x = x if x.is_contiguous() else x.contiguous()
        xm = mix_batch(x, perm, kernel_lam(lam, boxes), boxes)
        if self.seg:
            if y.dtype != torch.float32 or y.dim() not in (3, 4) or y.size(0) != N or tuple(y.shape[-2:]) != (H, W):
                raise ValueError(f"mix: a float32 mask batch [N,1,H,W] or [N,H,W] matching x expected, got {y.dtype} {tuple(y.shape)}")
            y4 = y.contiguous().view(N, -1, H, W)
            return xm, mix_batch(y4, perm, np.ones(N, np.float32), boxes).view(y.shape)
        if y.dim() != 1 or y.size(0) != N or y.dtype.is_floating_point:
            raise ValueError(f"mix: an integer label tensor [N] expected, got {y.dtype} {tuple(y.shape)}")
        ya = y.to(torch.int64)
        yb = ya[torch.from_numpy(np.asarray(perm, np.int64)).to(y.device, non_blocking=True)]
        return xm, MixedTarget(ya, yb, torch.from_numpy(np.asarray(lam, np.float32)).to(y.device, non_blocking=True))

    def __repr__(self):
        return (f"BatchMix(mixup_alpha={self.mixup_alpha}, cutmix_alpha={self.cutmix_alpha}, p={self.p}, switch_p={self.switch_p}, "
                f"per_sample={self.per_sample}, seed={self.seed}, seg={self.seg})")


class MixedBatches:
    """A training loader with the ``BatchMix`` that goes with it: ``train(model, MixedBatches(train_dl, batch_mix), val_dl, ...)``.
    ``train()`` takes the pair apart — it shards and iterates ``loader`` as it would without the wrapper and calls
    ``x, y = batch_mix(x, y)`` on every training batch behind its ``.to(device)``; the validation loader is never wrapped.
    ``batch_mix=None`` is the plain loader.  In a hand-written loop, iterating the wrapper yields the mixed batches; the loader
    must then deliver GPU batches (``GpuBatchLoader``), or ``device`` says where to move them first."""

    def __init__(self, loader, batch_mix=None, device=None):
        if batch_mix is not None and not callable(batch_mix):
            raise TypeError(f"MixedBatches: batch_mix must be a BatchMix or None, got {type(batch_mix).__name__}")
        self.loader, self.batch_mix, self.device = loader, batch_mix, device
        self.dataset = getattr(loader, "dataset", None)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for x, y in self.loader:
            if self.device is not None:
                x, y = x.to(self.device, non_blocking=True), y.to(self.device, non_blocking=True)
            yield (x, y) if self.batch_mix is None else self.batch_mix(x, y)
