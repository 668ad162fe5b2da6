"""fp64 numpy statement of the Dice / BCE + Dice segmentation loss and of its gradient (csrc/seg_loss.hip, mi355.nn.DiceLoss /
CombinedLoss), used by tests/test_seg_loss_cpu.py and tests/test_gpu_seg_loss.py.

With p = sigmoid(z), n = z.size, I = sum p t, P = sum p, T = sum t, D = P + T + smooth, the sums over the whole batch:

    dice_loss  = 1 - (2 I + smooth) / D
    loss       = bce_weight * mean(BCEWithLogits(z, t)) + dice_weight * dice_loss
    dloss/dz_i = bce_weight (p_i - t_i) / n  -  dice_weight (2 t_i D - (2 I + smooth)) / D^2 * p_i (1 - p_i)

``per_sample=True``: I, P, T, D and the Dice term per image (first axis), the B Dice terms averaged; the BCE term is unchanged.

PINNED: tests/test_seg_loss_cpu.py holds these formulas to tests/golden/seg_losses.npz, which records what the reference's own
``DiceLoss`` / ``CombinedLoss`` (utils/clip_seg_finetuner.py:40-74) and autograd give in fp64 (scripts/make_seg_loss_golden.py).
Nothing here shares code with the library or with torch: plain numpy, the gradient in closed form."""
import numpy as np


def sigmoid(z):
    """Stable for both signs: e = exp(-|z|) never overflows."""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_with_logits_terms(z, t):
    """Per-element nn.BCEWithLogitsLoss terms, stable form."""
    return np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))


def seg_loss(z, t, bce_weight=0.5, dice_weight=0.5, smooth=1.0, per_sample=False):
    """-> (loss: float, dloss/dz: float64 array of z's shape)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(z.shape)
    B, n = z.shape[0], z.size
    p = sigmoid(z)
    loss = bce_weight * bce_with_logits_terms(z, t).sum() / n
    # p - t without the cancellation at saturated logits: where p is next to 1, p - t = (1 - t) - (1 - p) with 1 - p = e / (1 + e)
    # (the plain difference, which the reference's autograd forms, is 1e-16 off — invisible next to a gradient of 1 / n, but all
    # there is when every logit is +-30 on the right side of its target)
    e = np.exp(-np.abs(z))
    q = e / (1.0 + e)
    grad = bce_weight * np.where(z >= 0, (1.0 - t) - q, q - t) / n
    pq = q * (1.0 - q)                                     # p (1 - p), the same on both sides
    groups = [slice(b, b + 1) for b in range(B)] if per_sample else [slice(0, B)]
    for g in groups:
        I, P, T = (p[g] * t[g]).sum(), p[g].sum(), t[g].sum()
        D, num = P + T + smooth, 2.0 * I + smooth
        w = dice_weight / len(groups)
        loss += w * (1.0 - num / D)
        grad[g] -= w * (2.0 * t[g] * D - num) / (D * D) * pq[g]
    return float(loss), grad


def dice_loss(z, t, smooth=1.0, per_sample=False):
    return seg_loss(z, t, 0.0, 1.0, smooth, per_sample)
