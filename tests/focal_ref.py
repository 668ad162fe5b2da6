"""fp64 numpy statement of the focal + (focal-)Tversky segmentation loss and of the focal cross-entropy, with their gradients in
closed form (csrc/focal_tversky.hip; mi355.nn.FocalTverskyLoss / FocalLoss / TverskyLoss / FocalCrossEntropyLoss), used by
tests/test_focal_cpu.py and tests/test_gpu_focal.py.

Segmentation, on logits z and targets binarised as t = (target > 0.5), p = sigmoid(z), n = z.size:

    focal_i = alpha_t (1 - p_t)^gamma ce_i,   p_t = t p + (1 - t)(1 - p),   ce = BCEWithLogits(z, t),
              alpha_t = alpha t + (1 - alpha)(1 - t), or 1 where alpha < 0          (torchvision.ops.sigmoid_focal_loss)
    TI      = (I + smooth) / (I + a FP + b FN + smooth),   I = sum p t,  FP = sum p (1 - t),  FN = sum (1 - p) t
    loss    = focal_weight mean_i(focal_i) + tversky_weight (1 - TI)^g

``per_sample=True``: TI and its term per image (first axis), the B terms averaged; the focal term is unchanged.  Where 1 - TI <= 0
the Tversky term and its (sub-)gradient are 0.

Classifiers, on logits z [B, C] with labels y, p = softmax(z_b), py = p[y_b], u = sum_{c != y_b} p_c:

    loss = (1 / B) sum_b w[y_b] u^gamma (-log py)

PINNED: tests/test_focal_cpu.py holds these formulas to torch's fp64 autograd of the same expressions written with torch ops.
Nothing here shares code with the library or with torch: plain numpy, the gradients in closed form."""
import numpy as np


def _parts(z, t):
    """p_t, u = 1 - p_t, ce = -log p_t, p (1 - p), p — all from e = exp(-|z|), without a 1 - p cancellation"""
    e = np.exp(-np.abs(z))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)             # sigmoid(|z|), sigmoid(-|z|)
    agree = (z >= 0) == (t > 0.5)                           # the logit is on its target's side
    pt, u = np.where(agree, big, small), np.where(agree, small, big)
    ce = np.where(agree, 0.0, np.abs(z)) + np.log1p(e)
    return pt, u, ce, big * small, np.where(z >= 0, big, small)


def _pow(u, gamma):
    """u^gamma with 0^0 = 1 and 0^gamma = 0"""
    if gamma == 0:
        return np.ones_like(u)
    return np.where(u > 0, np.power(np.where(u > 0, u, 1.0), gamma), 0.0)


def ftv_loss(z, target, focal_weight=0.0, tversky_weight=1.0, alpha=0.7, beta=0.3, exponent=0.75, focal_alpha=0.25, focal_gamma=2.0,
             smooth=1.0, per_sample=False, gscale=1.0):
    """-> (loss: float, gscale * dloss/dz: float64 array of z's shape)."""
    z = np.asarray(z, dtype=np.float64)
    t = (np.asarray(target, dtype=np.float64).reshape(z.shape) > 0.5).astype(np.float64)
    B, n = z.shape[0], z.size
    pt, u, ce, pq, p = _parts(z, t)
    at = np.ones_like(z) if focal_alpha < 0 else focal_alpha * t + (1.0 - focal_alpha) * (1.0 - t)
    ug = _pow(u, focal_gamma)
    loss = focal_weight * (at * ug * ce).sum() / n
    grad = focal_weight / n * at * ug * (2.0 * t - 1.0) * (-focal_gamma * pt * ce - u)
    groups = [slice(b, b + 1) for b in range(B)] if per_sample else [slice(0, B)]
    a, b_, g = float(alpha), float(beta), float(exponent)
    for s in groups:
        I, P, T = (p[s] * t[s]).sum(), p[s].sum(), t[s].sum()
        num = I + smooth
        den = I + a * (P - I) + b_ * (T - I) + smooth
        ome = (a * (P - I) + b_ * (T - I)) / den if den > 0 else 0.0          # 1 - TI
        if not ome > 0:
            continue
        w = tversky_weight / len(groups)
        loss += w * ome ** g
        A = w * g * ome ** (g - 1.0) / den
        C = A * num / den
        grad[s] -= (A * t[s] - C * (a + (1.0 - a - b_) * t[s])) * pq[s]
    return float(loss), float(gscale) * grad


def focal_loss(z, target, alpha=0.25, gamma=2.0):
    return ftv_loss(z, target, 1.0, 0.0, focal_alpha=alpha, focal_gamma=gamma)


def tversky_loss(z, target, alpha=0.5, beta=0.5, smooth=1.0, per_sample=False):
    return ftv_loss(z, target, 0.0, 1.0, alpha, beta, 1.0, smooth=smooth, per_sample=per_sample)


def ce_focal(z, y, weight=None, gamma=2.0, gscale=1.0):
    """-> (loss, dz [B, C]):  dz_bc = (gscale / B) w[y_b] ([c == y_b] - p_c) (gamma py u^(gamma - 1) log py - u^gamma), written as
    dz_by = k G, dz_bc = -k r_c G with G = u^gamma (gamma py log py - u) and r_c = p_c / u = the softmax over the classes other than
    y_b: no division by u."""
    z = np.asarray(z, np.float64)
    B, C = z.shape
    y = np.asarray(y, np.int64)
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    hot = np.arange(C)[None, :] == y[:, None]
    mx = z.max(1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(1, keepdims=True))
    logp = z - lse
    logpy = logp[hot]
    py = np.exp(logpy)
    u = np.where(hot, 0.0, np.exp(logp)).sum(1)
    zo = np.where(hot, -np.inf, z)
    if C > 1:
        mo = zo.max(1, keepdims=True)
        eo = np.exp(zo - mo)
        r = eo / eo.sum(1, keepdims=True)
    else:
        r = np.zeros_like(z)
    ug = _pow(u, gamma)
    wy = w[y]
    loss = float((wy * ug * -logpy).sum() / B)
    G = (float(gscale) / B) * wy * ug * (gamma * py * logpy - u)
    dz = np.where(hot, G[:, None], -r * G[:, None])
    return loss, dz
