"""fp64 numpy statement of the knowledge-distillation losses and of their gradients (csrc/distill.hip: mi355_kd_seg_*, mi355_ce_distill;
mi355.nn.SegDistillationLoss / DistillCrossEntropyLoss), used by tests/test_distill_cpu.py and tests/test_gpu_distill.py.

Binary segmentation, n = z.size, a = z / T, b = v / T, p_T = sigmoid(a), q = sigmoid(b):

    KD         = T^2 / n sum_i (softplus(-a_i) - softplus(-b_i) + (1 - q_i)(a_i - b_i))       = T^2 mean KL(Bern(q) || Bern(p_T))
    loss       = (hard, tests/seg_loss_ref.py::seg_loss) + kd_weight KD
    dloss/dz_i = (hard gradient) + kd_weight T (p_T,i - q_i) / n

Classifiers, z, v [B, C], hard labels y:

    KD          = T^2 / B sum_b sum_c q_bc (log q_bc - log p_bc),   p = softmax(z / T), q = softmax(v / T)
    loss        = hard_weight (hard, tests/mix_ref.py::ce_mix_ref on hard labels) + kd_weight KD
    dloss/dz_bc = hard_weight (hard gradient) + kd_weight T (p_bc - q_bc) / B

Both return ([total, hard, KD], gradient), the gradient times ``gscale``.  PINNED: tests/test_distill_cpu.py holds these closed forms to
torch's fp64 autograd (binary_cross_entropy_with_logits + Dice + T^2 kl_div; cross_entropy with probability targets + T^2 kl_div) to
1e-12.  Plain numpy, nothing shared with the library or with torch."""
import numpy as np

from mix_ref import ce_mix_ref
from seg_loss_ref import seg_loss


def softplus(x):
    """log(1 + exp(x)), stable for both signs"""
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid_diff(a, b):
    """sigmoid(a) - sigmoid(b) without the cancellation against 1: on the same side of 0 it is the difference of the two small tails
    sigmoid(-|x|) = e / (1 + e), e = exp(-|x|)"""
    ea, eb = np.exp(-np.abs(a)), np.exp(-np.abs(b))
    la, lb = ea / (1.0 + ea), eb / (1.0 + eb)                # sigmoid(-|a|), sigmoid(-|b|)
    sa, sb = 1.0 / (1.0 + ea), 1.0 / (1.0 + eb)              # sigmoid(|a|), sigmoid(|b|)
    pa, pb = a >= 0, b >= 0
    return np.where(pa & pb, lb - la, np.where(~pa & ~pb, la - lb, np.where(pa, sa - lb, la - sb)))


def kd_seg(z, t, v, bce_weight=0.5, dice_weight=0.5, smooth=1.0, per_sample=False, kd_weight=0.5, temperature=2.0, gscale=1.0):
    """-> ([total, hard, KD] floats, dloss/dz float64 of z's shape).  ``v`` None with kd_weight 0: the hard loss alone."""
    z = np.asarray(z, np.float64)
    hard, g = seg_loss(z, t, bce_weight, dice_weight, smooth, per_sample)
    kd = 0.0
    if kd_weight != 0:
        T = float(temperature)
        a, b = z / T, np.asarray(v, np.float64).reshape(z.shape) / T
        eb = np.exp(-np.abs(b))
        omq = np.where(b >= 0, eb / (1.0 + eb), 1.0 / (1.0 + eb))          # 1 - q
        kd = T * T * float((softplus(-a) - softplus(-b) + omq * (a - b)).sum()) / z.size
        g = g + kd_weight * T * sigmoid_diff(a, b) / z.size
    return [hard + kd_weight * kd, hard, kd], float(gscale) * g


def ce_distill(z, y, v, weight=None, smoothing=0.0, hard_weight=0.5, kd_weight=0.5, temperature=4.0, gscale=1.0):
    """-> ([total, hard, KD] floats, dloss/dz float64 [B, C]).  ``v`` None with kd_weight 0: the hard loss alone."""
    z = np.asarray(z, np.float64)
    B = z.shape[0]
    hard, gh = ce_mix_ref(z, y, None, None, weight, smoothing, 1.0)
    kd, g = 0.0, hard_weight * gh
    if kd_weight != 0:
        T = float(temperature)
        a, b = z / T, np.asarray(v, np.float64) / T
        lp = a - (a.max(1, keepdims=True) + np.log(np.exp(a - a.max(1, keepdims=True)).sum(1, keepdims=True)))
        lq = b - (b.max(1, keepdims=True) + np.log(np.exp(b - b.max(1, keepdims=True)).sum(1, keepdims=True)))
        kd = T * T * float((np.exp(lq) * (lq - lp)).sum()) / B
        g = g + kd_weight * T * (np.exp(lp) - np.exp(lq)) / B
    return [hard_weight * hard + kd_weight * kd, hard, kd], float(gscale) * g
