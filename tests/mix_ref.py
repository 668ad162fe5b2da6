"""numpy restatement of the batch-mixing kernel and the mixed-target cross-entropy (include/mi355conv.h: mi355_mix_batch_f32,
mi355_ce_mix) and of CutMix's box.  It imports nothing from the package; tests/test_mix_cpu.py pins it to torch and to hand-derived
facts, tests/test_gpu_mix.py compares the kernels with it."""
import math

import numpy as np

U = 2.0 ** -24                     # unit roundoff of float32


def mix_batch_ref(x, perm, lam, boxes):
    """x: float32 [N,C,H,W]; perm [N]; lam float32 [N]; boxes [N,4] = (y0, x0, y1, x1), half-open.  float32, one rounding per operation:
    out = b inside the box, fl(fl(lam a) + fl(fl(1 - lam) b)) outside, a = x[n], b = x[perm[n]]."""
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    out = np.empty_like(x)
    ii, jj = np.arange(H)[:, None], np.arange(W)[None, :]
    for n in range(N):
        a, b = x[n], x[int(perm[n])]
        l = np.float32(lam[n])
        oml = np.float32(np.float32(1.0) - l)
        m = (l * a).astype(np.float32) + (oml * b).astype(np.float32)
        y0, x0, y1, x1 = (int(v) for v in boxes[n])
        inside = (ii >= y0) & (ii < y1) & (jj >= x0) & (jj < x1)
        out[n] = np.where(inside[None], b, m.astype(np.float32))
    return out


def soft_targets(ya, yb, lam, C, smoothing):
    """t [B,C] float64 = (1 - s) (lam onehot(ya) + (1 - lam) onehot(yb)) + s / C; yb = lam = None: hard labels"""
    ya = np.asarray(ya, np.int64)
    B = len(ya)
    s = float(smoothing)
    cls = np.arange(C)[None, :]
    if yb is None:
        hot = (cls == ya[:, None]).astype(np.float64)
    else:
        l = np.asarray(lam, np.float64)[:, None]
        hot = l * (cls == ya[:, None]) + (1.0 - l) * (cls == np.asarray(yb, np.int64)[:, None])
    return (1.0 - s) * hot + s / C


def ce_mix_ref(z, ya, yb=None, lam=None, weight=None, smoothing=0.0, gscale=1.0):
    """float64 -> (loss, dz [B,C]):  loss = (1/B) sum_b sum_c w_c t_bc (-log_softmax(z_b)_c),
    dz_bc = (gscale / B) (softmax(z_b)_c sum_k w_k t_bk - w_c t_bc).  The inputs are widened as they are (pass the float32 values the
    kernel is given, ``smoothing`` included)."""
    z = np.asarray(z, np.float64)
    B, C = z.shape
    t = soft_targets(ya, yb, lam, C, smoothing)
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    mx = z.max(1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(1, keepdims=True))
    wt = w[None, :] * t
    loss = float((wt * (lse - z)).sum() / B)
    dz = (float(gscale) / B) * (np.exp(z - lse) * wt.sum(1, keepdims=True) - wt)
    return loss, dz


def ce_smooth_formula(z, y, smoothing):
    """the expression of mi355_ce_smooth (csrc/loss_optim.hip), in float64: -(1 - s) logp[y] - s mean_c logp, averaged over the rows"""
    z = np.asarray(z, np.float64)
    B, C = z.shape
    mx = z.max(1, keepdims=True)
    logp = z - (mx + np.log(np.exp(z - mx).sum(1, keepdims=True)))
    per = -(1.0 - smoothing) * logp[np.arange(B), np.asarray(y, np.int64)] - smoothing * logp.sum(1) / C
    tgt = (1.0 - smoothing) * (np.arange(C)[None, :] == np.asarray(y)[:, None]) + smoothing / C
    return float(per.sum() / B), (np.exp(logp) - tgt) / B


def ce_bound(ref):
    """what a value computed in double and rounded to float32 once may differ from the float64 reference ``ref`` by: one float32
    rounding, 2^-23 |ref| (twice the unit roundoff: room for the double arithmetic to move the value across a rounding boundary), plus
    1e-12 absolute for the double arithmetic itself"""
    return 2.0 ** -23 * np.abs(ref) + 1e-12


def cutmix_box_ref(h, w, lam0, cy, cx):
    """Yun et al.'s box: r = sqrt(1 - lam0), sides int(h r), int(w r) around (cy, cx), clipped -> (y0, x0, y1, x1), and the adjusted
    weight 1 - area / (h w)"""
    r = math.sqrt(1.0 - lam0)
    ch, cw = int(h * r), int(w * r)
    y0, y1 = int(np.clip(cy - ch // 2, 0, h)), int(np.clip(cy + ch // 2, 0, h))
    x0, x1 = int(np.clip(cx - cw // 2, 0, w)), int(np.clip(cx + cw // 2, 0, w))
    return (y0, x0, y1, x1), 1.0 - (y1 - y0) * (x1 - x0) / (h * w)
