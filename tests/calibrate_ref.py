"""fp64 numpy restatement of the post-hoc calibration of csrc/calibrate.hip — the temperature fit and the threshold sweep — and the bounds
the GPU tests hold the device to.  The yardstick of tests/test_calibrate_cpu.py (pinned there to scipy.optimize.brentq, to a brute-force
triple loop and to utils.tester._metrics_from_counts) and of tests/test_gpu_calibrate.py.

Temperature.  beta = 1 / T.  Per row, in double, with z = beta x and m = max_j z_j:
    NLL_i = log sum_j exp(z_j - m) + m - z_y        g'_i = E_p[d] - d_y        g''_i = E_p[(d - E_p[d])^2]
with p = softmax(z) and d = x - max x (exact in double; E_p[x] - x_y = E_p[d] - d_y without the cancellation of a common offset).
g is their mean: the NLL through np.mean as in ranking_ref (scikit-learn's log_loss), g' and g'' through math.fsum.  g'' is the two-pass
variance here; the device's one-pass S2 / S0 - (S1 / S0)^2 only steers Newton's step, so the tests hold it to a relative 1e-9, not to a
derived bound.

``temperature_ref`` restates the iteration of the header: evaluation 1 at beta = 1 (g'' = 0: status 3); evaluation 2 at the end of the
bracket [2^-6, 2^6] that g'(1) points to (no sign change there: status 1 / 2, beta = that end); then Newton on g', replaced by the
bracket's geometric mean when g'' <= 0 or the step leaves the bracket, the bracket shrinking by the sign of g'; it stops AT the evaluated
beta once |dbeta| <= 2^-40 beta (status 0), or after 64 evaluations (status 4).  Its beta and the device's differ in the last bits (other
summation orders), so the tests do not compare the two: they ask of EACH that this restatement's g' changes sign across
[beta (1 - 2^-30), beta (1 + 2^-30)].  That is a statement about beta alone; it is far above the rounding of g' — a few hundred u |d|
— as long as g''(beta) >= 1e-3, which moves g' by >= 1e-3 * 2^-30 beta ~ 1e-12 beta across half the bracket: the tests assert that and
2^-6 < beta < 2^6 on their inputs.  The clamp and flat cases are decided by signs and by exact zeros: status and beta are compared exactly.

TEMP_NLL_BOUND(N, C, L, max|beta x|) = ranking_ref.nll_bound(N, C, L) + 2^-52 max|beta x| between the device's mean NLL and
nll_terms(x, labels, beta_gpu): nll_bound covers exp, log, the row sums in any order and a mean folded through a tree of depth
tree(N) = 16 + ceil(N / 65536); the device's tree is 8 (a workgroup's lanes and waves, or 3 + 2 with a wave per row) + 8 + ceil(nb / 256)
over its nb <= N / 16 workgroups — not deeper for N <= 2^16, which the tests stay below.  The second term is the exponent's argument:
the device forms beta (x_j - max x) (one rounding, <= u |beta d|), the restatement fl(beta x_j) - fl(beta max x); averaged over a row's terms
and over the rows they differ by no more than 2 u max|beta x|.

Sweep.  v = the score (fp32), or with is_logit the fp64 sigmoid of the logit; bin = np.searchsorted(thr, v, side="left") = #{k : v >
thr[k]} for ascending thr, 0 for a NaN; positive where target > tthr;
    tp[b][k] = #{positive pixels with bin > k}     fp[b][k] = the same over the negatives     pos[b] = the positives
Exact integers: the device has to reproduce them.  The device's is_logit path is the fp32 expression 1.f / (1.f + __expf(-v)): the tests
draw logits whose fp64 sigmoid is at least 2^-20 from every candidate (``logit_margin``) — __expf is good to a few ulp of fp32, 2^-22 of
a value <= 1 — so the bin is decided whatever its last bits.

Fold.  Per image and candidate, in double, pp = tp + fp, tt = pos:
    Dice = (2 tp + 1e-7) / (pp + tt + 1e-7)        IoU = (tp + 1e-7) / (pp + tt - tp + 1e-7)
added image by image to running sums.  FOLD_BOUND(n) = (n + 4) u per candidate, u = 2^-53, on the sums over n images.  Every term is
<= 1 (2 tp <= pp + tt, tp <= union) and is formed by the same correctly rounded IEEE operations on both sides (2 tp, pp + tt and the
union are exact integers, so a fused multiply-add changes nothing); the fold order is fixed — image order, batch after batch — and is the
order of ``fold_ref``, so the two sums are the same chain of additions: the bound is headroom (four roundings of a term and one per
image), not something the chain needs.  ``pick_ref`` divides by n once (<= u relative, monotone) and takes the lowest index of the
largest mean Dice; two candidates whose restated means differ by more than 2 FOLD_BOUND(n) cannot swap places on the device."""
import math

import numpy as np

import ranking_ref as R

U = 2.0 ** -53
BETA_LO, BETA_HI = 2.0 ** -6, 2.0 ** 6
STEP_TOL = 2.0 ** -40
MAX_EVALS = 64
DEFAULT_THRESHOLDS = np.arange(1, 256, dtype=np.float32) / np.float32(256)


# ---- temperature -----------------------------------------------------------------------------------------------------------------
def nll_terms(x, labels, beta):
    """x fp32 [N, C], labels [N], beta -> dict: nll, g1, g2 (floats: g, g', g'' at beta), nll_max (max |NLL_i|), zmax (max |beta x|)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    y = np.asarray(labels).astype(np.int64)
    N = x.shape[0]
    rows = np.arange(N)
    z = beta * x
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1)
    nll_i = np.log(s) + m[:, 0] - z[rows, y]
    p = e / s[:, None]
    d = x - x.max(1, keepdims=True)
    mean = (p * d).sum(1)
    g1_i = mean - d[rows, y]
    g2_i = (p * (d - mean[:, None]) ** 2).sum(1)
    return {"nll": float(np.mean(nll_i)), "g1": math.fsum(g1_i) / N, "g2": math.fsum(g2_i) / N,
            "nll_max": float(np.abs(nll_i).max()), "zmax": float(np.abs(z).max())}


def temperature_ref(x, labels):
    """-> dict: beta, T, nll_before (at beta = 1), nll, g1, g2 (at beta), evals, status — mi355_temperature_fit's state"""
    lo, hi, beta, cand, phase, status, evals = BETA_LO, BETA_HI, 1.0, 1.0, 0, -1, 0
    nll_before = None
    while status < 0:
        t = nll_terms(x, labels, beta)
        evals += 1
        g1, g2 = t["g1"], t["g2"]
        if evals == 1:
            nll_before = t["nll"]
        nxt = beta
        if g1 != g1 or g2 != g2:
            status = 4
        elif phase == 0:
            if not g2 > 0.0:
                status = 3
            elif g1 == 0.0:
                status = 0
            else:
                cand = beta - g1 / g2
                if g1 < 0.0:
                    lo, nxt = beta, hi
                else:
                    hi, nxt = beta, lo
                phase = 1
        elif phase == 1:
            if beta > 1.0 and g1 <= 0.0:
                status = 2
            elif beta < 1.0 and g1 >= 0.0:
                status = 1
            else:
                nxt = cand if lo < cand < hi else math.sqrt(lo * hi)
                phase = 2
        elif g1 == 0.0:
            status = 0
        else:
            if g1 > 0.0:
                hi = beta
            else:
                lo = beta
            nxt = beta - g1 / g2
            if not g2 > 0.0 or (abs(nxt - beta) > STEP_TOL * beta and not lo < nxt < hi):
                nxt = math.sqrt(lo * hi)
            if abs(nxt - beta) <= STEP_TOL * beta:
                status = 0
        if status < 0 and evals >= MAX_EVALS:
            status = 4
        if status < 0:
            beta = nxt
    return {"beta": beta, "T": 1.0 / beta, "nll_before": nll_before, "nll": t["nll"], "g1": g1, "g2": g2, "evals": evals,
            "status": status}


def sign_change(x, labels, beta, rel=2.0 ** -30):
    """does the restated g' change sign (or vanish) across [beta (1 - rel), beta (1 + rel)]?  -> (bool, g' below, g' above)"""
    a, b = nll_terms(x, labels, beta * (1.0 - rel))["g1"], nll_terms(x, labels, beta * (1.0 + rel))["g1"]
    return a <= 0.0 <= b, a, b


def temp_nll_bound(N, C, L, zmax):
    return R.nll_bound(N, C, L) + 2.0 ** -52 * zmax


def temperature_inputs(N, C, T0, seed, scale=2.0):
    """Seeded fp32 logits scale * randn [N, C] with labels drawn from softmax(x / T0): the optimum is interior, near beta = 1 / T0."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(N, C) * scale).astype(np.float32)
    p = R.softmax64(x / np.float32(T0))[0]
    u = rng.rand(N, 1)
    labels = np.minimum((p.cumsum(1) < u).sum(1), C - 1).astype(np.int32)
    return x, labels


# ---- threshold sweep -------------------------------------------------------------------------------------------------------------
def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float32).astype(np.float64)))


def logit_margin(logits, thr):
    """the smallest distance of an fp64 sigmoid to a candidate"""
    return float(np.abs(sigmoid64(logits).reshape(-1, 1) - np.asarray(thr, dtype=np.float32).astype(np.float64).reshape(1, -1)).min())


def bins_ref(scores, thr, is_logit=False):
    thr = np.asarray(thr, dtype=np.float32)
    v = np.asarray(scores, dtype=np.float32)
    if is_logit:
        v, thr = sigmoid64(v), thr.astype(np.float64)
    b = np.searchsorted(thr, v, side="left")
    b[np.isnan(v)] = 0
    return b


def sweep_ref(scores, target, thr, is_logit=False, tthr=0.5):
    """scores, target fp32 [B, len], thr fp32 [K] ascending -> (tp int32 [B, K], fp int32 [B, K], pos int32 [B])"""
    scores = np.asarray(scores, dtype=np.float32)
    B, K = scores.shape[0], len(thr)
    y = np.asarray(target, dtype=np.float32) > np.float32(tthr)
    b = bins_ref(scores, thr, is_logit)
    tp, fp = np.zeros((B, K), np.int32), np.zeros((B, K), np.int32)
    for i in range(B):
        hp = np.bincount(b[i][y[i]], minlength=K + 1).astype(np.int64)
        hn = np.bincount(b[i][~y[i]], minlength=K + 1).astype(np.int64)
        tp[i] = (hp[::-1].cumsum()[::-1])[1:]
        fp[i] = (hn[::-1].cumsum()[::-1])[1:]
    return tp, fp, y.sum(1).astype(np.int32)


def fold_bound(n):
    return (n + 4) * U


def dice_iou(tp, fp, pos):
    """int arrays [B, K], [B, K], [B] -> (Dice, IoU) float64 [B, K]: tester._metrics_from_counts without the x 100"""
    t = np.asarray(tp, dtype=np.float64)
    pp = t + np.asarray(fp, dtype=np.float64)
    tt = np.asarray(pos, dtype=np.float64)[:, None]
    return (2.0 * t + 1e-7) / ((pp + tt) + 1e-7), (t + 1e-7) / (((pp + tt) - t) + 1e-7)


def fold_ref(batches, K):
    """[(tp, fp, pos), ...] -> (acc float64 [2, K], n): the running sums in image order, batch after batch"""
    acc, n = np.zeros((2, K), np.float64), 0
    for tp, fp, pos in batches:
        d, j = dice_iou(tp, fp, pos)
        for b in range(d.shape[0]):
            acc[0] += d[b]
            acc[1] += j[b]
            n += 1
    return acc, n


def pick_ref(acc, n, k_ref):
    """-> (k, mean Dice at k, mean IoU at k, mean Dice at k_ref, mean IoU at k_ref, the runner-up's distance: best mean Dice minus the
    largest mean Dice that is not equal to it, inf when every candidate ties)"""
    mean = acc / float(n)
    k = int(np.argmax(mean[0]))                    # the first maximum
    rest = mean[0][mean[0] < mean[0][k]]
    gap = float(mean[0][k] - rest.max()) if rest.size else float("inf")
    ref = (float(mean[0][k_ref]), float(mean[1][k_ref])) if k_ref >= 0 else (float("nan"), float("nan"))
    return k, float(mean[0][k]), float(mean[1][k]), ref[0], ref[1], gap
