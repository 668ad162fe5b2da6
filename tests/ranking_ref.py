"""fp64 numpy restatement of the ranking metrics and the calibration figures as csrc/ranking.hip defines them, and the bounds the GPU
tests hold the device to.  The yardstick of tests/test_ranking_cpu.py (pinned there to scikit-learn, live and through the committed
fixture tests/golden/ranking.npz, and to hand-worked cases) and of the GPU tests.

Ranking.  Per segment: a stable argsort of ``score + 0`` (fp32: -0.0 becomes +0.0), a tie group ends where s[k+1] != s[k], cumulative
counts in int64.  With A_g, B_g the negatives / positives up to and including group g (A_0 = B_0 = 0):
    U2 = sum_g (B_g - B_{g-1}) (A_g + A_{g-1})                       AUROC = U2 / (2 P N)
    ap = sum_g (p_g / P) tp_g / (tp_g + fp_g),  p_g = B_g - B_{g-1},  tp_g = P - B_{g-1},  fp_g = N - A_{g-1}
    operating points (score_g, tp_g, fp_g) in DESCENDING score order (scikit-learn's _binary_clf_curve)
Every integer is exact, so the device has to reproduce it; only ``ap`` is a floating-point sum.

AP_BOUND.  ap is a sum of at most len non-negative terms whose exact sum is <= 1.  Summed in ANY order in double, n such terms err by at
most (n - 1) u, u = 2^-53 (each partial sum is <= 1, each addition rounds once).  A term (p / P) * (tp / (tp + fp)) of exact integers
carries three roundings (two quotients, one product): <= 3 u relative, and the terms add up to <= 1, so <= 3 u in the sum; one more u
for a final rounding -> (len + 4) u.  The same bound holds between any two such evaluations' distance to the exact value, so it is used
one-sided for each and the tests compare against the restatement with it (the restatement's own error is within 2 % of it on every
case tried: lengths 1 .. 65536, continuous / quantised / constant scores, prevalence 0.5 and 0.01).

Calibration.  Softmax in double after subtracting the row maximum; conf = max_j p_j, pred = the first argmax, bin =
min(M - 1, max(0, ceil(conf M) - 1)); NLL_i = log sum_j exp(x_j - max) - (x_y - max) for logits and -log p_y for probabilities;
Brier_i = sum_j (p_j - 1[j = y])^2; ECE = sum_m |correct_m - conf_m| / N.  Sums here are math.fsum (exact, rounded once), so the
restatement's own folds contribute one u — except the NLL's, which is np.mean, the very operation scikit-learn's log_loss ends with, so
that the two are equal to the bit: numpy adds pairwise (eight running sums over blocks of 128, then halves), a chain of at most
np_depth(N) = 19 + max(0, ceil(log2(N / 128))) additions.

Calibration bounds (u = 2^-53; the device's double exp and log are taken at 1 ulp = 2 u relative, as tests/tta_ref.py takes expf: no
accuracy table is installed with the toolchain; numpy's at the same).  x_j - max is the same IEEE operation on both sides.
  PROB_ERR(C) = (2 C + 8) u: e_j = exp(.) differs by <= 4 u relative between the two sides (2 u each); the sum of C positive terms adds
    (C - 1) u per side for the order -> (2 C + 2) u; the quotient e_j / sum: 4 u + (2 C + 2) u + 2 u (one division each side).  p <= 1,
    so this is absolute as well.  With is_prob the probabilities are the inputs: no error, the same bound is kept.
  fold depth(N) = min(N, 256) + ceil(N / 256): the device adds a workgroup's <= 256 samples in order, then the workgroups in order, so a
    sum of n terms <= 1 errs by <= depth(N) n u.
  bin_conf_bound(n_m, N, C) = n_m (PROB_ERR(C) + (depth(N) + 1) u)          (n_m = the bin's count; + 1: the restatement's fsum)
  ece_bound(N, C, M) = PROB_ERR(C) + (depth(N) + 1) u + 4 M u + 2 u: the bins' bounds add up to N (...) and are divided by N; each
    |correct_m - conf_m| <= N rounds once per side (2 M N u), the fold over M bins once more per side (2 M N u), the division u each.
  brier_bound(N, C) = (4 C^2 + 22 C) u + 2 (tree(N) + 2) u: |p_j - o_j| <= 1 is off by PROB_ERR, its square by 2 PROB_ERR + 2 u, C
    of them and C - 1 additions of partial sums <= 2 -> (4 C^2 + 18 C) u + 4 C u per sample; the mean folds N values <= 2 through a
    tree of depth tree(N) = 16 + ceil(N / 65536) (lanes, waves, workgroups) -> 2 tree(N) u, the restatement's fsum and the divisions.
  nll_bound(N, C, L), L >= every |NLL_i|: log(sum) moves by the sum's relative error (2 C + 2) u, plus 2 u |log sum| <= 2 u log C per
    side; -log p_y (probabilities) by 2 u |log p_y| <= 2 u L per side; the subtraction rounds u L per side; the mean folds values <= L
    through the same tree, the restatement's through numpy's -> (2 C + 2 + 4 log C) u + (6 + tree(N) + np_depth(N) + 2) u L.
Every one of them is far below 1e-9 for the shapes of the tests, which assert that."""
import math

import numpy as np

U = 2.0 ** -53


# ---- ranking ---------------------------------------------------------------------------------------------------------------------
def ap_bound(length):
    return (length + 4) * U


def segment_ref(score, y):
    """One segment: fp32 scores [len], bool labels [len] -> dict of P, N, U2, T (Python ints), ap (float, NaN when P = 0), auroc (float,
    NaN when P = 0 or N = 0) and the operating points thresholds (fp32), tp, fp (int32) in descending threshold order."""
    s = np.asarray(score, dtype=np.float32).reshape(-1) + np.float32(0)
    y = np.asarray(y, dtype=bool).reshape(-1)
    assert s.shape == y.shape and s.size >= 1
    order = np.argsort(s, kind="stable")
    ss, ys = s[order], y[order]
    ends = np.r_[ss[1:] != ss[:-1], True]
    B = np.cumsum(ys, dtype=np.int64)[ends]
    A = np.cumsum(~ys, dtype=np.int64)[ends]
    Bp, Ap = np.r_[np.int64(0), B[:-1]], np.r_[np.int64(0), A[:-1]]
    P, N = int(B[-1]), int(A[-1])
    p, tp, fp = B - Bp, P - Bp, N - Ap
    U2 = int(np.sum(p * (A + Ap), dtype=np.int64))
    ap = float(np.sum((p / P) * (tp / (tp + fp)))) if P > 0 else float("nan")
    auroc = U2 / (2.0 * P * N) if P > 0 and N > 0 else float("nan")
    return {"P": P, "N": N, "U2": U2, "T": int(ends.sum()), "ap": ap, "auroc": auroc,
            "thresholds": ss[ends][::-1].copy(), "tp": tp[::-1].astype(np.int32), "fp": fp[::-1].astype(np.int32)}


def rank_ref(scores, target=None, labels=None, thr=0.5):
    """scores fp32 [S, len] with target [S, len] (y = target > thr) or labels [len] (y = labels == s) -> list of segment_ref dicts."""
    scores = np.asarray(scores, dtype=np.float32)
    assert (target is None) != (labels is None)
    out = []
    for s in range(scores.shape[0]):
        y = np.asarray(target)[s] > thr if target is not None else np.asarray(labels) == s
        out.append(segment_ref(scores[s], y))
    return out


def roc_ref(r):
    """segment_ref dict -> (fpr, tpr, thresholds) with sklearn.metrics.roc_curve(drop_intermediate=False)'s conventions."""
    tps, fps = np.r_[0, r["tp"]].astype(np.float64), np.r_[0, r["fp"]].astype(np.float64)
    return fps / fps[-1], tps / tps[-1], np.r_[np.float32(np.inf), r["thresholds"]]


def pr_ref(r):
    """segment_ref dict -> (precision, recall, thresholds) with sklearn.metrics.precision_recall_curve's conventions (P > 0)."""
    tps, fps = r["tp"].astype(np.float64), r["fp"].astype(np.float64)
    return np.r_[(tps / (tps + fps))[::-1], 1.0], np.r_[(tps / tps[-1])[::-1], 0.0], r["thresholds"][::-1].copy()


# ---- calibration -----------------------------------------------------------------------------------------------------------------
def softmax64(x):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    d = x - x.max(1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(1, keepdims=True), d, e


def calibration_ref(x, labels, bins=15, is_prob=False):
    """x fp32 [N, C], labels [N] -> dict: bin_count, bin_correct (int64 [bins]), bin_conf (float64 [bins]), nll, brier, ece (floats),
    scores_t (fp32 [C, N]), and what the tests assert ON THE INPUT: edge_distance (min over samples and bin edges of |conf - k / bins|),
    top2_gap (min over samples of the top two probabilities' difference), nll_max (max |NLL_i|)."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64)
    N, C = x.shape
    if is_prob:
        p = x.astype(np.float64)
        nll_i = -np.log(p[np.arange(N), y])
    else:
        p, d, e = softmax64(x)
        nll_i = np.log(e.sum(1)) - d[np.arange(N), y]
    conf, pred = p.max(1), p.argmax(1)
    b = np.clip(np.ceil(conf * bins).astype(np.int64) - 1, 0, bins - 1)
    onehot = np.zeros_like(p)
    onehot[np.arange(N), y] = 1.0
    brier_i = ((p - onehot) ** 2).sum(1)
    cnt = np.bincount(b, minlength=bins).astype(np.int64)
    ok = np.bincount(b, weights=(pred == y), minlength=bins).astype(np.int64)
    cs = np.array([math.fsum(conf[b == m]) for m in range(bins)])
    srt = np.sort(p, 1)
    return {"bin_count": cnt, "bin_correct": ok, "bin_conf": cs, "nll": float(np.mean(nll_i)), "brier": math.fsum(brier_i) / N,
            "ece": math.fsum(np.abs(ok - cs)) / N, "scores_t": np.ascontiguousarray(p.T).astype(np.float32), "pred": pred, "conf": conf,
            "edge_distance": float(np.abs(conf[:, None] - np.arange(bins + 1)[None] / bins).min()),
            "top2_gap": float((srt[:, -1] - srt[:, -2]).min()) if C > 1 else 1.0, "nll_max": float(np.abs(nll_i).max())}


def prob_err(C):
    return (2 * C + 8) * U


def depth(N):
    return min(N, 256) + -(-N // 256)


def tree(N):
    return 16 + -(-N // 65536)


def np_depth(N):
    return 19 + max(0, math.ceil(math.log2(N / 128.0)))


def bin_conf_bound(n_m, N, C):
    return n_m * (prob_err(C) + (depth(N) + 1) * U)


def ece_bound(N, C, bins):
    return prob_err(C) + (depth(N) + 1) * U + 4 * bins * U + 2 * U


def brier_bound(N, C):
    return (4 * C * C + 22 * C) * U + 2 * (tree(N) + 2) * U


def nll_bound(N, C, L):
    return (2 * C + 2 + 4 * math.log(C)) * U + (6 + tree(N) + np_depth(N) + 2) * U * L


def calibration_inputs(N, C, bins, seed, scale=2.0, is_prob=False, margin=1e-6):
    """Seeded fp32 logits (or, is_prob, their fp32 softmax) [N, C] and labels [N], redrawn until the fp64 confidence is at least
    ``margin`` from every bin edge and the top two probabilities are at least ``margin`` apart.  -> (x, labels, calibration_ref)"""
    for attempt in range(64):
        rng = np.random.RandomState(seed + 7919 * attempt)
        x = (rng.randn(N, C) * scale).astype(np.float32)
        labels = rng.randint(0, C, N).astype(np.int32)
        if is_prob:
            x = softmax64(x)[0].astype(np.float32)
        ref = calibration_ref(x, labels, bins, is_prob)
        if ref["edge_distance"] >= margin and ref["top2_gap"] >= margin:
            return x, labels, ref
    raise AssertionError(f"no seeded input with the margins found (N={N}, C={C}, bins={bins}, seed={seed})")
