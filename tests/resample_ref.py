"""numpy restatement of csrc/resample.hip as include/mi355conv.h defines it, and the bounds the GPU tests hold the device to.  The
yardstick of tests/test_resample_cpu.py (pinned there to the Random123 known-answer vectors, scikit-learn, scipy and a Fraction
evaluation of DeLong's definition) and of tests/test_gpu_resample.py.

Weights.  Philox4x32-10 in uint64 arithmetic: per round (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1,
lo(M0 c0)), the key bumped by the Weyl constants between rounds.  Draw k of replicate r is word k & 3 of the block with counter
(k >> 2, r, 0, 0) and key (seed & 0xffffffff, seed >> 32); idx = (word * n) >> 32.  Row 0 is ones.

Everything else is the unweighted definition applied to the resample written out with np.repeat: the weighted statistics of the device
have to equal the plain statistics of the expanded arrays.  Integers are exact.  The floating-point bounds (u = 2^-53):
  ap: ranking_ref.ap_bound(len) = (len + 4) u, derived there for any order of the at most len terms; the restatement's own sum is
    math.fsum, so all of the bound is the device's.
  sums: sum_i w_i v_i over n terms: each product rounds once (u |w v|), a sum in any order adds (n - 1) u sum |w v| -> (n + 4) u sum |w v|.
  interval: lo / hi are one interpolation between two neighbours: 1 ulp.  mean of R values: (R + 4) u mean |v|.  se: the centred squares
    are summed (<= (R + 4) u relative, every term positive) after centring with a mean that is off by (R + 4) u mean|v|; with a spread
    of at least a tenth of the mean that moves each deviation by <= 10 (R + 4) u of the spread -- the bound 8 (R + 4) u relative of the
    issue is held on inputs whose spread is well above that (asserted by the tests).
  DeLong: cov = S10 / ((P - 1) P) + S01 / ((N - 1) N), S = sum of centred products.  Summing n products in any order errs by
    <= (n - 1) u sum |product|, and each product carries about six roundings of its own (two quotients, two centrings by a mean formed
    from an exact integer sum, the product): <= (n + 10) u `mag`, mag = the same expression evaluated with |product| (returned by
    delong_ref).  For a variance mag is the variance.  The bound of the tests is 8 (n + 4) u RELATIVE TO |cov|; for a covariance that
    follows where |cov| >= mag / 4 (4 (n + 10) <= 8 (n + 4) from n = 2), which the tests assert of their inputs: two models that
    agree on half the samples.  (Where two models are uncorrelated the covariance is a small remainder of cancelling products and no
    relative bound holds for any summation.)"""
import math
from fractions import Fraction

import numpy as np

import ranking_ref

U = 2.0 ** -53
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """counter uint [..., 4], key uint [..., 2] (broadcast against each other) -> uint32 [..., 4]"""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def draws_ref(seed, r, n):
    """the n sample indices replicate r draws, in draw order"""
    nb = (n + 3) // 4
    ctr = np.zeros((nb, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nb)
    ctr[:, 1] = r
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    words = philox4x32(ctr, key).reshape(-1)[:n].astype(np.uint64)
    return ((words * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def counts_ref(seed, R, n):
    out = np.ones((R + 1, n), dtype=np.int32)
    for r in range(1, R + 1):
        out[r] = np.bincount(draws_ref(seed, r, n), minlength=n)
    return out


def expand(w, *arrays):
    """the resample written out: every array's element i repeated w[i] times"""
    return [np.repeat(np.asarray(a), np.asarray(w), axis=-1) for a in arrays]


def weighted_segment_ref(score, y, w):
    """one segment under integer weights -> P, N, U2 (Python ints), ap (math.fsum over the groups with positives; NaN when P = 0),
    auroc (NaN when P N = 0): ranking_ref.segment_ref's definitions on the expanded arrays."""
    s, yy = expand(w, np.asarray(score, dtype=np.float32), np.asarray(y, dtype=bool))
    if s.size == 0:
        return {"P": 0, "N": 0, "U2": 0, "ap": float("nan"), "auroc": float("nan")}
    s = s + np.float32(0)
    order = np.argsort(s, kind="stable")
    ss, ys = s[order], yy[order]
    ends = np.r_[ss[1:] != ss[:-1], True]
    B = np.cumsum(ys, dtype=np.int64)[ends]
    A = np.cumsum(~ys, dtype=np.int64)[ends]
    Bp, Ap = np.r_[np.int64(0), B[:-1]], np.r_[np.int64(0), A[:-1]]
    P, N = int(B[-1]), int(A[-1])
    p, tp, fp = B - Bp, P - Bp, N - Ap
    U2 = int(np.sum(p * (A + Ap), dtype=np.int64))
    ap = math.fsum(((p / P) * (tp / (tp + fp)))[p > 0]) if P > 0 else float("nan")
    return {"P": P, "N": N, "U2": U2, "ap": ap, "auroc": U2 / (2.0 * P * N) if P > 0 and N > 0 else float("nan")}


def boot_rank_ref(scores, counts, target=None, labels=None, thr=0.5):
    """scores fp32 [S, len], counts [R1, len] -> nested list [R1][S] of weighted_segment_ref dicts"""
    scores = np.asarray(scores, dtype=np.float32)
    assert (target is None) != (labels is None)
    ys = [np.asarray(target)[s] > thr if target is not None else np.asarray(labels) == s for s in range(scores.shape[0])]
    return [[weighted_segment_ref(scores[s], ys[s], w) for s in range(scores.shape[0])] for w in counts]


def confusion_ref(pred, labels, C, counts):
    """-> (int64 [R1, C, C], rows the truth; int64 [R1] weight of the samples with an id outside 0 .. C - 1)"""
    pred, labels = np.asarray(pred, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    ok = (pred >= 0) & (pred < C) & (labels >= 0) & (labels < C)
    cm = np.zeros((len(counts), C, C), dtype=np.int64)
    for r, w in enumerate(counts):
        np.add.at(cm[r], (labels[ok], pred[ok]), np.asarray(w, dtype=np.int64)[ok])
    return cm, np.array([int(np.asarray(w, dtype=np.int64)[~ok].sum()) for w in counts], dtype=np.int64)


def sums_ref(values, counts):
    """values float64 [M, n] -> (sum [R1, M] by math.fsum, weight int64 [R1, M], sum of |w v| [R1, M]) over the non-NaN values"""
    values = np.asarray(values, dtype=np.float64)
    R1, M = len(counts), values.shape[0]
    s, wt, mag = np.zeros((R1, M)), np.zeros((R1, M), dtype=np.int64), np.zeros((R1, M))
    for r, w in enumerate(counts):
        for m in range(M):
            ok = ~np.isnan(values[m])
            prod = np.asarray(w, dtype=np.float64)[ok] * values[m][ok]
            s[r, m], wt[r, m], mag[r, m] = math.fsum(prod), int(np.asarray(w, dtype=np.int64)[ok].sum()), math.fsum(np.abs(prod))
    return s, wt, mag


def interval_ref(reps, lo_q, hi_q):
    """reps float64 [R1, K] -> float64 [K, 6] = point, mean, se (ddof = 1), lo, hi, valid over the non-NaN rows 1 .. R"""
    reps = np.asarray(reps, dtype=np.float64)
    out = np.full((reps.shape[1], 6), np.nan)
    for k in range(reps.shape[1]):
        v = reps[1:, k]
        v = v[~np.isnan(v)]
        out[k, 0], out[k, 5] = reps[0, k], v.size
        if v.size >= 1:
            out[k, 1] = math.fsum(v) / v.size
            out[k, 3], out[k, 4] = np.quantile(v, lo_q, method="linear"), np.quantile(v, hi_q, method="linear")
        if v.size >= 2:
            out[k, 2] = math.sqrt(math.fsum((v - out[k, 1]) ** 2) / (v.size - 1))
    return out


def delong_components(x, y):
    """fp32 scores of the positives x [P] and the negatives y [N] -> twice the placement counts, by the O(P N) definition:
    for positive i  2 #{y < x_i} + #{y == x_i}   (= 2 N V10_i),  for negative j  2 #{x > y_j} + #{x == y_j}   (= 2 P V01_j)"""
    x, y = np.asarray(x, dtype=np.float32)[:, None], np.asarray(y, dtype=np.float32)[None, :]
    psi2 = 2 * (x > y).astype(np.int64) + (x == y).astype(np.int64)
    return psi2.sum(1), psi2.sum(0)


def delong_ref(scores, labels):
    """scores fp32 [M, C, n], labels [n] -> dict: v2 int64 [M, C, n], pnu int64 [M, C, 3], var [M, C], cov [C, M, M] and mag [C, M, M],
    the same expression as cov with the absolute centred products (what the device's rounding is relative to)"""
    scores, labels = np.asarray(scores, dtype=np.float32), np.asarray(labels)
    M, C, n = scores.shape
    v2, pnu = np.zeros((M, C, n), dtype=np.int64), np.zeros((M, C, 3), dtype=np.int64)
    cov, mag = np.full((C, M, M), np.nan), np.full((C, M, M), np.nan)
    for c in range(C):
        pos = labels == c
        P, N = int(pos.sum()), int(n - pos.sum())
        for m in range(M):
            a, b = delong_components(scores[m, c][pos], scores[m, c][~pos])
            v2[m, c][pos], v2[m, c][~pos] = a, b
            pnu[m, c] = (P, N, int(a.sum()))
        if P < 2 or N < 2:
            continue
        V10 = v2[:, c][:, pos] / (2.0 * N)
        V01 = v2[:, c][:, ~pos] / (2.0 * P)
        d10, d01 = V10 - V10.mean(1, keepdims=True), V01 - V01.mean(1, keepdims=True)
        for a in range(M):
            for b in range(M):
                cov[c, a, b] = math.fsum(d10[a] * d10[b]) / (P - 1) / P + math.fsum(d01[a] * d01[b]) / (N - 1) / N
                mag[c, a, b] = math.fsum(np.abs(d10[a] * d10[b])) / (P - 1) / P + math.fsum(np.abs(d01[a] * d01[b])) / (N - 1) / N
    var = np.stack([np.array([cov[c, m, m] for c in range(C)]) for m in range(M)])
    return {"v2": v2, "pnu": pnu, "var": var, "cov": cov, "mag": mag}


def delong_cov_fraction(xa, ya, xb, yb):
    """DeLong's covariance of two AUROCs on the same samples in exact rational arithmetic, straight from the definition (the scores of
    the positives x and the negatives y under models a and b) -> Fraction"""
    def placements(x, y):
        psi = [[Fraction(1) if xi > yj else Fraction(1, 2) if xi == yj else Fraction(0) for yj in y] for xi in x]
        return [sum(row) / len(y) for row in psi], [sum(psi[i][j] for i in range(len(x))) / len(x) for j in range(len(y))]

    def cov(u, v):
        mu, mv = sum(u) / len(u), sum(v) / len(v)
        return sum((p - mu) * (q - mv) for p, q in zip(u, v)) / (len(u) - 1)

    (a10, a01), (b10, b01) = placements(xa, ya), placements(xb, yb)
    return cov(a10, b10) / len(xa) + cov(a01, b01) / len(ya)


def mcnemar_ref(b, c):
    """exact two-sided binomial p of the discordant counts: min(1, 2 P(X <= min(b, c))), X ~ Bin(b + c, 1 / 2)"""
    n, k = b + c, min(b, c)
    return min(1.0, float(Fraction(2 * sum(math.comb(n, i) for i in range(k + 1)), 2 ** n)))


def ap_bound(length):
    return ranking_ref.ap_bound(length)
