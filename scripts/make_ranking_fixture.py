"""Writes tests/golden/ranking.npz: scikit-learn's own outputs on small seeded ranking and calibration problems, so that the numpy
restatement tests/ranking_ref.py stays pinned to scikit-learn on a machine without it (tests/test_ranking_cpu.py reads the file).

    python scripts/make_ranking_fixture.py

Per ranking case ``<len>_<kind>_<prevalence>``: s__ (fp32 scores), y__ (labels), auroc__, ap__ (roc_auc_score, average_precision_score),
roc_fpr__ / roc_tpr__ / roc_thr__ (roc_curve(drop_intermediate=False)), pr_p__ / pr_r__ / pr_thr__ (precision_recall_curve).  Per
calibration case ``<N>x<C>``: cx__ (fp32 probabilities), cy__ (labels), nll__ (log_loss).  Both classes occur in every ranking case."""
import os
import sys

import numpy as np
from sklearn import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ranking.npz")

LENGTHS = (5, 33, 64, 130)
KINDS = ("continuous", "quantised", "constant", "two_valued", "signed_zeros")
PREVALENCE = (0.5, 0.1)


def scores_of(kind, n, rng):
    if kind == "continuous":
        return rng.randn(n).astype(np.float32)
    if kind == "quantised":
        return (np.round(rng.randn(n) * 4) / 4).astype(np.float32)              # multiples of 0.25: ties
    if kind == "constant":
        return np.full(n, 0.75, dtype=np.float32)
    if kind == "two_valued":
        return np.where(rng.rand(n) < 0.5, np.float32(-1.5), np.float32(2.0)).astype(np.float32)
    z = np.round(rng.randn(n)).astype(np.float32)                               # integers, the zeros of both signs: one tie group
    z[(z == 0) & (rng.rand(n) < 0.5)] = np.float32(-0.0)
    return z


def main():
    data, cases = {}, []
    for n in LENGTHS:
        for ki, kind in enumerate(KINDS):
            prev = PREVALENCE[(ki + LENGTHS.index(n)) % 2]
            rng = np.random.RandomState(1000 * n + ki)
            s = scores_of(kind, n, rng)
            y = rng.rand(n) < prev
            y[0], y[-1] = True, False                                           # both classes occur
            name = f"{n}_{kind}_{prev}"
            cases.append(name)
            s_in = s + np.float32(0)                                            # scikit-learn sorts bit patterns of equal zeros alike
            fpr, tpr, thr = metrics.roc_curve(y, s_in, drop_intermediate=False)
            pp, rr, pthr = metrics.precision_recall_curve(y, s_in)
            data.update({"s__" + name: s, "y__" + name: y, "auroc__" + name: np.float64(metrics.roc_auc_score(y, s_in)),
                         "ap__" + name: np.float64(metrics.average_precision_score(y, s_in)),
                         "roc_fpr__" + name: fpr, "roc_tpr__" + name: tpr, "roc_thr__" + name: thr,
                         "pr_p__" + name: pp, "pr_r__" + name: rr, "pr_thr__" + name: pthr})
    cal = []
    for N, C in ((6, 3), (65, 2), (257, 5)):
        rng = np.random.RandomState(N + C)
        z = rng.randn(N, C) * 2
        p = np.exp(z - z.max(1, keepdims=True))
        p = (p / p.sum(1, keepdims=True)).astype(np.float32)
        y = rng.randint(0, C, N)
        y[:C] = np.arange(C)
        name = f"{N}x{C}"
        cal.append(name)
        data.update({"cx__" + name: p, "cy__" + name: y.astype(np.int32),
                     "nll__" + name: np.float64(metrics.log_loss(y, p.astype(np.float64), labels=np.arange(C)))})
    np.savez_compressed(OUT, cases=np.array(cases), calibration_cases=np.array(cal), **data)
    print(f"{OUT}: {len(cases)} ranking cases, {len(cal)} calibration cases, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
