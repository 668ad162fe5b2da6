"""The yardstick of the resampling kernels (tests/resample_ref.py) pinned on the CPU: Philox against the Random123 known-answer vectors,
the weighted ranking metrics against scikit-learn's sample_weight, DeLong's covariance against a Fraction evaluation of the definition,
McNemar's p against scipy's exact binomial test — and the ABI the device side is declared with."""
import ctypes
import math

import numpy as np
import pytest

import resample_ref as RR
from mi355.lib import parse_header


@pytest.mark.parametrize("counter, key, expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, expect):
    got = RR.philox4x32(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(v) for v in got] == list(expect), [hex(int(v)) for v in got]


def test_philox_is_vectorised_consistently():
    ctr = np.array([[0, 0, 0, 0], [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], dtype=np.uint64)
    key = np.array([0xa4093822, 0x299f31d0], dtype=np.uint64)
    both = RR.philox4x32(ctr, key)
    for i in range(2):
        assert np.array_equal(both[i], RR.philox4x32(ctr[i], key))


@pytest.mark.parametrize("n, R", [(1, 3), (5, 4), (7, 4), (257, 2)])
def test_counts_rows(n, R):
    c = RR.counts_ref(1234, R, n)
    assert c.shape == (R + 1, n) and (c[0] == 1).all() and (c.sum(1) == n).all() and (c >= 0).all()
    if n > 1:
        assert not np.array_equal(RR.counts_ref(1235, R, n)[1:], c[1:])


def test_counts_moments():
    """multinomial(n, 1 / n): every cell is Bin(n, p = 1 / n), mean 1, variance n p q = 1 - 1 / n.  Over R replicates the cell's sample
    mean has standard error sqrt(var / R) and its sample variance sqrt((mu4 - var^2) / R), mu4 = n p q (1 + 3 (n - 2) p q) the
    binomial's fourth central moment."""
    n, R = 7, 2000
    c = RR.counts_ref(0, R, n)[1:].astype(np.float64)
    p = 1.0 / n
    var = n * p * (1 - p)
    mu4 = var * (1 + 3 * (n - 2) * p * (1 - p))        # binomial: n p q (1 + 3 (n - 2) p q)
    assert (np.abs(c.mean(0) - 1.0) <= 5 * math.sqrt(var / R)).all(), c.mean(0)
    assert (np.abs(c.var(0, ddof=1) - var) <= 5 * math.sqrt((mu4 - var * var) / R)).all(), c.var(0, ddof=1)


def test_weighted_rank_matches_sklearn():
    from sklearn.metrics import average_precision_score, roc_auc_score
    rng = np.random.RandomState(3)
    n = 97
    score = (rng.randint(0, 6, n) / 4.0).astype(np.float32)       # tied scores
    y = rng.rand(n) < 0.4
    counts = RR.counts_ref(7, 12, n)
    for w in counts:
        r = RR.weighted_segment_ref(score, y, w)
        keep = w > 0
        assert r["P"] == int(w[y].sum()) and r["N"] == int(w[~y].sum())
        assert abs(r["auroc"] - roc_auc_score(y[keep], score[keep], sample_weight=w[keep])) <= 1e-12
        assert abs(r["ap"] - average_precision_score(y[keep], score[keep], sample_weight=w[keep])) <= 1e-12


def test_weighted_rank_is_the_expanded_rank():
    import ranking_ref
    rng = np.random.RandomState(4)
    n = 64
    score = (rng.randint(0, 4, n) / 4.0).astype(np.float32)
    y = rng.rand(n) < 0.5
    for w in RR.counts_ref(1, 5, n):
        r = RR.weighted_segment_ref(score, y, w)
        s, yy = RR.expand(w, score, y)
        e = ranking_ref.segment_ref(s, yy)
        assert (r["P"], r["N"], r["U2"]) == (e["P"], e["N"], e["U2"])
        assert abs(r["ap"] - e["ap"]) <= ranking_ref.ap_bound(n)


def test_weighted_rank_undefined():
    r = RR.weighted_segment_ref(np.array([0.1, 0.2, 0.3], np.float32), np.array([True, False, False]), np.array([0, 2, 1]))
    assert r["P"] == 0 and r["N"] == 3 and math.isnan(r["ap"]) and math.isnan(r["auroc"])


def test_delong_matches_fraction():
    rng = np.random.RandomState(5)
    n, M, C = 23, 2, 3
    labels = rng.randint(0, C, n)
    scores = (rng.randint(0, 8, (M, C, n)) / 8.0).astype(np.float32)       # ties, exactly representable
    d = RR.delong_ref(scores, labels)
    for c in range(C):
        pos = labels == c
        for a in range(M):
            for b in range(M):
                f = RR.delong_cov_fraction(scores[a, c][pos].tolist(), scores[a, c][~pos].tolist(), scores[b, c][pos].tolist(),
                                           scores[b, c][~pos].tolist())
                assert abs(d["cov"][c, a, b] - float(f)) <= 1e-12 * abs(float(f)), (c, a, b, d["cov"][c, a, b], float(f))
            assert d["var"][a, c] == d["cov"][c, a, a]
            P, N, U2 = d["pnu"][a, c]
            assert (P, N) == (pos.sum(), n - pos.sum())
            assert U2 == int(d["v2"][a, c][pos].sum()) == int(d["v2"][a, c][~pos].sum())       # both sum psi over every pair


def test_delong_undefined():
    d = RR.delong_ref(np.zeros((1, 2, 4), np.float32), np.array([0, 0, 0, 1]))
    assert np.isnan(d["var"]).all()


@pytest.mark.parametrize("b, c", [(0, 0), (0, 1), (3, 3), (1, 7), (12, 5), (40, 61), (0, 30), (300, 340)])
def test_mcnemar_matches_scipy(b, c):
    from scipy.stats import binomtest
    want = 1.0 if b + c == 0 else min(1.0, binomtest(min(b, c), b + c).pvalue)
    assert abs(RR.mcnemar_ref(b, c) - want) <= 1e-12


def test_interval_ref_is_nanquantile():
    rng = np.random.RandomState(6)
    reps = rng.rand(65, 3)
    reps[5:20, 1] = np.nan
    out = RR.interval_ref(reps, 0.025, 0.975)
    for k in range(3):
        assert out[k, 3] == np.nanquantile(reps[1:, k], 0.025, method="linear")
        assert out[k, 4] == np.nanquantile(reps[1:, k], 0.975, method="linear")
        assert abs(out[k, 2] - np.nanstd(reps[1:, k], ddof=1)) <= 1e-14
    assert out[1, 5] == 64 - 15


def test_header_declares_the_symbols():
    protos = parse_header()
    want = {
        "mi355_boot_counts_lds_max": [],
        "mi355_boot_counts": [ctypes.c_uint64, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p],
        "mi355_boot_rank_ws_ints": [ctypes.c_int, ctypes.c_longlong],
        "mi355_boot_rank": [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p, ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
        "mi355_boot_confusion": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
        "mi355_boot_sums": [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p],
        "mi355_boot_interval": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                ctypes.c_void_p],
        "mi355_delong_ws_ints": [ctypes.c_int, ctypes.c_int, ctypes.c_longlong],
        "mi355_delong": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                         ctypes.c_longlong] + [ctypes.c_void_p] * 5,
    }
    for name, types in want.items():
        assert name in protos, name
        ret, args = protos[name]
        assert ret is ctypes.c_int and [t for t, _ in args] == types, (name, args)
        if name not in ("mi355_boot_counts_lds_max", "mi355_boot_rank_ws_ints", "mi355_delong_ws_ints"):
            assert args[-1][1] == "s", name


def test_tester_flags_settings_and_csv_columns():
    import inspect
    from utils import tester
    ap = tester.build_parser()
    d = ap.parse_args([])
    assert (d.ci, d.ci_level, d.ci_seed) == (0, 0.95, 0) and (d.auc, d.surface, d.tta, d.sw_tile) == (False, False, None, 0)
    a = ap.parse_args("--auc --ci 2000 --ci-level 0.9 --ci-seed 7".split())
    assert (a.ci, a.ci_level, a.ci_seed, a.auc) == (2000, 0.9, 7, True)
    assert inspect.signature(tester.test_all_models).parameters["ci"].default is None
    assert inspect.signature(tester.evaluate_classification_model).parameters["ci"].default is None
    assert inspect.signature(tester.evaluate_segmentation_model_ci).parameters["ci"].default is None
    assert tester._check_ci(None) is None and tester._check_ci(0) is None
    c = tester._check_ci((64, 0.9, 5))
    assert (c.replicates, c.level, c.seed, c.kept) == (64, 0.9, 5, {}) and tester._check_ci(c) is c and tester._check_ci(8).replicates == 8
    assert c.footer() == "Bootstrap: 64 replicates, 90% percentile intervals, seed 5"
    for bad in ((0,), (8193,), (2.5,), (8, 0.0), (8, 1.0)):
        with pytest.raises(ValueError):
            tester.CI(*bad)
    row = tester._csv_row("m", {"accuracy": 90.0, "confusion_matrix": np.eye(2), "accuracy_ci": (88.0, 92.0), "accuracy_se": 1.0,
                                "ci_detail": {}, "auroc_ci_per_class": np.zeros((2, 2)), "ci_replicates": 8})
    assert row == {"Model": "m", "accuracy": 90.0, "accuracy_lo": 88.0, "accuracy_hi": 92.0, "accuracy_se": 1.0, "ci_replicates": 8}
    assert list(row) == ["Model", "accuracy", "accuracy_lo", "accuracy_hi", "accuracy_se", "ci_replicates"]
    assert tester.print_paired_tests({}, None) == {} and tester.print_paired_tests({}, tester.CI(4)) == {}


def test_public_functions_refuse_host_tensors():
    import torch
    from utils import resample
    x = torch.zeros(4)
    for call in (lambda: resample.boot_means(x, x), lambda: resample.interval(torch.zeros(3, 2, dtype=torch.float64)),
                 lambda: resample.delong(torch.zeros(2, 4), torch.zeros(4, dtype=torch.int32)),
                 lambda: resample.mcnemar(x, x), lambda: resample.bootstrap_counts(4, 2, device="cpu"),
                 lambda: resample.boot_confusion(x.int(), x.int(), 2, x.int()),
                 lambda: resample.boot_rank_metrics(x, x.int(), labels=x.int())):
        with pytest.raises(ValueError):
            call()
    assert resample._mcnemar_p(3, 3) == 1.0 and resample._mcnemar_p(0, 0) == 1.0
    assert abs(resample._mcnemar_p(1, 7) - RR.mcnemar_ref(1, 7)) == 0.0
