"""CPU: the ranking metrics and the calibration figures below the GPU — the numpy restatement (tests/ranking_ref.py) against scikit-learn
(live where it is installed, and through the committed fixture tests/golden/ranking.npz of its outputs everywhere), hand-worked cases,
the Python surface and its errors, the tester's flags, the C ABI's argument checks (which run before anything touches the device) and
the new kernels' code-object notes."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import ranking_ref as R
from mi355 import lib as L

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "ranking.npz")


def _cases():
    """(name, fp32 scores, bool labels): every length from 1 to 9, then lengths to 65536, continuous / quantised / constant scores at
    prevalence 0.5 and 0.01 (both classes forced to occur where the length allows)"""
    for n in list(range(1, 10)) + [63, 64, 65, 221, 2049, 65536]:
        for kind in ("continuous", "quantised", "constant"):
            for prev in (0.5, 0.01):
                rng = np.random.RandomState(n * 7 + len(kind))
                s = rng.randn(n)
                s = {"continuous": s, "quantised": np.round(s * 4) / 4, "constant": np.full(n, 0.5)}[kind].astype(np.float32)
                y = rng.rand(n) < prev
                if n >= 2:
                    y[rng.randint(n)] = True
                    y[np.flatnonzero(~y)[0] if (~y).any() else 0] = False
                yield f"{n}_{kind}_{prev}", s, y


def test_restatement_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    worst = {"auroc": 0.0, "ap": 0.0}
    for name, s, y in _cases():
        r = R.segment_ref(s, y)
        assert r["P"] == int(y.sum()) and r["N"] == int((~y).sum()) and r["T"] == np.unique(s).size, name
        if r["P"] == 0 or r["N"] == 0:
            assert np.isnan(r["auroc"]) and (np.isnan(r["ap"]) == (r["P"] == 0)), name
            continue
        bound = R.ap_bound(s.size)
        d_auc = abs(r["auroc"] - metrics.roc_auc_score(y, s))
        d_ap = abs(r["ap"] - metrics.average_precision_score(y, s))
        worst["auroc"], worst["ap"] = max(worst["auroc"], d_auc / bound), max(worst["ap"], d_ap / bound)
        assert d_auc <= bound and d_ap <= bound, (name, d_auc, d_ap, bound)
        fpr, tpr, thr = metrics.roc_curve(y, s, drop_intermediate=False)
        mine = R.roc_ref(r)
        assert np.array_equal(thr, mine[2]) and thr.size == r["T"] + 1, name
        assert np.array_equal(np.rint(tpr * r["P"]).astype(np.int64), np.r_[0, r["tp"]]), name
        assert np.array_equal(np.rint(fpr * r["N"]).astype(np.int64), np.r_[0, r["fp"]]), name
        assert np.abs(tpr * r["P"] - np.rint(tpr * r["P"])).max() < 1e-6 and np.abs(fpr * r["N"] - np.rint(fpr * r["N"])).max() < 1e-6
        pp, rr, pthr = metrics.precision_recall_curve(y, s)
        mine = R.pr_ref(r)
        assert np.array_equal(pp, mine[0]) and np.array_equal(rr, mine[1]) and np.array_equal(pthr, mine[2]), name
    print(f"worst |restatement - sklearn| / bound: auroc {worst['auroc']:.3f}, ap {worst['ap']:.3f}")


def test_restatement_log_loss_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    for N, C in ((6, 3), (64, 2), (1025, 5)):
        x, labels, ref = R.calibration_inputs(N, C, 15, seed=N + C, is_prob=True)
        labels[:C] = np.arange(C)
        ref = R.calibration_ref(x, labels, 15, is_prob=True)
        assert ref["nll"] == metrics.log_loss(labels, x.astype(np.float64), labels=np.arange(C)), (N, C)


def test_restatement_reproduces_scikit_learns_recorded_outputs():
    z = np.load(FIXTURE)
    cases = [str(k) for k in z["cases"]]
    assert os.path.getsize(FIXTURE) <= 100 * 1024 and len(cases) >= 16
    kinds, lengths = set(), set()
    for name in cases:
        s, y = z["s__" + name], z["y__" + name]
        assert s.dtype == np.float32 and y.dtype == bool and y.any() and not y.all()
        lengths.add(s.size)
        kinds.add(name.split("_", 1)[1].rsplit("_", 1)[0])
        r = R.segment_ref(s, y)
        bound = R.ap_bound(s.size)
        assert abs(r["auroc"] - float(z["auroc__" + name])) <= bound and abs(r["ap"] - float(z["ap__" + name])) <= bound, name
        fpr, tpr, thr = R.roc_ref(r)
        assert np.array_equal(thr, z["roc_thr__" + name]), name
        assert np.array_equal(np.rint(z["roc_tpr__" + name] * r["P"]).astype(np.int64), np.r_[0, r["tp"]]), name
        assert np.array_equal(np.rint(z["roc_fpr__" + name] * r["N"]).astype(np.int64), np.r_[0, r["fp"]]), name
        pp, rr, pthr = R.pr_ref(r)
        assert np.array_equal(pp, z["pr_p__" + name]) and np.array_equal(rr, z["pr_r__" + name]), name
        assert np.array_equal(pthr, z["pr_thr__" + name]), name
    assert kinds == {"continuous", "quantised", "constant", "two_valued", "signed_zeros"} and lengths == {5, 33, 64, 130}
    sz = z["s__130_signed_zeros_0.1"]
    assert (np.signbit(sz) & (sz == 0)).any() and (~np.signbit(sz) & (sz == 0)).any()      # both zeros are in it: one tie group
    for name in (str(k) for k in z["calibration_cases"]):
        ref = R.calibration_ref(z["cx__" + name], z["cy__" + name], 15, is_prob=True)
        assert ref["nll"] == float(z["nll__" + name]), name


def test_hand_worked_case_with_ties():
    """scores 0.1 0.4 0.4 0.4 0.8 0.8 0.9 with labels 0 1 0 1 0 1 1, ascending groups {0.1} {0.4 x3} {0.8 x2} {0.9}:
    B = 0 2 3 4, A = 1 2 3 3.  U2 = 0 + 2 (2 + 1) + 1 (3 + 2) + 1 (3 + 3) = 17, AUROC = 17 / 24.
    descending points: (0.9: tp 1 fp 0) (0.8: tp 2 fp 1) (0.4: tp 4 fp 2) (0.1: tp 4 fp 3);
    ap = (1/4)(1/1) + (1/4)(2/3) + (2/4)(4/6) + 0 = 3/4."""
    s = np.array([0.4, 0.9, 0.1, 0.8, 0.4, 0.8, 0.4], dtype=np.float32)
    y = np.array([1, 1, 0, 0, 0, 1, 1], dtype=bool)
    r = R.segment_ref(s, y)
    assert (r["P"], r["N"], r["U2"], r["T"]) == (4, 3, 17, 4)
    assert r["auroc"] == 17 / 24 and abs(r["ap"] - 0.75) <= R.ap_bound(7)
    assert r["thresholds"].tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.4), np.float32(0.1)]
    assert r["tp"].tolist() == [1, 2, 4, 4] and r["fp"].tolist() == [0, 1, 2, 3]
    # both zeros are one group, whose threshold is +0.0
    z = R.segment_ref(np.array([0.0, -0.0, 1.0], dtype=np.float32), np.array([1, 0, 1], dtype=bool))
    assert (z["U2"], z["T"]) == (1 * 1 + 1 * 2, 2) and not np.signbit(z["thresholds"][1])
    # labels mode: one-vs-rest
    two = R.rank_ref(np.stack([s, -s]), labels=np.array([0, 0, 1, 1, 1, 0, 0]))
    assert (two[0]["P"], two[0]["U2"]) == (4, 17) and (two[1]["P"], two[1]["N"]) == (3, 4) and two[1]["U2"] == 17
    none = R.segment_ref(s, np.zeros(7, dtype=bool))
    assert (none["P"], none["U2"]) == (0, 0) and np.isnan(none["ap"]) and np.isnan(none["auroc"]) and none["tp"].tolist() == [0] * 4
    every = R.segment_ref(s, np.ones(7, dtype=bool))
    assert np.isnan(every["auroc"]) and abs(every["ap"] - 1.0) <= R.ap_bound(7)


def test_python_curve_helpers_follow_scikit_learns_conventions():
    from utils import ranking as UR
    s = np.array([0.4, 0.9, 0.1, 0.8, 0.4, 0.8, 0.4], dtype=np.float32)
    y = np.array([1, 1, 0, 0, 0, 1, 1], dtype=bool)
    r = R.segment_ref(s, y)
    fpr, tpr, thr = UR.roc_from_points(r["thresholds"], r["tp"], r["fp"])
    assert thr[0] == np.inf and thr.dtype == np.float32 and fpr.tolist() == [0, 0, 1 / 3, 2 / 3, 1] and tpr.tolist() == [0, 0.25, 0.5, 1, 1]
    pp, rr, pthr = UR.pr_from_points(r["thresholds"], r["tp"], r["fp"])
    assert pp.tolist() == [4 / 7, 4 / 6, 2 / 3, 1.0, 1.0] and rr.tolist() == [1, 1, 0.5, 0.25, 0] and pthr.tolist() == r["thresholds"][::-1].tolist()
    for got, want in zip((fpr, tpr, thr), R.roc_ref(r)):
        assert np.array_equal(got, want)
    for got, want in zip((pp, rr, pthr), R.pr_ref(r)):
        assert np.array_equal(got, want)
    none = R.segment_ref(s, np.zeros(7, dtype=bool))
    fpr, tpr, _ = UR.roc_from_points(none["thresholds"], none["tp"], none["fp"])
    assert np.isnan(tpr).all() and fpr[-1] == 1
    assert UR.pr_from_points(none["thresholds"], none["tp"], none["fp"])[1].tolist() == [1, 1, 1, 1, 0]


def test_calibration_by_hand_on_six_samples():
    """probabilities (is_prob), 2 bins (0, 0.5], (0.5, 1]:
      sample  p                  y  conf  pred  bin  correct
        0     0.5  0.25 0.25     0  0.5    0     0     1        (0.5 is the upper edge of bin 0; the first of the maxima)
        1     0.25 0.5  0.25     2  0.5    1     0     0
        2     0.125 0.125 0.75   2  0.75   2     1     1
        3     0.75 0.125 0.125   1  0.75   0     1     0
        4     0    1    0        1  1      1     1     1
        5     0.25 0.25 0.5      2  0.5    2     0     1
    bin 0: count 3, correct 2, conf 1.5; bin 1: count 3, correct 2, conf 2.5; ECE = (0.5 + 0.5) / 6."""
    p = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.125, 0.125, 0.75], [0.75, 0.125, 0.125], [0, 1, 0], [0.25, 0.25, 0.5]], dtype=np.float32)
    y = np.array([0, 2, 2, 1, 1, 2])
    r = R.calibration_ref(p, y, bins=2, is_prob=True)
    assert r["bin_count"].tolist() == [3, 3] and r["bin_correct"].tolist() == [2, 2] and r["bin_conf"].tolist() == [1.5, 2.5]
    assert r["pred"].tolist() == [0, 1, 2, 0, 1, 2] and r["ece"] == 1.0 / 6
    brier = [0.25 + 2 / 16, 1 / 16 + 0.25 + 9 / 16, 2 / 64 + 1 / 16, 9 / 16 + 49 / 64 + 1 / 64, 0.0, 2 / 16 + 0.25]
    assert abs(r["brier"] - sum(brier) / 6) < 1e-15
    assert abs(r["nll"] - (-np.log([0.5, 0.25, 0.75, 0.125, 1.0, 0.5]).sum() / 6)) < 1e-15
    assert r["scores_t"].shape == (3, 6) and np.array_equal(r["scores_t"], p.T)
    # logits: the same figures through the softmax; +-80 stays finite
    z = np.log(np.maximum(p, 1e-30)).astype(np.float32)
    lr = R.calibration_ref(z[[0, 1, 2, 3, 5]], y[[0, 1, 2, 3, 5]], bins=2)
    assert abs(lr["brier"] - sum(brier[:4] + brier[5:]) / 5) < 1e-6 and lr["bin_count"].sum() == 5
    big = R.calibration_ref(np.array([[80, -80, 0], [-80, 80, 80]], dtype=np.float32), np.array([1, 0]), bins=15)
    assert np.isfinite([big["nll"], big["brier"], big["ece"]]).all() and abs(big["nll"] - (160 + 160 + np.log(2)) / 2) < 1e-12
    # every bound is far below 1e-9 for the shapes of the GPU tests
    for N in (1, 63, 64, 65, 257, 1025, 4097):
        for C in (2, 3, 5):
            for bins in (10, 15):
                assert max(R.bin_conf_bound(N, N, C), R.ece_bound(N, C, bins), R.brier_bound(N, C), R.nll_bound(N, C, 200.0)) <= 1e-9


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_signatures_defaults_and_errors():
    import torch
    from mi355 import nn as mnn
    from utils import ranking as UR
    from utils import tester
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    for f in (UR.rank_metrics, UR.binary_curve, UR.roc_curve, UR.precision_recall_curve):
        assert sig(f) == [("scores", E), ("target", None), ("labels", None), ("threshold", 0.5)], f.__name__
    assert sig(UR.calibration) == [("logits_or_probs", E), ("labels", E), ("bins", 15), ("is_prob", False)]
    assert sig(tester.test_classification_model)[4:] == [("tta", None), ("auc", False), ("calibration_bins", 15)]
    # test_segmentation_model keeps the argument list tests/test_surface_cpu.py pins; the loop with ``auc`` is evaluate_segmentation_model
    assert sig(tester.test_segmentation_model)[4:] == [("surface", False)]
    assert sig(tester.evaluate_segmentation_model) == sig(tester.test_segmentation_model) + [("auc", False)]
    assert sig(tester.test_all_models)[-3:] == [("auc", False), ("calibration_bins", 15), ("surface", False)]
    assert callable(mnn._rank_metrics) and callable(mnn._cls_calibration)
    s, t, y = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(8, dtype=torch.int32)
    for f in (UR.rank_metrics, UR.binary_curve, UR.roc_curve, UR.precision_recall_curve):
        with pytest.raises(ValueError, match="device tensor"):
            f(s, target=t)
        with pytest.raises(ValueError, match="device tensor"):
            f(s, labels=y)
        with pytest.raises(ValueError, match="exactly one of target and labels"):
            f(s, target=t, labels=y)
        with pytest.raises(ValueError, match="exactly one of target and labels"):
            f(s)
    with pytest.raises(ValueError, match="device tensor"):
        UR.calibration(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))


def test_tester_flags():
    from utils import tester
    ap = tester.build_parser()
    d = ap.parse_args([])
    assert (d.auc, d.calibration_bins) == (False, 15)
    assert (d.surface, d.tta, d.tta_merge, d.clahe_clip, d.clahe_grid) == (False, None, "prob", 0.0, 8)      # the others are unchanged
    a = ap.parse_args(["--auc", "--calibration-bins", "10"])
    assert (a.auc, a.calibration_bins) == (True, 10)
    with pytest.raises(SystemExit):
        ap.parse_args(["--calibration-bins", "many"])


def test_summary_and_csv_only_change_with_the_new_keys(tmp_path, capsys):
    from utils import tester
    cls = {"accuracy": 90.0, "precision": 91.0, "recall": 89.0, "f1": 90.0, "precision_per_class": np.ones(3), "recall_per_class": np.ones(3),
           "f1_per_class": np.ones(3), "confusion_matrix": np.eye(3, dtype=np.int64)}
    seg = {"iou": 70.0, "dice": 80.0, "pixel_accuracy": 95.0, "precision": 81.0, "recall": 79.0, "f1": 80.0}
    tester.print_summary({"ResNet18": dict(cls), "AttentionUNet": dict(seg)})
    plain = capsys.readouterr().out
    assert "RANKING" not in plain
    cls.update(auroc=0.9, average_precision=0.8, auc_classes=3, auroc_per_class=np.full(3, 0.9), ap_per_class=np.full(3, 0.8), ece=0.05,
               brier=0.2, nll=0.4)
    seg.update(pixel_auroc=0.97, pixel_ap=0.66, auc_samples=5)
    results = {"ResNet18": cls, "AttentionUNet": seg}
    tester.print_summary(results)
    text = capsys.readouterr().out
    assert "CLASSIFICATION MODELS, RANKING AND CALIBRATION" in text and "SEGMENTATION MODELS, PIXEL RANKING" in text
    assert "0.9000" in text and "0.9700" in text and "0.6600" in text
    rest = iter(text.splitlines())
    assert all(any(l == r for r in rest) for l in plain.splitlines())      # the old lines are all still there, in their order
    assert len([l for l in text.splitlines() if l not in plain.splitlines()]) == 6      # two tables: title, header, row
    pytest.importorskip("pandas")
    tester.save_results_to_csv(results, str(tmp_path / "c.csv"), str(tmp_path / "s.csv"))
    head = open(tmp_path / "c.csv").readline().strip().split(",")
    assert head == ["Model", "accuracy", "precision", "recall", "f1", "auroc", "average_precision", "auc_classes", "ece", "brier", "nll"]
    assert open(tmp_path / "s.csv").readline().strip().split(",")[-3:] == ["pixel_auroc", "pixel_ap", "auc_samples"]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NAMES = {"mi355_rank_ws_ints": ["S", "len"],
         "mi355_rank_metrics": ["scores", "target", "labels", "S", "len", "thr", "ws", "ws_ints", "counts", "ap", "thresholds", "tp", "fp",
                                "npoints", "s"],
         "mi355_cls_calibration_ws_ints": ["N", "C", "bins"],
         "mi355_cls_calibration": ["x", "N", "C", "is_prob", "labels", "bins", "ws", "ws_ints", "bin_count", "bin_correct", "bin_conf", "out",
                                   "scores_t", "s"]}


def test_abi_declares_exports_and_replays_the_new_entry_points():
    protos = L.parse_header()
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name, args in NAMES.items():
        assert name in protos and protos[name][0] is ctypes.c_int, name
        assert [n for _, n in protos[name][1]] == args, name
        assert hasattr(dll, name), name
        assert arity(name.encode()) == len(args), name
    sort_ws, rank_ws = L.lib.raw("mi355_segsort_ws_ints"), L.lib.raw("mi355_rank_ws_ints")
    for S, n in ((1, 1), (3, 221), (32, 65536), (1, 1 << 21), (65535, 4), (1, 1 << 26), (65535, 1024)):
        assert sort_ws(S, n) + 2 * S * n <= rank_ws(S, n) <= sort_ws(S, n) + 3 * S * n + 80 * S, (S, n)
    cal_ws = L.lib.raw("mi355_cls_calibration_ws_ints")
    assert 0 < cal_ws(1, 3, 15) <= cal_ws(4097, 3, 15) <= 17 * (4 * 15 + 4)


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    rank_ws, cal_ws = lib.raw("mi355_rank_ws_ints"), lib.raw("mi355_cls_calibration_ws_ints")
    for bad in ((0, 16), (-1, 16), (65536, 16), (2, 0), (2, -4), (2, (1 << 25) + 1), (1, (1 << 26) + 1), (65535, 1025)):
        assert rank_ws(*bad) == -1 and b"rank_ws_ints" in err() and b"2^26" in err(), (bad, err())
    for bad in ((0, 3, 15), (4, 0, 15), (4, 4097, 15), (1 << 25, 3, 15), (4, 3, 0), (4, 3, 1025)):
        assert cal_ws(*bad) == -1 and b"cls_calibration_ws_ints" in err(), (bad, err())
    buf = (ctypes.c_double * 4096)()                    # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)

    need = rank_ws(2, 64)
    assert need > 0
    run = lib.raw("mi355_rank_metrics")
    ok = dict(scores=p, target=p, labels=None, S=2, len=64, thr=0.5, ws=p, ws_ints=need, counts=p, ap=p, thresholds=None, tp=None, fp=None,
              npoints=None)

    def call(**kw):
        a = dict(ok, **kw)
        return run(a["scores"], a["target"], a["labels"], a["S"], a["len"], a["thr"], a["ws"], a["ws_ints"], a["counts"], a["ap"],
                   a["thresholds"], a["tp"], a["fp"], a["npoints"], None)

    for bad, word in (({"scores": None}, b"null pointer (scores)"), ({"labels": p}, b"exactly one of target and labels"),
                      ({"target": None}, b"exactly one of target and labels"), ({"ws": None}, b"null pointer (ws)"),
                      ({"counts": None}, b"null pointer (counts)"), ({"ap": None}, b"null pointer (ap)"),
                      ({"thresholds": p}, b"given together"), ({"tp": p, "fp": p, "npoints": p}, b"given together"),
                      ({"S": 0}, b"S"), ({"S": 65536}, b"65535"), ({"len": 0}, b"len"), ({"len": -3}, b"len"),
                      ({"len": (1 << 25) + 1}, b"2^26"), ({"ws_ints": need - 1}, b"too short"), ({"ws_ints": 0}, b"too short"),
                      ({"target": None, "labels": p, "ws_ints": need - 1}, b"too short")):
        assert call(**bad) == -1, bad
        assert word in err() and b"rank_metrics" in err(), (bad, err())

    need = cal_ws(64, 3, 15)
    assert need > 0
    run_c = lib.raw("mi355_cls_calibration")
    okc = dict(x=p, N=64, C=3, is_prob=0, labels=p, bins=15, ws=p, ws_ints=need, bin_count=p, bin_correct=p, bin_conf=p, out=p, scores_t=p)

    def call_c(**kw):
        a = dict(okc, **kw)
        return run_c(a["x"], a["N"], a["C"], a["is_prob"], a["labels"], a["bins"], a["ws"], a["ws_ints"], a["bin_count"], a["bin_correct"],
                     a["bin_conf"], a["out"], a["scores_t"], None)

    for bad, word in ([({k: None}, f"null pointer ({k})".encode()) for k in ("x", "labels", "ws", "bin_count", "bin_correct", "bin_conf", "out",
                                                                           "scores_t")]
                      + [({"N": 0}, b"N"), ({"C": 0}, b"C"), ({"C": 4097}, b"4096"), ({"N": 1 << 25}, b"2^26"), ({"bins": 0}, b"bins"),
                         ({"bins": 1025}, b"1024"), ({"ws_ints": need - 1}, b"too short"), ({"ws_ints": 0}, b"too short")]):
        assert call_c(**bad) == -1, bad
        assert word in err() and b"cls_calibration" in err(), (bad, err())


def test_new_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    """Read as tests/test_lovasz_cpu.py reads its own: no private segment, no spilled register, <= 128 VGPRs, <= 40 KB of LDS."""
    import re
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed here")
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built"
    so = shutil.copy(L.SO_PATH, tmp_path)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp_path)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp_path, f)], check=True, capture_output=True,
                               text=True).stdout
        if "rank_" not in notes and "calib_" not in notes:
            continue
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if re.search(r"rank_(gather|carry|tile|finalize)_kernel|calib_(rows|finalize)_kernel", name):
                found[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                               for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                         "group_segment_fixed_size")}
    # gather (target / labels), carry, tile (with / without the curve), finalize; calibration: rows, finalize
    assert sum("rank_gather" in k for k in found) == 2 and sum("rank_tile" in k for k in found) == 2, sorted(found)
    assert sum("rank_carry" in k for k in found) == 1 and sum("rank_finalize" in k for k in found) == 1, sorted(found)
    assert sum("calib_rows" in k for k in found) == 1 and sum("calib_finalize" in k for k in found) == 1 and len(found) == 8, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] <= 40 * 1024, (name, k)
