"""The yardstick of the calibration tests on the CPU: tests/calibrate_ref.py against scipy's root finder, a brute-force sweep and the
tester's own Dice; the ABI's declarations; the new flags, the sidecar and the refusal of host tensors.  No GPU."""
import inspect
import json

import numpy as np
import pytest
import torch

import calibrate_ref as CR


@pytest.mark.parametrize("N,C,T0", [(64, 3, 0.5), (65, 33, 1.0), (257, 2, 3.0), (63, 1000, 3.0), (1, 4, None)])
def test_restated_beta_is_the_root_of_the_gradient(N, C, T0):
    from scipy.optimize import brentq
    if T0 is None:
        x, labels = np.array([[2.0, 0.5, -1.0, -1.5]], dtype=np.float32), np.array([1])
    else:
        x, labels = CR.temperature_inputs(N, C, T0, seed=100 * N + C)
    r = CR.temperature_ref(x, labels)
    assert r["status"] == 0 and CR.BETA_LO < r["beta"] < CR.BETA_HI and r["g2"] >= 1e-3 and r["evals"] <= 16
    ok, below, above = CR.sign_change(x, labels, r["beta"])
    assert ok, (below, above)
    root = brentq(lambda b: CR.nll_terms(x, labels, b)["g1"], CR.BETA_LO, CR.BETA_HI, xtol=1e-14, rtol=1e-14)
    assert abs(r["beta"] - root) <= 1e-6 * root
    # a minimum of the NLL, and nll_before is the NLL at T = 1
    assert r["nll"] <= min(CR.nll_terms(x, labels, r["beta"] * f)["nll"] for f in (0.99, 1.01)) and r["nll"] <= r["nll_before"]
    assert r["nll_before"] == CR.nll_terms(x, labels, 1.0)["nll"] and r["T"] == 1.0 / r["beta"]
    assert CR.temp_nll_bound(N, C, 20.0, 64.0) < 1e-9


def test_restated_nll_is_scikit_learns():
    from sklearn.metrics import log_loss
    x, labels = CR.temperature_inputs(257, 5, 1.0, seed=3)
    for beta in (0.3, 1.0, 2.5):
        p = np.exp(beta * x.astype(np.float64))
        p /= p.sum(1, keepdims=True)
        assert abs(CR.nll_terms(x, labels, beta)["nll"] - log_loss(labels, p, labels=np.arange(5))) <= 1e-12


def test_restated_clamps_and_flat():
    rng = np.random.RandomState(0)
    x = rng.randn(40, 4).astype(np.float32)
    top, low = x.argmax(1), x.argmin(1)
    sep = x.copy()
    sep[np.arange(40), top] += 50
    r = CR.temperature_ref(sep, top)
    assert (r["status"], r["beta"], r["evals"]) == (2, 64.0, 2)
    inv = x.copy()
    inv[np.arange(40), low] -= 50
    r = CR.temperature_ref(inv, low)
    assert (r["status"], r["beta"], r["evals"]) == (1, 2.0 ** -6, 2)
    r = CR.temperature_ref(np.repeat(x[:, :1], 4, axis=1), top)
    assert (r["status"], r["beta"], r["evals"]) == (3, 1.0, 1) and abs(r["nll"] - np.log(4)) < 1e-15


def _brute(scores, target, thr, tthr=0.5):
    B, n = scores.shape
    tp, fp = np.zeros((B, len(thr)), np.int32), np.zeros((B, len(thr)), np.int32)
    for b in range(B):
        for k in range(len(thr)):
            for i in range(n):
                if scores[b, i] > thr[k]:
                    if target[b, i] > tthr:
                        tp[b, k] += 1
                    else:
                        fp[b, k] += 1
    return tp, fp, (target > tthr).sum(1).astype(np.int32)


def test_sweep_restatement_is_the_triple_loop():
    rng = np.random.RandomState(1)
    thr = np.array([-0.25, 0.0, 0.125, 0.5, 0.75], dtype=np.float32)
    scores = rng.rand(2, 90).astype(np.float32)
    scores[:, :30] = thr[rng.randint(0, 5, (2, 30))]          # ties with the candidates: the compare is strict
    scores[:, 30:34] = np.array([0.0, -0.0, np.nan, 2.0], dtype=np.float32)
    target = (rng.rand(2, 90) < 0.5).astype(np.float32)
    for a, b in zip(CR.sweep_ref(scores, target, thr), _brute(scores, target, thr)):
        assert np.array_equal(a, b)
    assert CR.bins_ref(np.array([np.nan, -0.0, 0.0, 1e-45], np.float32), thr).tolist() == [0, 1, 1, 2]
    z = (rng.randn(2, 90) * 3).astype(np.float32)
    assert np.array_equal(CR.sweep_ref(z, target, thr[2:], is_logit=True)[0], _brute(CR.sigmoid64(z), target, thr[2:].astype(np.float64))[0])


def test_dice_at_candidate_127_is_the_testers_at_one_half():
    from utils import tester
    rng = np.random.RandomState(2)
    thr = CR.DEFAULT_THRESHOLDS
    assert thr.dtype == np.float32 and len(thr) == 255 and thr[127] == 0.5 and (np.diff(thr) > 0).all()
    scores = rng.rand(3, 500).astype(np.float32)
    target = (rng.rand(3, 500) < 0.3).astype(np.float32)
    target[2] = 0
    scores[2] = 0.25                                # an empty image without a prediction: Dice = IoU = 1
    tp, fp, pos = CR.sweep_ref(scores, target, thr)
    dice, iou = CR.dice_iou(tp, fp, pos)
    for b in range(3):
        p, t = scores[b] > 0.5, target[b] > 0.5
        m = tester._metrics_from_counts((float((p & t).sum()), float(p.sum()), float(t.sum()), float((p == t).sum())), 500)
        assert dice[b, 127] * 100 == m["dice"] and iou[b, 127] * 100 == m["iou"]
    assert dice[2, 127] == 1.0 and (dice <= 1.0).all() and (iou <= 1.0).all()
    acc, n = CR.fold_ref([(tp[:2], fp[:2], pos[:2]), (tp[2:], fp[2:], pos[2:])], 255)
    assert n == 3 and np.abs(acc[0] - dice.sum(0)).max() <= CR.fold_bound(3)
    k = CR.pick_ref(acc, n, 127)
    assert k[0] == int(np.argmax(acc[0])) and k[3] == acc[0][127] / 3


def test_header_declares_the_calibration_abi():
    from mi355.lib import parse_header
    protos = parse_header()
    want = {"mi355_temperature_fit_ws_ints": 2, "mi355_temperature_fit": 8, "mi355_temperature_eval": 9, "mi355_logits_scale": 6,
            "mi355_thr_sweep_chunk": 0, "mi355_thr_sweep_ws_ints": 3, "mi355_thr_sweep": 14, "mi355_thr_sweep_fold": 8, "mi355_thr_sweep_pick": 7}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs, name
    assert [a for _, a in protos["mi355_temperature_fit"][1]] == ["x", "N", "C", "labels", "ws", "ws_ints", "state", "s"]


def test_flags_parse_and_default_to_off():
    from utils import tester, trainer
    for build, flag, key, on in ((trainer.build_parser, ["--calibrate"], "calibrate", True),
                                 (tester.build_parser, ["--calibration", "weights"], "calibration", "weights")):
        off, with_flag = vars(build().parse_args([])), vars(build().parse_args(flag))
        assert off[key] in (False, None) and with_flag[key] == on
        assert {k: v for k, v in off.items() if k != key} == {k: v for k, v in with_flag.items() if k != key}
    for fn in (tester.evaluate_classification_model, tester.evaluate_segmentation_model_ci, tester.test_all_models):
        assert inspect.signature(fn).parameters["calibration"].default is None


def test_sidecar_round_trips(tmp_path):
    from utils.calibrate import Calibration, find_sidecar
    cal = Calibration("classification", temperature=1.7320508075688772, before=0.9876543210123457, after=0.5, status=0, samples=640)
    path = cal.save(Calibration.path(tmp_path, "ResNet18"))
    assert path.endswith("ResNet18_calibration.json") and Calibration.load(path) == cal
    assert set(json.load(open(path))) == {"kind", "temperature", "threshold", "before", "after", "status", "samples"}
    seg = Calibration("segmentation", threshold=float(np.float32(100 / 256)), before=0.61, after=0.64, samples=12)
    (tmp_path / "segmentation_models").mkdir()
    seg.save(Calibration.path(tmp_path / "segmentation_models", "AttentionUNet"))
    assert find_sidecar(str(tmp_path), "AttentionUNet", "segmentation_models") == seg
    with pytest.raises(FileNotFoundError, match="R2Unet_calibration.json"):
        find_sidecar(str(tmp_path), "R2Unet", "segmentation_models")
    assert "T = 1.7321" in cal.describe() and "t* = 0.3906" in seg.describe()


def test_public_functions_refuse_host_tensors():
    from utils import calibrate as UC
    x, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.long)
    for call in (lambda: UC.fit_temperature(x, y), lambda: UC.apply_temperature(x, 2.0), lambda: UC.nll_at(x, y, 2.0),
                 lambda: UC.dice_sweep(torch.zeros(2, 8), torch.zeros(2, 8))):
        with pytest.raises(ValueError, match="device tensors"):
            call()
    assert np.array_equal(UC.default_thresholds(), CR.DEFAULT_THRESHOLDS) and UC.default_thresholds()[127] == 0.5
    with pytest.raises(ValueError, match="ascending"):
        UC._check_thresholds([0.2, 0.1])
