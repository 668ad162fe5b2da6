"""-m gpu: mi355_cls_calibration (csrc/ranking.hip) against the numpy restatement tests/ranking_ref.py.  The seeded inputs are redrawn
until the restatement's fp64 confidence is at least 1e-6 from every bin edge and the top two probabilities at least 1e-6 apart — both
asserted here, on the restatement — so that the prediction and the bin are decided far outside the device's error and bin_count /
bin_correct are compared as integers.  bin_conf, ece, brier and nll are held to the bounds derived in ranking_ref.py from the accuracy
of the device's double exp / log (1 ulp), each asserted to be at most 1e-9; scores_t to one fp32 ulp of the restated probabilities.
Outputs sit between guard bands; two runs are bit-identical."""
import numpy as np
import pytest
import torch

import ranking_ref as R
from mi355.lib import lib
from test_gpu_ranking import DEV, Guarded

pytestmark = pytest.mark.gpu


def op_calibration(x, labels, bins, is_prob, runs=2):
    N, C = x.shape
    need = lib.raw("mi355_cls_calibration_ws_ints")(N, C, bins)
    assert need > 0, lib.raw("mi355_last_error")()
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    yd = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(DEV)
    outs = []
    for _ in range(runs):
        g = {"ws": Guarded(need, torch.int32), "bin_count": Guarded(bins, torch.int64), "bin_correct": Guarded(bins, torch.int64),
             "bin_conf": Guarded(bins, torch.float64), "out": Guarded(3, torch.float64), "scores_t": Guarded(C * N, torch.float32)}
        lib.mi355_cls_calibration(xd, N, C, 1 if is_prob else 0, yd, bins, g["ws"].t, need, g["bin_count"].t, g["bin_correct"].t,
                                  g["bin_conf"].t, g["out"].t, g["scores_t"].t)
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values()), "a guard region next to ws or an output was written"
        outs.append({k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"})
    for o in outs[1:]:
        assert all(np.array_equal(o[k].view(np.uint8), outs[0][k].view(np.uint8)) for k in o), "second run differs"
    assert np.array_equal(xd.cpu().numpy().view(np.int32), np.ascontiguousarray(x, np.float32).view(np.int32))
    return outs[0]


def check(got, ref, N, C, bins, what):
    assert ref["edge_distance"] >= 1e-6 and ref["top2_gap"] >= 1e-6, what          # conditions on the reference's input
    assert np.array_equal(got["bin_count"], ref["bin_count"]) and np.array_equal(got["bin_correct"], ref["bin_correct"]), what
    assert int(got["bin_count"].sum()) == N
    L = ref["nll_max"] + 1.0
    bounds = {"bin_conf": max(R.bin_conf_bound(int(c), N, C) for c in ref["bin_count"]), "ece": R.ece_bound(N, C, bins),
              "brier": R.brier_bound(N, C), "nll": R.nll_bound(N, C, L)}
    assert max(bounds.values()) <= 1e-9, bounds
    err = {"bin_conf": np.abs(got["bin_conf"] - ref["bin_conf"]), "nll": abs(got["out"][0] - ref["nll"]),
           "brier": abs(got["out"][1] - ref["brier"]), "ece": abs(got["out"][2] - ref["ece"])}
    print(f"{what}: " + ", ".join(f"{k} {np.max(v):.2e} (bound {bounds[k]:.2e})" for k, v in err.items()))
    assert (err["bin_conf"] <= np.array([R.bin_conf_bound(int(c), N, C) for c in ref["bin_count"]])).all(), what
    assert err["nll"] <= bounds["nll"] and err["brier"] <= bounds["brier"] and err["ece"] <= bounds["ece"], (what, err, bounds)
    want = ref["scores_t"]
    assert (np.abs(got["scores_t"].reshape(C, N).astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64)).all(), what


@pytest.mark.parametrize("bins", [10, 15])
@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1025, 4097])
def test_calibration_of_logits_is_the_restatement(N, C, bins):
    x, labels, ref = R.calibration_inputs(N, C, bins, seed=100 * N + 10 * C + bins)
    check(op_calibration(x, labels, bins, False), ref, N, C, bins, (N, C, bins))


@pytest.mark.parametrize("N,C,bins", [(1, 3, 15), (65, 2, 10), (1025, 3, 15), (4097, 5, 10)])
def test_calibration_of_probabilities_is_the_restatement(N, C, bins):
    x, labels, ref = R.calibration_inputs(N, C, bins, seed=N + C, is_prob=True)
    got = op_calibration(x, labels, bins, True)
    check(got, ref, N, C, bins, (N, C, bins, "prob"))
    assert np.array_equal(got["scores_t"].reshape(C, N), x.T)          # the inputs, transposed


def test_large_logits_stay_finite():
    x = np.array([[80, -80, 0], [-80, 80, 80], [80, 80, 80], [-80, -80, -79], [0, 80, -80]], dtype=np.float32)
    labels = np.array([1, 0, 2, 2, 1], dtype=np.int32)
    ref = R.calibration_ref(x, labels, 15)
    got = op_calibration(x, labels, 15, False)
    assert np.isfinite(got["out"]).all() and np.isfinite(got["bin_conf"]).all() and np.isfinite(got["scores_t"]).all()
    assert np.array_equal(got["bin_count"], ref["bin_count"]) and np.array_equal(got["bin_correct"], ref["bin_correct"])
    assert abs(got["out"][0] - ref["nll"]) <= R.nll_bound(5, 3, 161.0) and abs(got["out"][1] - ref["brier"]) <= R.brier_bound(5, 3)
    assert ref["nll"] > 60 and ref["bin_count"].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 2]      # 1/3, 1/2 (first argmax), 0.576, 1, 1
    assert ref["pred"].tolist() == [0, 1, 0, 2, 1] and ref["bin_correct"].tolist() == [0] * 8 + [1] + [0] * 5 + [1]


def test_python_surface_matches_the_abi():
    from utils import ranking as UR
    N, C, bins = 257, 3, 15
    x, labels, ref = R.calibration_inputs(N, C, bins, seed=5)
    want = op_calibration(x, labels, bins, False, runs=1)
    r = UR.calibration(torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV).long())
    assert set(r) == {"ece", "brier", "nll", "bin_count", "bin_correct", "bin_confidence", "scores_t"} and all(v.is_cuda for v in r.values())
    assert r["ece"].shape == () and r["ece"].dtype == torch.float64 and r["scores_t"].shape == (C, N)
    assert [float(r["nll"]), float(r["brier"]), float(r["ece"])] == want["out"].tolist()
    assert np.array_equal(r["bin_count"].cpu().numpy(), want["bin_count"]) and np.array_equal(r["bin_correct"].cpu().numpy(), want["bin_correct"])
    assert np.array_equal(r["bin_confidence"].cpu().numpy(), want["bin_conf"])
    assert np.array_equal(r["scores_t"].cpu().numpy().reshape(-1), want["scores_t"])
    ten = UR.calibration(torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV), bins=10)
    assert ten["bin_count"].shape == (10,) and float(ten["nll"]) == float(r["nll"])
    # the transposed probabilities are what rank_metrics ranks, one class per segment
    m = UR.rank_metrics(r["scores_t"], labels=torch.from_numpy(labels).to(DEV))
    refs = R.rank_ref(r["scores_t"].cpu().numpy(), labels=labels)
    assert np.array_equal(m["u2"].cpu().numpy(), [q["U2"] for q in refs])
    with pytest.raises(ValueError, match="bins"):
        UR.calibration(torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV), bins=0)
    with pytest.raises(ValueError, match="labels"):
        UR.calibration(torch.from_numpy(x).to(DEV), torch.from_numpy(labels[:5]).to(DEV))
