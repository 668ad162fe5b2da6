"""CPU: the weight-averaging ABI (csrc/weight_avg.hip) is declared and exported, the numpy restatement tests/averaging_ref.py is pinned
to hand-computed values and to fp64 means, and the trainer / tester flags exist, are off by default and exclude each other."""
import ctypes
import os

import numpy as np
import pytest

import averaging_ref as R
from mi355 import lib as L

f32 = np.float32
PROTOS = {
    "mi355_avg_update": ["avg", "p", "n", "mode", "decay", "warmup", "count", "found_inf", "s"],
    "mi355_avg_update_table": ["table", "rows", "mode", "decay", "warmup", "count", "found_inf", "s"],
    "mi355_swap_table": ["table", "rows", "s"],
    "mi355_bn_debias_table": ["table", "rows", "momentum", "s"],
}


def test_header_declares_the_prototypes_with_the_documented_arguments():
    protos = L.parse_header()
    for name, args in PROTOS.items():
        assert name in protos, name
        assert [a for _, a in protos[name][1]] == args, name
        assert protos[name][0] is ctypes.c_int
    assert protos["mi355_avg_update_grid_elems"][1] == []
    # const follows who is written: the table and the live parameters are read, the average is written
    import plan_access as pa
    k = dict(pa.parse_slots()["mi355_avg_update"])
    assert (k["avg"], k["p"], k["count"], k["found_inf"]) == ("out", "in", "in", "in")
    assert all(dict(pa.parse_slots()[n])["table"] == "in" for n in list(PROTOS)[1:])


@pytest.mark.skipif(not os.path.exists(L.SO_PATH), reason="libmi355conv.so not built (run __graft_entry__.build())")
def test_library_exports_them_and_validates_arguments_without_a_gpu():
    dll = ctypes.CDLL(L.SO_PATH)
    for name in list(PROTOS) + ["mi355_avg_update_grid_elems"]:
        assert hasattr(dll, name), name
    lib = L.lib
    assert lib.raw("mi355_plan_arity")(b"mi355_avg_update") == 9 and lib.raw("mi355_plan_arity")(b"mi355_swap_table") == 3
    g = lib.raw("mi355_avg_update_grid_elems")()
    assert g > 0 and g % 1024 == 0
    err = lib.raw("mi355_last_error")
    # n == 0 and rows == 0 are no-ops that return OK before anything is dereferenced or launched
    assert lib.raw("mi355_avg_update")(None, None, 0, 0, 0.9, 0.0, None, None, None) == 0
    assert lib.raw("mi355_avg_update_table")(None, 0, 1, 0.0, 0.0, None, None, None) == 0
    assert lib.raw("mi355_swap_table")(None, 0, None) == 0
    assert lib.raw("mi355_bn_debias_table")(None, 0, 0.1, None) == 0
    assert lib.raw("mi355_avg_update")(None, None, 4, 0, 0.9, 0.0, None, None, None) == -1 and b"null" in err()
    assert lib.raw("mi355_avg_update")(None, None, 4, 2, 0.9, 0.0, None, None, None) == -1 and b"mode" in err()
    assert lib.raw("mi355_avg_update")(None, None, 4, 0, 1.5, 0.0, None, None, None) == -1 and b"decay" in err()
    assert lib.raw("mi355_swap_table")(None, 3, None) == -1 and b"null" in err()
    assert lib.raw("mi355_swap_table")(None, 70000, None) == -1 and b"rows" in err()
    assert lib.raw("mi355_bn_debias_table")(None, 3, 0.0, None) == -1 and b"momentum" in err()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_ema_schedule_is_timms_formula():
    """timm.utils.ModelEmaV3.get_decay with use_warmup: min(decay, (1 + t) / (warmup + t)); values worked out by hand"""
    assert R.ema_decay(1, 0.999, 10) == 2.0 / 11.0
    assert R.ema_decay(5, 0.999, 10) == 6.0 / 15.0
    assert R.ema_decay(10, 0.999, 10) == 11.0 / 20.0
    assert R.ema_decay(8990, 0.999, 10) == 8991.0 / 9000.0            # 0.999 exactly as a ratio: still below float32(0.999)
    assert R.ema_decay(10 ** 4, 0.999, 10) == float(f32(0.999))          # decay-limited: 10001 / 10010 = 0.99910...
    assert R.ema_decay(1, 0.999, 0) == float(f32(0.999)) and R.ema_decay(1, 0.5, 10) == 2.0 / 11.0 and R.ema_decay(3, 0.25, 10) == 0.25
    # the coefficient is rounded to float32 once, from the double 1 - d
    assert R.coefficient(R.EMA, 5, 0.999, 10) == ("update", f32(1.0 - 6.0 / 15.0))
    assert R.coefficient(R.EMA, 10 ** 4, 0.999, 10) == ("update", f32(1.0 - float(f32(0.999))))
    assert R.coefficient(R.EMA, 0) == ("skip", f32(0)) and R.coefficient(R.EQUAL, 1)[0] == "copy"
    assert R.coefficient(R.EQUAL, 7) == ("update", f32(1.0 / 7.0))


def test_update_rounds_every_operation_and_keeps_equal_values():
    avg, p = np.array([1.0, -0.0, 0.0, 1e-42, 3.0], f32), np.array([2.0, -0.0, -0.0, 1e-42, 3.0], f32)
    a = R.coefficient(R.EMA, 5, 0.999, 10)[1]
    out = R.update(avg, p, R.EMA, 5, 0.999, 10)
    assert out[0] == f32(f32(1.0) + f32(a * f32(1.0)))
    assert out.view(np.int32)[1:].tolist() == avg.view(np.int32)[1:].tolist()           # -0, +0 against -0, a denormal: avg's bits
    assert np.array_equal(R.update(avg, p, R.EMA, 5, found_inf=1.0).view(np.int32), avg.view(np.int32))
    assert np.array_equal(R.update(avg, p, R.EQUAL, 1).view(np.int32), p.view(np.int32))   # the first equal-weight update copies
    assert R.tick(3, 0.0) == 4 and R.tick(3, 1.0) == 3


@pytest.mark.parametrize("T", [2, 7, 50])
def test_equal_average_is_the_fp64_mean_within_T_roundings(T):
    rng = np.random.default_rng(T)
    xs = rng.standard_normal((T, 257)).astype(f32)
    avg = np.zeros(257, f32)
    for t in range(1, T + 1):
        avg = R.update(avg, xs[t - 1], R.EQUAL, t)
    mean = xs.astype(np.float64).mean(0)
    # update t rounds diff (|diff| <= 2 X, then scaled by 1 / t), the step (<= 2 X / t) and the sum (<= X), X = max |x|: at most
    # u X (4 / t + 1) of new error, u = 2^-24, which later updates damp to t / T of it: sum_t (t / T)(4 / t + 1) u X
    # = (4 + (T + 1) / 2) u X <= (T + 4) u X
    assert np.all(np.abs(avg - mean) <= (T + 4) * 2.0 ** -24 * np.abs(xs).max())


@pytest.mark.parametrize("k", [1, 2, 50, 4000])
def test_debias_of_a_zero_initialised_recurrence_returns_the_constant_input(k):
    b = np.array([0.37, -12.5, 1e-3], np.float64)
    r = np.array([R.bn_recurrence([v] * k, 0.1) for v in b], f32)
    got, exact = R.bn_debias(r, k, 0.1)
    assert np.all(np.abs(exact - b) <= (min(k, 20) + 1) * 2.0 ** -24 * np.abs(b) / R.bn_correction(k, 0.1))
    assert np.all(np.abs(got - b) <= (min(k, 20) + 2) * 2.0 ** -24 * np.abs(b) / R.bn_correction(k, 0.1))
    assert np.array_equal(R.bn_debias(r, 0, 0.1)[0].view(np.int32), r.view(np.int32))        # k = 0: untouched
    assert abs(R.bn_weighted_mean([[1.0], [1.0], [1.0]], 0.1)[0] - 1.0) < 1e-15
    w = R.bn_weighted_mean(np.eye(3), 0.1)
    m = float(f32(0.1))
    assert np.allclose(w, np.array([m * (1 - m) ** 2, m * (1 - m), m]) / (1 - (1 - m) ** 3), rtol=1e-15)


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
def test_trainer_flags_are_off_by_default_and_exclude_each_other():
    from utils import trainer
    ap = trainer.build_parser()
    args = ap.parse_args([])
    assert args.ema_decay is None and args.swa_start is None and args.ema_warmup == 10.0
    assert trainer.averaging_arg(args) is None
    assert trainer.averaging_arg(ap.parse_args(["--ema-decay", "0.99"])) == {"mode": "ema", "decay": 0.99, "warmup": 10.0}
    assert trainer.averaging_arg(ap.parse_args(["--ema-decay", "0.99", "--ema-warmup", "0"]))["warmup"] == 0.0
    assert trainer.averaging_arg(ap.parse_args(["--swa-start", "3", "--epochs", "4"])) == {"mode": "swa", "swa_start": 3}
    with pytest.raises(ValueError, match="mutually exclusive"):
        trainer.averaging_arg(ap.parse_args(["--ema-decay", "0.99", "--swa-start", "3"]))
    with pytest.raises(ValueError, match="--ema-decay"):
        trainer.averaging_arg(ap.parse_args(["--ema-decay", "1.0"]))
    with pytest.raises(ValueError, match="--swa-start"):
        trainer.averaging_arg(ap.parse_args(["--swa-start", "9", "--epochs", "4"]))


def test_trainer_rejects_both_flags_before_any_data_is_read(monkeypatch):
    """main() raises on the flags alone: the dataset and loader constructors are never reached"""
    import torch
    from utils import trainer
    touched = []
    monkeypatch.setattr(trainer, "synthetic_dataset", lambda *a, **k: touched.append("data"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr("sys.argv", ["trainer.py", "--task", "seg", "--ema-decay", "0.99", "--swa-start", "2"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(ValueError, match="mutually exclusive"):
        trainer.main()
    assert touched == []


def test_tester_flag_and_file_names():
    from utils import tester
    ap = tester.build_parser()
    assert ap.parse_args([]).weights_variant == "raw" and ap.parse_args(["--weights-variant", "swa"]).weights_variant == "swa"
    with pytest.raises(SystemExit):
        ap.parse_args(["--weights-variant", "best"])
    assert tester.variant_files(tester._CLS_FILES, "raw") is tester._CLS_FILES
    assert tester.variant_files(tester._CLS_FILES, "ema")["ResNet18"] == "ResNet18_ema_best_acc.pt"
    assert tester.variant_files(tester._SEG_FILES, "ema")["AttentionUNet"] == "AttentionUNet_ema_best_loss.pt"
    assert tester.variant_files(tester._SEG_FILES, "swa")["R2Unet"] == "R2Unet_swa.pt"
    assert tester.variant_files(tester._CLS_FILES, "swa")["VGG16"] == "VGG16_swa.pt"
    with pytest.raises(ValueError, match="weights_variant"):
        tester.variant_files(tester._SEG_FILES, "best")


def test_train_validates_the_averaging_argument_first():
    from mi355.averaging import WithAveraging
    from utils import helpers
    assert helpers._averaging_spec({"mode": "swa"}, 8) == ({"mode": "swa"}, "swa", 6)           # 75 % of the epochs
    assert helpers._averaging_spec({"mode": "ema", "decay": 0.9, "swa_start": 2}, 4)[1:] == ("ema", 2)
    with pytest.raises(ValueError):
        helpers._averaging_spec({"mode": "polyak"}, 4)
    with pytest.raises(ValueError):
        helpers._averaging_spec({"mode": "swa", "swa_start": 9}, 4)
    with pytest.raises(TypeError):
        helpers.train(None, WithAveraging(None, 3), None, "cpu", 2, 1e-3, "x", ".")
    w = WithAveraging([1, 2, 3], {"mode": "ema"})
    assert list(w) == [1, 2, 3] and len(w) == 3 and w.loader == [1, 2, 3] and w.averaging == {"mode": "ema"}


def test_with_averaging_inside_mixed_batches_is_an_error_not_a_dropped_request():
    """train() takes WithAveraging off first, then MixedBatches: in the other order the averaging request would be lost with the
    inner wrapper, so it raises"""
    import torch
    from mi355.averaging import WithAveraging
    from utils import helpers
    from utils.mix import MixedBatches
    with pytest.raises(TypeError, match="OUTSIDE MixedBatches"):
        helpers.train(torch.nn.Linear(2, 2), MixedBatches(WithAveraging([], {"mode": "ema"}), None), [], "cpu", 2, 1e-3, "x", ".")
