"""CPU: tests/distill_ref.py (the fp64 numpy restatement of the knowledge-distillation losses, csrc/distill.hip) pinned to torch's fp64
autograd to 1e-12, and the host-side surface of the feature: utils/distill.py, the trainer's flags, train()'s wrapper order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_ref as R

TEMPS = [0.5, 1.0, 2.0, 4.0]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


def _torch_kd_seg(z, t, v, bw, dw, smooth, ps, kw, T):
    z = torch.from_numpy(z).clone().requires_grad_(True)
    t, v = torch.from_numpy(t), torch.from_numpy(v)
    p = torch.sigmoid(z)
    dims = tuple(range(1, z.dim())) if ps else tuple(range(z.dim()))
    I, P, S = (p * t).sum(dims), p.sum(dims), t.sum(dims)
    dice = (1 - (2 * I + smooth) / (P + S + smooth)).mean()
    hard = bw * F.binary_cross_entropy_with_logits(z, t) + dw * dice
    a, b = z / T, v / T
    logp = torch.stack([F.logsigmoid(a), F.logsigmoid(-a)], -1)          # the two-class distributions
    q = torch.stack([torch.sigmoid(b), torch.sigmoid(-b)], -1)
    kd = T * T * F.kl_div(logp, q, reduction="sum") / z.numel()
    total = hard + kw * kd
    total.backward()
    return [float(total.detach()), float(hard.detach()), float(kd.detach()) if kw != 0 else 0.0], z.grad.numpy()      # (kd_weight 0: v is never read, KD is reported as 0)


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("shape", [(3, 1, 17, 13), (2, 1, 96, 172)])
def test_segmentation_restatement_is_torch_fp64_autograd(shape, T):
    rng = np.random.default_rng(sum(shape))
    z, v = rng.normal(0, 2, shape), rng.normal(0, 2, shape)
    t = (rng.random(shape) < 0.35).astype(np.float64)
    for ps in (False, True):
        for bw, dw, kw, smooth in ((0.5, 0.5, 0.5, 1.0), (0.0, 0.0, 1.0, 1.0), (1.0, 0.0, 0.0, 1.0), (0.3, 0.7, 0.25, 1e-3)):
            want, gwant = _torch_kd_seg(z, t, v, bw, dw, smooth, ps, kw, T)
            got, g = R.kd_seg(z, t, v, bw, dw, smooth, ps, kw, T)
            assert _close(got, want), (ps, bw, dw, kw, got, want)
            assert _close(g, gwant), (ps, bw, dw, kw)
    assert np.array_equal(R.kd_seg(z, t, v, 0.5, 0.5, 1.0, False, 0.5, T, gscale=3.0)[1], 3.0 * R.kd_seg(z, t, v, 0.5, 0.5, 1.0, False, 0.5, T)[1])


def test_segmentation_restatement_identities():
    rng = np.random.default_rng(5)
    z = rng.normal(0, 2, (2, 1, 9, 7))
    t = (rng.random(z.shape) < 0.5).astype(np.float64)
    (total, hard, kd), g = R.kd_seg(z, t, z.copy(), 0.5, 0.5, 1.0, False, 0.7, 2.0)
    (total0, hard0, kd0), g0 = R.kd_seg(z, t, None, 0.5, 0.5, 1.0, False, 0.0, 2.0)
    assert kd == 0.0 and kd0 == 0.0 and total == total0 == hard and np.array_equal(g, g0)
    # saturated, opposing: KL(Bern(q) || Bern(p)) = softplus(|a|) where q is 0 or 1
    (_, _, kd), g = R.kd_seg(np.full((1, 4), 100.0), np.ones((1, 4)), np.full((1, 4), -100.0), 0.0, 0.0, 1.0, False, 1.0, 0.5)
    assert abs(kd - 0.25 * 200.0) < 1e-12 and np.allclose(g, 0.5 / 4)


def _torch_ce_distill(z, y, v, w, s, hw, kw, T):
    z = torch.from_numpy(z).clone().requires_grad_(True)
    B, C = z.shape
    tgt = (1 - s) * F.one_hot(torch.from_numpy(y), C).double() + s / C
    hard = F.cross_entropy(z, tgt, weight=None if w is None else torch.from_numpy(w))
    kd = T * T * F.kl_div(F.log_softmax(z / T, 1), F.softmax(torch.from_numpy(v) / T, 1), reduction="batchmean")
    total = hw * hard + kw * kd
    total.backward()
    return [float(total.detach()), float(hard.detach()), float(kd.detach()) if kw != 0 else 0.0], z.grad.numpy()      # (kd_weight 0: v is never read, KD is reported as 0)


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("B,C", [(1, 3), (257, 3), (600, 10)])
def test_classifier_restatement_is_torch_fp64_autograd(B, C, T):
    rng = np.random.default_rng(100 * B + C)
    z, v = rng.normal(0, 3, (B, C)), rng.normal(0, 3, (B, C))
    y = rng.integers(0, C, B)
    w = 0.25 + 2 * rng.random(C)
    for weight in (None, w):
        for s, hw, kw in ((0.0, 0.5, 0.5), (0.1, 0.25, 0.75), (0.1, 1.0, 0.0), (0.0, 0.0, 1.0)):
            want, gwant = _torch_ce_distill(z, y, v, weight, s, hw, kw, T)
            got, g = R.ce_distill(z, y, v, weight, s, hw, kw, T)
            assert _close(got, want), (s, hw, kw, got, want)
            assert _close(g, gwant), (s, hw, kw)
    (total, hard, kd), _ = R.ce_distill(z, y, z.copy(), None, 0.1, 0.5, 0.5, T)
    assert kd == 0.0 and total == 0.5 * hard


# ---- utils/distill.py -------------------------------------------------------------------------------------------------------------------
def test_distill_target_surface():
    from utils.distill import DistillTarget
    y, v = torch.tensor([0, 2, 1]), torch.randn(3, 3, dtype=torch.float64)
    d = DistillTarget(y, v)
    assert d.hard is y and d.teacher_logits is v and d.size(0) == 3 and len(d) == 3 and d.size() == y.size()
    e = d.to("cpu", torch.float32)
    assert isinstance(e, DistillTarget) and e.hard.dtype == torch.int64 and e.teacher_logits.dtype == torch.float32
    assert d.to(torch.device("cpu"), non_blocking=True).hard.dtype == torch.int64
    assert "DistillTarget" in repr(d)
    with pytest.raises(ValueError, match="3 hard targets but 2 rows"):
        DistillTarget(y, v[:2])
    with pytest.raises(ValueError, match="floating point"):
        DistillTarget(y, y)
    with pytest.raises(TypeError, match="two tensors"):
        DistillTarget(y, None)


def test_teacher_logits_and_distilled_wrapper():
    from utils.distill import Distilled, DistillTarget, teacher_logits

    class Teacher(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.modes = []

        def forward(self, x):
            self.modes.append((self.training, torch.is_grad_enabled()))
            return (self.w * x.sum(1)).double()              # [N, H, W]: a segmenter that squeezed its channel

    t = Teacher().train()
    x = torch.randn(2, 3, 5, 4)
    v = teacher_logits(t, x)
    assert v.shape == (2, 1, 5, 4) and v.dtype == torch.float32 and not v.requires_grad and v.is_contiguous()
    assert t.modes == [(False, False)] and t.training                # eval mode and no graph inside, the previous mode put back
    t.eval()
    teacher_logits(t, x)
    assert not t.training
    with pytest.raises(TypeError, match="logit tensor"):
        teacher_logits(lambda x: (x, x), x)

    batches = [(torch.randn(2, 3, 5, 4), torch.rand(2, 1, 5, 4)) for _ in range(3)]
    dl = Distilled(batches, t)
    assert len(dl) == 3 and dl.loader is batches and dl.teacher is t
    got = list(dl)
    assert len(got) == 3 and all(isinstance(y, DistillTarget) for _, y in got)
    assert torch.equal(got[1][1].hard, batches[1][1]) and torch.equal(got[1][1].teacher_logits, teacher_logits(t, batches[1][0]))
    with pytest.raises(TypeError, match="callable"):
        Distilled(batches, 3)


def test_loss_modules_validate_their_arguments():
    from mi355 import nn as mnn
    for bad in (dict(kd_weight=-0.1), dict(kd_weight=1.5), dict(kd_weight=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
                dict(temperature=float("inf")), dict(temperature=float("nan"))):
        with pytest.raises(ValueError, match="kd_weight|temperature"):
            mnn.SegDistillationLoss(**bad)
        with pytest.raises(ValueError, match="kd_weight|temperature"):
            mnn.DistillCrossEntropyLoss(**bad)
    for bad in (dict(bce_weight=-1.0), dict(dice_weight=-1.0), dict(smooth=-1.0), dict(bce_weight=float("inf"))):
        with pytest.raises(ValueError, match="bce_weight|finite"):
            mnn.SegDistillationLoss(**bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        mnn.DistillCrossEntropyLoss(label_smoothing=1.5)
    for crit in (mnn.SegDistillationLoss(), mnn.DistillCrossEntropyLoss()):
        assert crit.accepts_mixed_target is False and crit.accepts_distill_target is True and crit.last_terms is None
    assert not hasattr(mnn.CombinedLoss(), "accepts_distill_target") and not hasattr(mnn.MixCrossEntropyLoss(), "accepts_distill_target")
    c = mnn.SegDistillationLoss()
    assert (c.bce_weight, c.dice_weight, c.smooth, c.per_sample, c.kd_weight, c.temperature) == (0.5, 0.5, 1.0, False, 0.5, 2.0)
    c = mnn.DistillCrossEntropyLoss()
    assert (c.kd_weight, c.temperature, c.label_smoothing, c.weight, c.check_labels) == (0.5, 4.0, 0.0, None, False)


def test_abi_rejects_bad_arguments_before_the_device_is_touched():
    """mi355_kd_seg_* / mi355_ce_distill: null pointers, B > 65535, T not finite or <= 0, negative weights -> MI355_ERR_ARG (-1)"""
    import ctypes
    import os
    from mi355 import lib as L
    if not os.path.exists(L.SO_PATH):
        pytest.skip("libmi355conv.so not built (run __graft_entry__.build())")
    dll = ctypes.CDLL(L.SO_PATH)
    dll.mi355_last_error.restype = ctypes.c_char_p
    protos = L.parse_header()

    def fn(name):
        f = getattr(dll, name)
        f.restype = ctypes.c_int
        f.argtypes = [t for t, _ in protos[name][1]]
        return f

    p = ctypes.c_void_p(4096)          # never dereferenced: every call below fails its argument check
    rows, fwd, bwd, ce = fn("mi355_kd_seg_rows"), fn("mi355_kd_seg_fwd"), fn("mi355_kd_seg_bwd"), fn("mi355_ce_distill")
    assert rows(0, 10) == -1 and rows(65536, 10) == -1 and rows(2, 0) == -1
    assert rows(3, 221) == 3 and rows(1, 4096) == 1 and rows(2, 16512) == 8 and rows(32, 65536) == 32 * 16
    inf, nan = float("inf"), float("nan")
    ok = dict(z=p, t=p, v=p, B=2, per=16, bw=0.5, dw=0.5, sm=1.0, ps=0, kw=0.5, T=2.0, partial=p, state=p, loss=p)

    def call_fwd(**kw):
        a = dict(ok, **kw)
        return fwd(a["z"], a["t"], a["v"], a["B"], a["per"], a["bw"], a["dw"], a["sm"], a["ps"], a["kw"], a["T"], a["partial"], a["state"],
                   a["loss"], None)

    for bad in (dict(z=None), dict(t=None), dict(v=None), dict(partial=None), dict(state=None), dict(loss=None), dict(B=65536), dict(B=0),
                dict(per=0), dict(T=0.0), dict(T=-1.0), dict(T=inf), dict(T=nan), dict(bw=-1.0), dict(dw=-1.0), dict(kw=-1.0), dict(sm=-1.0),
                dict(partial=ctypes.c_void_p(4100))):
        assert call_fwd(**bad) == -1, bad
        assert b"kd_seg_fwd" in dll.mi355_last_error()

    def call_bwd(**kw):
        a = dict(dict(ok, dz=p, gs=None), **kw)
        return bwd(a["z"], a["t"], a["v"], a["B"], a["per"], a["bw"], a["kw"], a["T"], a["state"], a["gs"], a["dz"], None)

    for bad in (dict(z=None), dict(t=None), dict(v=None), dict(state=None), dict(dz=None), dict(B=65536), dict(T=0.0), dict(T=nan),
                dict(T=inf), dict(bw=-1.0), dict(kw=-1.0)):
        assert call_bwd(**bad) == -1, bad
        assert b"kd_seg_bwd" in dll.mi355_last_error()

    def call_ce(**kw):
        a = dict(dict(z=p, y=p, v=p, w=None, loss=p, dz=None, gs=None, B=4, C=3, s=0.1, hw=0.5, kw=0.5, T=4.0), **kw)
        return ce(a["z"], a["y"], a["v"], a["w"], a["loss"], a["dz"], a["gs"], a["B"], a["C"], a["s"], a["hw"], a["kw"], a["T"], None)

    for bad in (dict(z=None), dict(y=None), dict(v=None), dict(loss=None), dict(B=0), dict(C=0), dict(T=0.0), dict(T=-2.0), dict(T=inf),
                dict(T=nan), dict(hw=-1.0), dict(kw=-1.0), dict(s=-0.1), dict(s=1.5)):
        assert call_ce(**bad) == -1, bad
        assert b"ce_distill" in dll.mi355_last_error()


# ---- trainer flags ----------------------------------------------------------------------------------------------------------------------
def test_distill_arg_defaults_and_errors():
    from utils import trainer
    ap = trainer.build_parser()
    args = ap.parse_args([])
    assert args.teacher is None and args.teacher_model is None and args.kd_weight == 0.5 and args.kd_temperature is None
    assert trainer.distill_arg(args) is None
    base = ["--teacher", "t.pt", "--teacher-model", "attentionunet"]
    assert trainer.distill_arg(ap.parse_args(base)) == dict(path="t.pt", model="attentionunet", kd_weight=0.5, temperature=2.0)
    cls = ["--task", "cls", "--teacher", "t.pt", "--teacher-model", "resnet50"]
    assert trainer.distill_arg(ap.parse_args(cls)) == dict(path="t.pt", model="resnet50", kd_weight=0.5, temperature=4.0)
    assert trainer.distill_arg(ap.parse_args(base + ["--kd-weight", "1", "--kd-temperature", "3", "--seg-loss", "bce_dice"])) == \
        dict(path="t.pt", model="attentionunet", kd_weight=1.0, temperature=3.0)
    for flags, msg in ((["--teacher", "t.pt"], "go together"),
                       (["--teacher-model", "resnet18"], "go together"),
                       (base + ["--task", "both"], "one teacher fits one task"),
                       (base + ["--seg-loss", "lovasz"], "bce\\|dice\\|bce_dice"),
                       (base + ["--seg-loss", "focal_dice"], "bce\\|dice\\|bce_dice"),
                       (base + ["--boundary-weight", "0.01"], "--boundary-weight"),
                       (base + ["--lovasz-weight", "0.5"], "--lovasz-weight"),
                       (base + ["--seg-classes", "3"], "--seg-classes"),
                       (cls + ["--cls-loss", "focal"], "--cls-loss focal"),
                       (cls + ["--mixup-alpha", "0.2"], "--mixup-alpha"),
                       (cls + ["--cutmix-alpha", "1.0"], "--cutmix-alpha"),
                       (base + ["--kd-weight", "1.5"], "--kd-weight"),
                       (base + ["--kd-weight", "-0.1"], "--kd-weight"),
                       (base + ["--kd-weight", "nan"], "--kd-weight"),
                       (base + ["--kd-temperature", "0"], "--kd-temperature"),
                       (base + ["--kd-temperature", "-2"], "--kd-temperature"),
                       (base + ["--kd-temperature", "inf"], "--kd-temperature"),
                       (base + ["--kd-temperature", "nan"], "--kd-temperature")):
        with pytest.raises(ValueError, match=msg):
            trainer.distill_arg(ap.parse_args(flags))
    # segmentation CutMix stays allowed next to a teacher (the teacher sees the mixed image)
    assert trainer.distill_arg(ap.parse_args(base + ["--cutmix-alpha", "1.0"])) is not None


def test_distill_criterion_follows_the_flags():
    from mi355 import nn as mnn
    from utils import trainer
    ap = trainer.build_parser()
    base = ["--teacher", "t.pt", "--teacher-model", "attentionunet"]
    for flags, want in (([], (1.0, 0.0)), (["--seg-loss", "dice"], (0.0, 1.0)),
                        (["--seg-loss", "bce_dice", "--bce-weight", "0.3", "--dice-weight", "0.7"], (0.3, 0.7))):
        args = ap.parse_args(base + flags + ["--kd-weight", "0.25", "--dice-per-sample"])
        crit = trainer.distill_criterion(args, trainer.distill_arg(args))
        assert isinstance(crit, mnn.SegDistillationLoss) and (crit.bce_weight, crit.dice_weight) == want
        assert crit.kd_weight == 0.25 and crit.temperature == 2.0 and crit.per_sample
    args = ap.parse_args(["--task", "cls", "--teacher", "t.pt", "--teacher-model", "resnet50"])
    crit = trainer.distill_criterion(args, trainer.distill_arg(args), [1.0, 2.0, 0.5])
    assert isinstance(crit, mnn.DistillCrossEntropyLoss) and crit.label_smoothing == 0.1 and crit.temperature == 4.0
    assert crit.weight.tolist() == [1.0, 2.0, 0.5]


def test_trainer_rejects_distill_flags_before_any_data_is_read(monkeypatch):
    from utils import trainer
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(trainer, "synthetic_dataset", lambda *a, **k: touched.append("data"))
    monkeypatch.setattr(trainer, "load_teacher", lambda *a, **k: touched.append("teacher"))
    monkeypatch.setattr("sys.argv", ["trainer.py", "--task", "seg", "--teacher", "t.pt"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(ValueError, match="go together"):
        trainer.main()
    assert touched == []


# ---- train(): wrapper order ------------------------------------------------------------------------------------------------------------
def test_train_names_the_wrapper_order():
    """train() takes WithAveraging off first, then Distilled, then MixedBatches; any other nesting raises before the model is moved"""
    from mi355.averaging import WithAveraging
    from utils import helpers
    from utils.distill import Distilled
    from utils.mix import MixedBatches

    class Model(torch.nn.Linear):
        def to(self, *a, **k):
            raise AssertionError("the model was moved before the wrapper order was checked")

    teacher = torch.nn.Linear(2, 2)
    order = r"WithAveraging\(Distilled\(MixedBatches\(loader, batch_mix\), teacher\), averaging\)"
    with pytest.raises(TypeError, match="OUTSIDE Distilled.*" + order):
        helpers.train(Model(2, 2), Distilled(WithAveraging([], {"mode": "ema"}), teacher), [], "cpu", 2, 1e-3, "x", ".")
    with pytest.raises(TypeError, match="Distilled goes OUTSIDE MixedBatches.*" + order):
        helpers.train(Model(2, 2), MixedBatches(Distilled([], teacher), None), [], "cpu", 2, 1e-3, "x", ".")
    with pytest.raises(TypeError, match="Distilled goes OUTSIDE MixedBatches"):
        helpers.train(Model(2, 2), WithAveraging(MixedBatches(Distilled([], teacher), None), None), [], "cpu", 2, 1e-3, "x", ".")
    teacher.train()
    with pytest.raises(TypeError, match="OUTSIDE Distilled"):
        helpers.train(Model(2, 2), Distilled(WithAveraging([], None), teacher), [], "cpu", 2, 1e-3, "x", ".")
    assert teacher.training                                  # the mode the teacher came with
