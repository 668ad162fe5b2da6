"""CPU: the focal / Tversky / focal-Tversky losses and the focal cross-entropy below the GPU — the fp64 restatement
(tests/focal_ref.py) against torch's fp64 autograd of the same formulas written with torch ops (the focal term is the body of
torchvision.ops.sigmoid_focal_loss, restated where torchvision is not installed), the identities that tie the new losses to the ones
the project has, the C ABI (declared, exported, known to the plan engine, arguments validated before the device is touched) and the
Python surface (``mi355.nn``, the trainer's command line)."""
import ctypes
import inspect
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as R
import seg_loss_ref as S
from mi355 import lib as L

EPS = 1e-12
GAMMAS, ALPHAS = (0.0, 0.5, 2.0), (-1.0, 0.25)
AB = ((0.5, 0.5), (0.7, 0.3), (0.3, 0.7))
EXPS = (1.0, 0.75, 2.0)


def _sigmoid_focal_loss(z, t, alpha, gamma):
    try:
        from torchvision.ops import sigmoid_focal_loss
        return sigmoid_focal_loss(z, t, alpha=alpha, gamma=gamma, reduction="none")
    except ImportError:                                  # torchvision/ops/focal_loss.py, restated
        p = torch.sigmoid(z)
        ce = F.binary_cross_entropy_with_logits(z, t, reduction="none")
        p_t = p * t + (1 - p) * (1 - t)
        loss = ce * ((1 - p_t) ** gamma)
        if alpha >= 0:
            loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
        return loss


def _torch_ftv(z, t, fw, tw, a, b, g, fa, fg, sm, ps):
    z = torch.from_numpy(z).double().requires_grad_(True)
    t = torch.from_numpy(t).double()
    loss = fw * _sigmoid_focal_loss(z, t, fa, fg).mean()
    p = torch.sigmoid(z)
    dims = tuple(range(1, z.dim())) if ps else tuple(range(z.dim()))
    tp, fp, fn = (p * t).sum(dims), (p * (1 - t)).sum(dims), ((1 - p) * t).sum(dims)
    ti = (tp + sm) / (tp + a * fp + b * fn + sm)
    loss = loss + tw * ((1 - ti) ** g).mean()
    loss.backward()
    return float(loss.detach()), z.grad.numpy()


def _data(shape=(3, 1, 9, 11), seed=5):
    rng = np.random.RandomState(seed)
    return rng.randn(*shape) * 2, (rng.rand(*shape) < 0.35).astype(np.float64)


@pytest.mark.parametrize("ps", [False, True])
def test_restatement_matches_torch_autograd(ps):
    """Both are fp64 evaluations of one expression: 1e-12 of the loss, 1e-12 of the gradient tensor's maximum.  The whole grid:
    gamma x alpha x (a, b) x g x weights."""
    z, t = _data()
    n = 0
    for fg, fa, (a, b), g, (fw, tw) in itertools.product(GAMMAS, ALPHAS, AB, EXPS, ((1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.3, 0.7))):
        for sm in (1.0, 1e-3):
            want = _torch_ftv(z, t, fw, tw, a, b, g, fa, fg, sm, ps)
            got = R.ftv_loss(z, t, fw, tw, a, b, g, fa, fg, sm, ps)
            assert abs(got[0] - want[0]) <= EPS * max(1.0, abs(want[0])), (fg, fa, a, b, g, fw, tw, sm, got[0], want[0])
            assert np.abs(got[1] - want[1]).max() <= EPS * max(np.abs(want[1]).max(), 1e-3), (fg, fa, a, b, g, fw, tw, sm)
            n += 1
    assert n == 3 * 2 * 3 * 3 * 4 * 2


def test_restatement_binarises_the_target_and_scales_the_gradient():
    z, t = _data()
    soft = np.where(t > 0, 0.6 + 0.4 * np.random.RandomState(1).rand(*t.shape), 0.5 * np.random.RandomState(2).rand(*t.shape))
    a, b = R.ftv_loss(z, t, 0.5, 0.5), R.ftv_loss(z, soft, 0.5, 0.5)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    c = R.ftv_loss(z, t, 0.5, 0.5, gscale=3.0)
    assert c[0] == a[0] and np.allclose(c[1], 3.0 * a[1], rtol=1e-15, atol=0)


def test_restatement_gradient_is_the_derivative_of_its_loss():
    rng = np.random.RandomState(7)
    z, t = rng.randn(2, 1, 4, 5), (rng.rand(2, 1, 4, 5) < 0.5).astype(np.float64)
    for ps in (False, True):
        kw = dict(focal_weight=0.4, tversky_weight=0.6, alpha=0.3, beta=0.7, exponent=0.75, focal_alpha=0.25, focal_gamma=0.5, per_sample=ps)
        _, g = R.ftv_loss(z, t, **kw)
        for idx in [(0, 0, 0, 0), (1, 0, 3, 4), (0, 0, 2, 1)]:
            h = 1e-6
            zp, zm = z.copy(), z.copy()
            zp[idx] += h
            zm[idx] -= h
            fd = (R.ftv_loss(zp, t, **kw)[0] - R.ftv_loss(zm, t, **kw)[0]) / (2 * h)
            assert abs(fd - g[idx]) < 1e-8, (ps, idx, fd, g[idx])


def test_restatement_corner_cases():
    """saturated logits: finite; the perfect saturated prediction: Tversky term and gradient exactly 0; gamma = 0 with u = 0"""
    t = (np.random.RandomState(3).rand(2, 1, 8, 8) < 0.5).astype(np.float64)
    for mag in (30.0, 100.0, 1000.0):
        z = np.where(t > 0, mag, -mag)
        for g in (0.75, 1.0, 2.0):
            for fg in (0.0, 0.5, 2.0):
                l, d = R.ftv_loss(z, t, 0.5, 0.5, exponent=g, focal_gamma=fg)
                assert np.isfinite(l) and np.all(np.isfinite(d)), (mag, g, fg)
                l, d = R.ftv_loss(-z, t, 0.5, 0.5, exponent=g, focal_gamma=fg)
                assert np.isfinite(l) and np.all(np.isfinite(d)), (mag, g, fg)
    z = np.where(t > 0, 1000.0, -1000.0)                 # exp(-1000) = 0 in double: p = t exactly
    l, d = R.ftv_loss(z, t, 0.0, 1.0, exponent=0.75)
    assert l == 0.0 and not d.any()
    l, d = R.ftv_loss(z, t, 1.0, 0.0, focal_gamma=0.0, focal_alpha=-1.0)
    assert l == 0.0 and not d.any()
    l, d = R.ftv_loss(z, np.zeros_like(t), 0.0, 1.0, smooth=0.0)      # all-zero target, smooth 0: Den = a P
    assert np.isfinite(l) and np.all(np.isfinite(d))


@pytest.mark.parametrize("ps", [False, True])
def test_tversky_half_half_is_dice_with_twice_the_smooth(ps):
    z, t = _data()
    for s in (0.5, 1.0, 1e-3):
        a, b = R.tversky_loss(z, t, 0.5, 0.5, smooth=s, per_sample=ps), S.dice_loss(z, t, smooth=2 * s, per_sample=ps)
        assert abs(a[0] - b[0]) <= EPS and np.abs(a[1] - b[1]).max() <= EPS * np.abs(b[1]).max()


def test_focal_without_focus_and_balance_is_mean_bce():
    z, t = _data()
    a, b = R.focal_loss(z, t, alpha=-1.0, gamma=0.0), S.seg_loss(z, t, 1.0, 0.0)
    assert abs(a[0] - b[0]) <= EPS and np.abs(a[1] - b[1]).max() <= EPS * np.abs(b[1]).max()


def _ce_data(B=7, C=3, seed=0):
    rng = np.random.RandomState(seed)
    z = rng.randn(B, C) * 3
    z[0, 0] += 60.0
    return z, rng.randint(0, C, B), 0.25 + 2 * rng.rand(C)


@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("weighted", [False, True])
def test_ce_focal_restatement_matches_torch_autograd(C, weighted):
    z, y, w = _ce_data(C=C)
    y[0] = 0                                             # the +60 logit is the true class: u ~ 1e-26
    w = w if weighted else None
    for gamma in GAMMAS:
        zt = torch.from_numpy(z).double().requires_grad_(True)
        logp = F.log_softmax(zt, 1)
        hot = F.one_hot(torch.from_numpy(y), C).bool()
        logpy = logp[hot]
        u = torch.where(hot, torch.zeros_like(logp), logp.exp()).sum(1)
        wy = torch.ones(len(y), dtype=torch.float64) if w is None else torch.from_numpy(w)[torch.from_numpy(y)]
        loss = (wy * (u ** gamma if gamma else 1.0) * -logpy).sum() / len(y)
        loss.backward()
        got = R.ce_focal(z, y, w, gamma)
        assert abs(got[0] - float(loss.detach())) <= EPS * max(1.0, float(loss.detach())), (gamma, got[0], float(loss.detach()))
        assert np.abs(got[1] - zt.grad.numpy()).max() <= EPS * max(np.abs(zt.grad.numpy()).max(), 1e-3), gamma
        if gamma == 0:
            want = F.cross_entropy(torch.from_numpy(z), torch.from_numpy(y), weight=None if w is None else torch.from_numpy(w),
                                   reduction="sum") / len(y)
            assert abs(got[0] - float(want)) <= EPS * max(1.0, float(want))
        assert np.all(np.isfinite(got[1]))
    # a row without any weight on the other classes: loss 0, gradient 0, for every gamma > 0
    zz = np.array([[800.0, 0.0, -3.0]])
    for gamma in (0.5, 2.0):
        l, d = R.ce_focal(zz, [0], None, gamma)
        assert l == 0.0 and not d.any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
NEW = ("mi355_ftv_loss_rows", "mi355_ftv_loss_fwd", "mi355_ftv_loss_bwd", "mi355_ce_focal")


def test_abi_declares_exports_and_replays_the_new_entry_points():
    protos = L.parse_header()
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name in NEW:
        assert name in protos and protos[name][0] is ctypes.c_int, name
        assert hasattr(dll, name), name
        assert arity(name.encode()) == len(protos[name][1]), name
    assert [n for _, n in protos["mi355_ftv_loss_fwd"][1]] == ["z", "t", "B", "per", "focal_weight", "focal_alpha", "focal_gamma",
                                                               "tversky_weight", "tv_a", "tv_b", "tv_exp", "smooth", "per_sample",
                                                               "partial", "state", "loss", "s"]
    assert [n for _, n in protos["mi355_ftv_loss_bwd"][1]] == ["z", "t", "B", "per", "focal_weight", "focal_alpha", "focal_gamma", "tv_a",
                                                               "tv_b", "state", "gscale", "dz", "s"]
    assert [n for _, n in protos["mi355_ce_focal"][1]] == ["z", "y", "weight", "loss", "dz", "gscale", "B", "C", "gamma", "s"]
    rows = L.lib.raw("mi355_ftv_loss_rows")
    assert rows(32, 256 * 256) >= 32 and rows(2, 17 * 13) == 2 and rows(1, 1) == 1 and rows(2, 96 * 172) > 2
    assert rows(32, 256 * 256) <= 4096 and rows(65535, 4) == 65535


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    fwd, bwd, rows, cef = (lib.raw(n) for n in ("mi355_ftv_loss_fwd", "mi355_ftv_loss_bwd", "mi355_ftv_loss_rows", "mi355_ce_focal"))
    buf = (ctypes.c_float * 64)()                       # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(z=p, t=p, B=2, per=8, fw=0.5, fa=0.25, fg=2.0, tw=0.5, a=0.7, b=0.3, g=0.75, sm=1.0, ps=0, partial=p, state=p, loss=p,
              gscale=None, dz=p)
    nan = float("nan")

    def call_fwd(**kw):
        a = dict(ok, **kw)
        return fwd(a["z"], a["t"], a["B"], a["per"], a["fw"], a["fa"], a["fg"], a["tw"], a["a"], a["b"], a["g"], a["sm"], a["ps"],
                   a["partial"], a["state"], a["loss"], None)

    def call_bwd(**kw):
        a = dict(ok, **kw)
        return bwd(a["z"], a["t"], a["B"], a["per"], a["fw"], a["fa"], a["fg"], a["a"], a["b"], a["state"], a["gscale"], a["dz"], None)

    shared = (({"z": None}, b"null"), ({"t": None}, b"null"), ({"state": None}, b"null"), ({"B": 0}, b"B"), ({"B": -3}, b"B"),
              ({"B": 65536}, b"B"), ({"per": 0}, b"per"), ({"fw": -0.5}, b"focal_weight"), ({"fw": nan}, b"focal_weight"),
              ({"fg": -1.0}, b"focal_gamma"), ({"fa": 1.5}, b"focal_alpha"), ({"fa": nan}, b"focal_alpha"), ({"a": -0.1}, b"tv_a"),
              ({"b": -0.1}, b"tv_b"), ({"a": 0.0, "b": 0.0}, b"tv_a + tv_b"), ({"a": nan}, b"tv_a"))
    for bad, word in shared + (({"partial": None}, b"null"), ({"loss": None}, b"null"), ({"tw": -1.0}, b"tversky_weight"),
                               ({"sm": -1e-3}, b"smooth"), ({"g": 0.0}, b"tv_exp"), ({"g": -1.0}, b"tv_exp"), ({"g": nan}, b"tv_exp")):
        assert call_fwd(**bad) == -1, bad
        assert b"ftv_loss_fwd" in err() and word in err(), (bad, err())
    for bad, word in shared + (({"dz": None}, b"null"),):
        assert call_bwd(**bad) == -1, bad
        assert b"ftv_loss_bwd" in err() and word in err(), (bad, err())
    assert rows(0, 8) == -1 and rows(2, 0) == -1 and rows(65536, 8) == -1 and b"ftv_loss_rows" in err()
    for args, word in (((None, p, None, p, None, None, 2, 3, 2.0, None), b"null"), ((p, None, None, p, None, None, 2, 3, 2.0, None), b"null"),
                       ((p, p, None, None, None, None, 2, 3, 2.0, None), b"null"), ((p, p, None, p, None, None, 0, 3, 2.0, None), b"B"),
                       ((p, p, None, p, None, None, 2, 0, 2.0, None), b"C"), ((p, p, None, p, None, None, 2, 3, -1.0, None), b"gamma"),
                       ((p, p, None, p, None, None, 2, 3, nan, None), b"gamma")):
        assert cef(*args) == -1, args
        assert b"ce_focal" in err() and word in err(), (args, err())


# ---- mi355.nn ----------------------------------------------------------------------------------------------------------------------
def test_loss_modules_constructors_and_their_errors():
    from mi355 import nn as mnn
    sig = inspect.signature(mnn.FocalTverskyLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == \
        [("focal_weight", 0.0), ("tversky_weight", 1.0), ("alpha", 0.7), ("beta", 0.3), ("exponent", 0.75), ("focal_alpha", 0.25),
         ("focal_gamma", 2.0), ("smooth", 1.0), ("per_sample", False)]
    sig = inspect.signature(mnn.FocalLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("alpha", 0.25), ("gamma", 2.0)]
    sig = inspect.signature(mnn.TverskyLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("alpha", 0.5), ("beta", 0.5), ("smooth", 1.0), ("per_sample", False)]
    sig = inspect.signature(mnn.FocalCrossEntropyLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:3]] == [("gamma", 2.0), ("weight", None)]

    def cfg(c):
        return (c.focal_weight, c.tversky_weight, c.alpha, c.beta, c.exponent, c.focal_alpha, c.focal_gamma, c.smooth, c.per_sample)

    assert cfg(mnn.FocalTverskyLoss()) == (0.0, 1.0, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0, False)
    f = mnn.FocalLoss(alpha=-1, gamma=0)
    assert isinstance(f, mnn.FocalTverskyLoss) and cfg(f)[:2] == (1.0, 0.0) and cfg(f)[5:7] == (-1.0, 0.0)
    t = mnn.TverskyLoss(0.3, 0.7, 0.5, True)
    assert isinstance(t, mnn.FocalTverskyLoss) and cfg(t) == (0.0, 1.0, 0.3, 0.7, 1.0, 0.25, 2.0, 0.5, True)
    nan = float("nan")
    for kw in (dict(focal_weight=-0.1), dict(tversky_weight=-1), dict(smooth=-1e-3), dict(alpha=-0.1), dict(beta=-0.1), dict(alpha=0, beta=0),
               dict(exponent=0), dict(exponent=-1), dict(focal_gamma=-0.5), dict(focal_alpha=1.5), dict(focal_weight=nan), dict(exponent=nan),
               dict(focal_alpha=nan), dict(alpha=float("inf")), dict(focal_gamma=float("inf"))):
        with pytest.raises(ValueError):
            mnn.FocalTverskyLoss(**kw)
    for bad in (lambda: mnn.FocalLoss(gamma=-1), lambda: mnn.FocalLoss(alpha=2), lambda: mnn.TverskyLoss(0, 0), lambda: mnn.TverskyLoss(smooth=-1),
                lambda: mnn.FocalCrossEntropyLoss(gamma=-1), lambda: mnn.FocalCrossEntropyLoss(gamma=nan),
                lambda: mnn.FocalCrossEntropyLoss(weight=[1.0, -1.0, 1.0]), lambda: mnn.FocalCrossEntropyLoss(weight=[])):
        with pytest.raises(ValueError):
            bad()
    c = mnn.FocalCrossEntropyLoss(0.5, [1.0, 2.0, 0.5])
    assert c.gamma == 0.5 and c.weight.dtype == torch.float32 and c.weight.tolist() == [1.0, 2.0, 0.5]
    assert not getattr(c, "accepts_mixed_target", False) and mnn.MixCrossEntropyLoss.accepts_mixed_target
    z = torch.zeros(2, 3)
    for bad_target in (torch.zeros(2), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 3])):
        with pytest.raises(ValueError):
            c(z, bad_target)
    with pytest.raises(ValueError, match="classes"):
        mnn.FocalCrossEntropyLoss(2.0, [1.0, 2.0])(z, torch.tensor([0, 1]))


# ---- utils/trainer.py ---------------------------------------------------------------------------------------------------------------
def test_trainer_builds_the_new_criteria():
    from mi355 import nn as mnn
    from utils import trainer
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert (d.focal_gamma, d.focal_alpha, d.tversky_alpha, d.tversky_beta, d.tversky_exponent, d.focal_weight, d.tversky_weight, d.cls_loss) == \
        (2.0, 0.25, 0.7, 0.3, 0.75, 0.5, 0.5, "ce")

    def cfg(argv):
        c = trainer.seg_criterion(ap.parse_args(argv))
        assert type(c) is mnn.FocalTverskyLoss
        return (c.focal_weight, c.tversky_weight, c.alpha, c.beta, c.exponent, c.focal_alpha, c.focal_gamma, c.smooth, c.per_sample)

    # the focal loss alone: focal_dice without the Dice term (the name "focal" stays a choice the parser rejects)
    assert cfg(["--seg-loss", "focal_dice", "--focal-weight", "1", "--tversky-weight", "0"]) == (1.0, 0.0, 0.5, 0.5, 1.0, 0.25, 2.0, 1.0, False)
    assert cfg(["--seg-loss", "focal_dice", "--focal-gamma", "0.5", "--focal-alpha", "-1"])[5:7] == (-1.0, 0.5)
    with pytest.raises(SystemExit):
        ap.parse_args(["--seg-loss", "focal"])
    assert cfg(["--seg-loss", "tversky"]) == (0.0, 1.0, 0.7, 0.3, 1.0, 0.25, 2.0, 1.0, False)
    assert cfg(["--seg-loss", "tversky", "--tversky-alpha", "0.3", "--tversky-beta", "0.7", "--dice-per-sample", "--tversky-exponent", "2"]) == \
        (0.0, 1.0, 0.3, 0.7, 1.0, 0.25, 2.0, 1.0, True)
    assert cfg(["--seg-loss", "focal_tversky"]) == (0.0, 1.0, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0, False)
    assert cfg(["--seg-loss", "focal_tversky", "--tversky-exponent", "0.5", "--tversky-alpha", "0.4", "--tversky-beta", "0.6"])[2:5] == (0.4, 0.6, 0.5)
    assert cfg(["--seg-loss", "focal_dice"]) == (0.5, 0.5, 0.5, 0.5, 1.0, 0.25, 2.0, 1.0, False)
    assert cfg(["--seg-loss", "focal_dice", "--focal-weight", "0.3", "--tversky-weight", "0.7", "--tversky-alpha", "0.9", "--dice-per-sample",
                "--focal-gamma", "1"]) == (0.3, 0.7, 0.5, 0.5, 1.0, 0.25, 1.0, 1.0, True)
    c = trainer.cls_criterion(ap.parse_args(["--task", "cls", "--cls-loss", "focal", "--focal-gamma", "1.5"]), None)
    assert type(c) is mnn.FocalCrossEntropyLoss and c.gamma == 1.5 and c.weight is None

    class Files:
        samples = [("a", 0), ("b", 0), ("c", 1), ("d", 2)]

    said = []
    c = trainer.cls_criterion(ap.parse_args(["--task", "cls", "--cls-loss", "focal", "--class-weight", "balanced"]), None, Files(), None, said.append)
    assert type(c) is mnn.FocalCrossEntropyLoss and c.gamma == 2.0 and np.allclose(c.weight.tolist(), [4 / 6, 4 / 3, 4 / 3]) and len(said) == 1
    said = []
    c = trainer.cls_criterion(ap.parse_args(["--task", "cls", "--cls-loss", "focal", "--class-weight", "balanced"]), None, None, None, said.append)
    assert type(c) is mnn.FocalCrossEntropyLoss and c.weight is None and "ignored" in said[0]


FORBIDDEN = [(["--seg-loss", s] + extra, word) for s in ("tversky", "focal_tversky", "focal_dice")
             for extra, word in ((["--boundary-weight", "0.1"], "--boundary-weight"), (["--lovasz-weight", "0.5"], "--lovasz-weight"),
                                 (["--seg-classes", "3"], "--seg-loss " + s))]


@pytest.mark.parametrize("argv,word", FORBIDDEN)
def test_trainer_rejects_the_new_seg_losses_next_to_terms_they_do_not_combine_with(argv, word):
    from utils import trainer
    with pytest.raises(ValueError, match=word):
        trainer.seg_criterion(trainer.build_parser().parse_args(argv))


def test_trainer_rejects_values_out_of_range_and_focal_ce_on_mixed_batches():
    from utils import trainer
    ap = trainer.build_parser()
    for argv, word in ((["--seg-loss", "focal_dice", "--focal-gamma", "-1"], "--focal-gamma"), (["--seg-loss", "focal_dice", "--focal-alpha", "1.5"], "--focal-alpha"),
                       (["--seg-loss", "tversky", "--tversky-alpha", "-0.1"], "--tversky-alpha"),
                       (["--seg-loss", "tversky", "--tversky-alpha", "0", "--tversky-beta", "0"], "--tversky-beta"),
                       (["--seg-loss", "focal_tversky", "--tversky-exponent", "0"], "--tversky-exponent"),
                       (["--seg-loss", "focal_dice", "--focal-weight", "-1"], "--focal-weight"),
                       (["--seg-loss", "focal_dice", "--tversky-weight", "nan"], "--tversky-weight"),
                       (["--seg-loss", "focal_dice", "--focal-gamma", "nan"], "--focal-gamma")):
        with pytest.raises(ValueError, match=word):
            trainer.seg_criterion(ap.parse_args(argv))
        with pytest.raises(ValueError, match=word):
            trainer.focal_arg(ap.parse_args(argv))
    for argv, word in ((["--task", "cls", "--cls-loss", "focal", "--mixup-alpha", "0.2"], "--mixup-alpha"),
                       (["--task", "cls", "--cls-loss", "focal", "--cutmix-alpha", "1.0"], "--cutmix-alpha"),
                       (["--task", "both", "--cls-loss", "focal", "--cutmix-alpha", "1.0"], "--cutmix-alpha"),
                       (["--task", "cls", "--cls-loss", "focal", "--mixup-alpha", "0.2", "--cutmix-alpha", "1.0"], "--mixup-alpha, --cutmix-alpha"),
                       (["--task", "cls", "--cls-loss", "focal", "--focal-gamma", "-2"], "--focal-gamma"),
                       (["--task", "seg", "--cls-loss", "focal"], "classifiers")):
        with pytest.raises(ValueError, match=word):
            trainer.cls_loss_arg(ap.parse_args(argv))
        with pytest.raises(ValueError, match=word):
            trainer.cls_criterion(ap.parse_args(argv), None)
    with pytest.raises(SystemExit):
        ap.parse_args(["--cls-loss", "hinge"])
    # the range flags are read by the new losses only: out of range next to another loss, nothing is raised
    assert trainer.seg_criterion(ap.parse_args(["--focal-gamma", "-1", "--tversky-exponent", "0"])) is None
    assert trainer.focal_arg(ap.parse_args(["--seg-loss", "dice", "--focal-alpha", "7"])) is None


def test_default_flags_build_what_they_built():
    from mi355 import nn as mnn
    from utils import trainer
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert trainer.seg_criterion(d) is None and trainer.focal_arg(d) is None and trainer.cls_loss_arg(d) is False
    assert trainer.cls_criterion(ap.parse_args(["--task", "cls"]), None) is None
    said = []
    assert trainer.cls_criterion(ap.parse_args(["--task", "cls", "--class-weight", "balanced"]), None, None, None, said.append) is None
    assert said == ["--class-weight balanced needs the file list of --data-root: ignored for synthetic data"]

    class Files:
        samples = [("a", 0), ("b", 0), ("c", 1), ("d", 2)]

    said = []
    c = trainer.cls_criterion(ap.parse_args(["--task", "cls", "--class-weight", "balanced"]), None, Files(), [0, 2, 3], said.append)
    assert type(c) is mnn.MixCrossEntropyLoss and c.label_smoothing == 0.1 and np.allclose(c.weight.tolist(), [1.0, 1.0, 1.0])
    assert len(said) == 1 and said[0].startswith("class weights (balanced): ")
    assert type(trainer.seg_criterion(ap.parse_args(["--seg-loss", "dice"]))) is mnn.DiceLoss
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "bce_dice"]))
    assert type(c) is mnn.CombinedLoss and (c.bce_weight, c.dice_weight, c.smooth, c.per_sample) == (0.5, 0.5, 1.0, False)
    assert type(trainer.seg_criterion(ap.parse_args(["--seg-loss", "lovasz"]))) is mnn.LovaszHingeLoss
    assert type(trainer.seg_criterion(ap.parse_args(["--task", "seg", "--seg-classes", "3"]))) is mnn.MultiClassSegLoss
