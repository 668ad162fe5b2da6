"""CPU: the multi-class segmentation path without a GPU — tests/multiclass_ref.py (the fp64 restatement the GPU tests measure against)
pinned to torch fp64 (F.cross_entropy, autograd through a one-hot Dice) and to brute-force loops, the four prototypes of
csrc/mcseg.hip in the header, the launchers' argument checks, the trainer's and the tester's flag wiring and formatting."""
import ctypes
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as R
from mi355.lib import available, lib, parse_header

IGN = 255


def _case(seed, N=3, C=4, H=7, W=9, absent=2):
    g = np.random.default_rng(seed)
    z = g.normal(0, 3, (N, C, H, W))
    y = g.integers(0, C, (N, H, W))
    y[y == absent] = (absent + 1) % C            # a class absent from the targets
    y[0, :2] = IGN                               # rows of ignore_index
    y[1, 3, 4] = C + 3                           # an out-of-range label that is not ignore_index
    return z, y


def _torch_loss(z, y, w, cw, dw, smooth, per_sample, include_bg, ign=IGN):
    """torch fp64: F.cross_entropy + a one-hot Dice, gradient by autograd."""
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    C = zt.shape[1]
    yt = torch.tensor(y, dtype=torch.int64)
    yt = torch.where((yt >= 0) & (yt < C), yt, torch.full_like(yt, ign))      # every label >= C is ignored
    wt = None if w is None else torch.tensor(w, dtype=torch.float64)
    ce = F.cross_entropy(zt, yt, weight=wt, ignore_index=ign)
    p = torch.softmax(zt, 1)
    v = (yt != ign)
    oh = F.one_hot(torch.where(v, yt, torch.zeros_like(yt)), C).permute(0, 3, 1, 2).double() * v[:, None]
    pv = p * v[:, None]
    dims = (2, 3) if per_sample else (0, 2, 3)
    I, P, T = (pv * oh).sum(dims), pv.sum(dims), oh.sum(dims)
    dice_c = (2 * I + smooth) / (P + T + smooth)
    sel = dice_c[..., (0 if include_bg else 1):]
    dice = (1 - sel.mean(-1)).mean()
    total = cw * ce + dw * dice
    total.backward()
    return (float(total.detach()), float(ce.detach()), float(dice.detach())), zt.grad.numpy()


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("include_bg", [False, True])
@pytest.mark.parametrize("weight", [None, [0.5, 2.0, 0.0, 1.25]])
def test_restatement_is_torch_fp64(per_sample, include_bg, weight):
    for seed, (cw, dw, smooth) in enumerate([(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.5, 0.5, 1.0), (0.3, 0.7, 1e-3)]):
        z, y = _case(seed)
        (t, ce, dice), dz = R.mc_loss(z, y, weight, cw, dw, smooth, per_sample, include_bg)
        (tt, tce, tdice), tdz = _torch_loss(z, y, weight, cw, dw, smooth, per_sample, include_bg)
        dl, dg = max(abs(t - tt), abs(ce - tce), abs(dice - tdice)), float(np.abs(dz - tdz).max())
        print(f"ps={per_sample} bg={include_bg} w={weight is not None} ({cw},{dw},{smooth}): loss diff {dl:.1e}, grad diff {dg:.1e}")
        assert dl <= 1e-14 and dg <= 1e-15
        assert not np.any(dz[0, :, :2]) and not np.any(dz[1, :, 3, 4])            # ignored pixels: zero gradient


def test_restatement_gscale_and_all_ignored():
    z, y = _case(5)
    _, dz1 = R.mc_loss(z, y, None, 0.5, 0.5)
    _, dzs = R.mc_loss(z, y, None, 0.5, 0.5, gscale=65536.0)
    assert np.array_equal(dzs, dz1 * 65536.0)
    (t, ce, dice), dz = R.mc_loss(z, np.full_like(y, IGN), None, 1.0, 0.0)
    assert ce == 0.0 and t == 0.0 and not dz.any()                                # torch gives NaN here; documented departure
    (t, ce, dice), dz = R.mc_loss(z, np.full_like(y, IGN), None, 0.0, 1.0, smooth=1.0)
    assert dice == 0.0 and not dz.any()                                           # every dice_c = smooth / smooth


def test_argmax_confusion_and_metrics_against_loops():
    g = np.random.default_rng(0)
    N, C, H, W = 3, 4, 6, 5
    z = np.round(g.normal(0, 1, (N, C, H, W)) * 2) / 2                            # multiples of 0.5: ties
    y = g.integers(0, C, (N, H, W))
    y[0][y[0] == 3] = 1                                                           # class 3 absent from image 0's labels ...
    z[0, 3] = -50.0                                                               # ... and from its predictions: NaN for (0, 3)
    z[0, 1, 0, 0] = np.nan                                                        # a NaN never wins
    z[0, :, 0, 1] = np.nan                                                        # all NaN -> class 0
    y[2, 0] = IGN
    y[1, 1, 1] = C
    conf, pred = R.confusion(z, y)
    bconf = np.zeros((N, C, C), dtype=np.int64)
    for n in range(N):
        for i in range(H):
            for j in range(W):
                best, p = -np.inf, 0
                for c in range(C):
                    if z[n, c, i, j] > best:
                        best, p = z[n, c, i, j], c
                assert pred[n, i, j] == p
                if 0 <= y[n, i, j] < C:
                    bconf[n, y[n, i, j], p] += 1
    assert np.array_equal(conf, bconf)
    assert pred[0, 0, 1] == 0 and pred[0, 0, 0] != 1
    assert conf.sum() == N * H * W - W - 1
    m = R.metrics(conf)
    for n in range(N):
        for c in range(C):
            tp, row, col = bconf[n, c, c], bconf[n, c].sum(), bconf[n, :, c].sum()
            if row + col == 0:
                assert np.isnan(m["iou"][n, c]) and np.isnan(m["dice"][n, c])
            else:
                assert m["iou"][n, c] == tp / (row + col - tp) and m["dice"][n, c] == 2 * tp / (row + col)
    assert np.isnan(m["iou"][0, 3]) and not np.isnan(m["iou_per_class"]).any()     # every class is in some image
    assert abs(m["iou_per_class"][3] - np.mean([m["iou"][1, 3], m["iou"][2, 3]])) < 1e-15
    assert abs(m["mean_iou"] - m["iou_per_class"].mean()) < 1e-15
    assert m["pixel_acc"] == np.trace(bconf.sum(0)) / bconf.sum()
    # the host-side function the tester uses is the same statement
    from utils.multiclass import metrics_from_confusion
    mm = metrics_from_confusion(conf)
    for k in ("iou", "dice", "iou_per_class", "dice_per_class"):
        assert np.array_equal(mm[k], m[k], equal_nan=True), k
    assert mm["mean_iou"] == m["mean_iou"] and mm["mean_dice"] == m["mean_dice"] and mm["pixel_accuracy"] == m["pixel_acc"]
    assert np.array_equal(mm["confusion_matrix"], bconf.sum(0))
    # val_metric: classes with a non-zero union of the batch-summed matrix
    c = bconf.sum(0).astype(np.float64)
    ious = [c[k, k] / (c[k].sum() + c[:, k].sum() - c[k, k]) for k in range(C) if c[k].sum() + c[:, k].sum() - c[k, k] > 0]
    assert abs(R.val_metric(conf) - np.mean(ious)) < 1e-15
    assert R.val_metric(np.zeros((2, 3, 3))) == 0.0


def test_header_declares_the_four_launchers():
    protos = parse_header()
    names = {
        "mi355_mcseg_rows": ["N", "HW"],
        "mi355_mcseg_loss_fwd": ["z", "y", "N", "C", "HW", "weight", "ignore_index", "ce_weight", "dice_weight", "smooth", "per_sample",
                                 "include_background", "partial", "state", "loss", "s"],
        "mi355_mcseg_loss_bwd": ["z", "y", "N", "C", "HW", "weight", "ignore_index", "ce_weight", "dice_weight", "state", "gscale", "dz", "s"],
        "mi355_mcseg_confusion": ["z", "y", "N", "C", "HW", "ignore_index", "conf", "pred", "s"],
    }
    for fn, args in names.items():
        assert fn in protos, fn
        assert [a for _, a in protos[fn][1]] == args, fn
        assert protos[fn][0] is ctypes.c_int


def test_launchers_reject_bad_arguments_before_touching_the_device():
    assert available(), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    ERR_ARG = -1
    err = lambda: lib.raw("mi355_last_error")().decode()      # noqa: E731
    p = 1 << 20                                                # a non-null, aligned address that is never dereferenced
    fwd, bwd, conf, rows = (lib.raw(n) for n in ("mi355_mcseg_loss_fwd", "mi355_mcseg_loss_bwd", "mi355_mcseg_confusion", "mi355_mcseg_rows"))

    def f(z=p, y=p, N=2, C=3, HW=64, ign=255, cw=1.0, dw=0.5, sm=1.0, partial=p, state=p, loss=p):
        return fwd(z, y, N, C, HW, None, ign, cw, dw, sm, 0, 1, partial, state, loss, None)

    def b(z=p, y=p, N=2, C=3, HW=64, ign=255, state=p, dz=p):
        return bwd(z, y, N, C, HW, None, ign, 1.0, 0.5, state, None, dz, None)

    def c(z=p, y=p, N=2, C=3, HW=64, ign=255, conf_=p):
        return conf(z, y, N, C, HW, ign, conf_, None, None)

    for call in (f, b, c):
        for kw, word in (({"z": None}, "null"), ({"y": None}, "null"), ({"C": 1}, "C"), ({"C": 17}, "C"), ({"ign": 0}, "ignore_index"),
                         ({"ign": 2}, "ignore_index"), ({"ign": 256}, "ignore_index"), ({"HW": -5}, "HW"), ({"HW": 0}, "HW"),
                         ({"N": 0}, "N")):
            rc = call(**kw)
            assert rc == ERR_ARG and word in err(), (call.__name__, kw, rc, err())
    for kw in ({"partial": None}, {"state": None}, {"loss": None}, {"cw": -1.0}, {"sm": -1.0}):
        assert f(**kw) == ERR_ARG, kw
    assert b(state=None) == ERR_ARG and b(dz=None) == ERR_ARG and c(conf_=None) == ERR_ARG
    assert rows(0, 64) == -1 and "N" in err()
    assert rows(2, -1) == -1 and rows(2, (1 << 30) + 1) == -1
    # rows: a function of (N, HW); the chunk is where one image's workgroup count steps from 1 to 2
    assert rows(1, 1) == 1 and rows(3, 1) == 3
    chunk = max(hw for hw in (256, 512, 1024, 2048, 4096) if rows(1, hw) == 1)
    assert rows(1, chunk + 1) == 2 and rows(2, 2 * chunk - 1) == 4 and rows(2, 2 * chunk + 1) == 6
    assert rows(65535, 1 << 20) == 65535


def _args(*argv):
    from utils import trainer
    return trainer.build_parser().parse_args(list(argv))


def test_trainer_flags_and_criterion_wiring():
    from mi355 import nn as mnn
    from utils import trainer
    a = _args()
    assert a.seg_classes == 1 and trainer.multiclass_arg(a) is None and trainer.seg_criterion(a) is None
    assert isinstance(trainer.seg_criterion(_args("--seg-classes", "1", "--seg-loss", "dice")), mnn.DiceLoss)
    crit = trainer.seg_criterion(_args("--seg-classes", "3", "--seg-ce-weight", "0.5", "--seg-dice-weight", "0.5", "--seg-class-weight",
                                       "1,2,0", "--seg-ignore-index", "254", "--dice-per-sample"))
    assert isinstance(crit, mnn.MultiClassSegLoss) and hasattr(crit, "val_metric")
    assert (crit.num_classes, crit.ce_weight, crit.dice_weight, crit.ignore_index, crit.per_sample) == (3, 0.5, 0.5, 254, True)
    assert crit.class_weight.tolist() == [1.0, 2.0, 0.0]
    for bad, word in ((("--seg-loss", "lovasz"), "--seg-loss lovasz"), (("--boundary-weight", "0.1"), "--boundary-weight"),
                      (("--lovasz-weight", "0.5"), "--lovasz-weight"), (("--cutmix-alpha", "1.0"), "--cutmix-alpha"),
                      (("--calibrate",), "--calibrate")):
        with pytest.raises(ValueError, match="binary segmentation") as e:
            trainer.seg_criterion(_args("--seg-classes", "3", *bad))
        assert word in str(e.value)
    for bad in (("--seg-classes", "17"), ("--seg-classes", "0"), ("--seg-classes", "3", "--seg-class-weight", "1,2"),
                ("--seg-classes", "3", "--seg-class-weight", "1,-2,1"), ("--seg-classes", "3", "--seg-ignore-index", "2"),
                ("--seg-classes", "3", "--task", "cls"), ("--seg-classes", "3", "--seg-ce-weight", "-1")):
        with pytest.raises(ValueError):
            trainer.multiclass_arg(_args(*bad))
    with pytest.raises(ValueError, match="num_classes"):
        mnn.MultiClassSegLoss(1)
    d = mnn.MultiClassDiceLoss(4, include_background=False)
    assert (d.ce_weight, d.dice_weight, d.include_background) == (0.0, 1.0, False)


def test_synthetic_dataset_binary_unchanged_and_multiclass_labels():
    from utils import trainer
    x, m = trainer.synthetic_dataset("seg", 8, 32).tensors
    # the binary set as it has always been built
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(8, 3, 32, 32, generator=g)
    yy, xx = torch.meshgrid(torch.arange(32, dtype=torch.float32), torch.arange(32, dtype=torch.float32), indexing="ij")
    c = torch.rand(8, 4, generator=g)
    cy, cx = (0.4 + 0.2 * c[:, 0]) * 32, (0.4 + 0.2 * c[:, 1]) * 32
    ry, rx = (0.25 + 0.1 * c[:, 2]) * 32, (0.25 + 0.1 * c[:, 3]) * 32
    m0 = ((((yy[None] - cy[:, None, None]) / ry[:, None, None]) ** 2 + ((xx[None] - cx[:, None, None]) / rx[:, None, None]) ** 2) <= 1).float()
    assert torch.equal(m, m0[:, None]) and torch.equal(x, x0 + m0[:, None] * torch.tensor([1.0, -0.7, 0.4]).view(1, 3, 1, 1))
    x1, m1 = trainer.synthetic_dataset("seg", 8, 32, classes=1).tensors
    assert torch.equal(x1, x) and torch.equal(m1, m) and m1.dtype == torch.float32
    x3, l3 = trainer.synthetic_dataset("seg", 8, 32, classes=3).tensors
    assert l3.dtype == torch.uint8 and l3.shape == (8, 32, 32) and x3.shape == x.shape
    assert sorted(l3.unique().tolist()) == [0, 1, 2]
    assert all(sorted(l3[i].unique().tolist()) == [0, 1, 2] for i in range(8))     # every image holds every class
    assert torch.equal(l3 > 0, m0 > 0)                                            # the foreground is the binary ellipse
    assert torch.equal(x3[:, :, 0, 0], x0[:, :, 0, 0])                            # background pixels are not tinted
    with pytest.raises(ValueError):
        trainer.synthetic_dataset("cls", 8, 32, classes=3)


def test_get_seg_model_passes_the_class_count():
    from utils.helpers import get_seg_model
    a1, a3 = get_seg_model("attentionunet"), get_seg_model("attentionunet", classes=3)
    n1, n3 = sum(p.numel() for p in a1.parameters()), sum(p.numel() for p in a3.parameters())
    assert n3 > n1
    with pytest.raises(ValueError):
        get_seg_model("attentionunet", classes=0)


def test_tester_flags_summary_and_csv_row():
    from utils import tester
    conf = np.array([[[50, 2, 0], [3, 20, 1], [0, 4, 10]], [[40, 0, 5], [1, 30, 0], [2, 0, 12]]])
    from utils.multiclass import check_class_names, metrics_from_confusion
    names = check_class_names("background, lung,heart", 3)
    assert names == ["background", "lung", "heart"] and check_class_names(None, 2) == ["class0", "class1"]
    with pytest.raises(ValueError):
        check_class_names("a,b", 3)
    r = tester.multiclass_result(metrics_from_confusion(conf), names, 2)
    ref = R.metrics(conf)
    assert abs(r["dice"] - 100 * ref["mean_dice"]) < 1e-12 and abs(r["iou"] - 100 * ref["mean_iou"]) < 1e-12
    assert np.allclose(r["dice_per_class"], 100 * ref["dice_per_class"], rtol=0, atol=1e-12)
    assert r["confusion_matrix"] == conf.sum(0).tolist() and r["samples"] == 2 and r["num_classes"] == 3
    lines = tester.multiclass_summary_lines({"AttentionUNet": r}, ["AttentionUNet"])
    text = "\n".join(lines)
    assert "MULTI-CLASS" in text and f"{r['iou']:>8.2f}%" in text and "lung" in text and "heart" in text
    assert f"{r['dice_per_class'][2]:>8.2f}%" in text
    assert tester.multiclass_summary_lines({}, []) == []
    # print_summary: the multi-class table only when such a result is present; a binary result prints as before
    import contextlib
    binary = {"iou": 80.0, "dice": 88.0, "pixel_accuracy": 97.0, "precision": 90.0, "recall": 86.0, "f1": 88.0}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tester.print_summary({"R2Unet": binary})
    assert "MULTI-CLASS" not in buf.getvalue() and "SEGMENTATION MODELS:" in buf.getvalue()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tester.print_summary({"AttentionUNet": r})
    assert "MULTI-CLASS" in buf.getvalue() and "SEGMENTATION MODELS:" not in buf.getvalue()
    row = tester._csv_row("AttentionUNet", r)
    assert row["Model"] == "AttentionUNet" and row["dice_lung"] == r["dice_per_class"][1] and row["iou_heart"] == r["iou_per_class"][2]
    assert "confusion_matrix" not in row and "class_names" not in row and "dice_per_class" not in row
    assert all(np.isscalar(v) for v in row.values())
    assert tester._csv_row("R2Unet", binary) == {"Model": "R2Unet", **binary}
    # flags
    p = tester.build_parser()
    a = p.parse_args([])
    assert a.seg_classes == 1 and tester.multiclass_kwargs(a) == {}
    kw = tester.multiclass_kwargs(p.parse_args(["--seg-classes", "3", "--class-names", "bg,lung,heart", "--seg-ignore-index", "250"]))
    assert kw == {"seg_classes": 3, "seg_ignore_index": 250, "class_names": ["bg", "lung", "heart"]}
    for bad in (["--surface"], ["--tta", "hflip"], ["--sw-tile", "128"], ["--auc"], ["--ci", "100"], ["--calibration", "d"]):
        with pytest.raises(ValueError, match="binary") as e:
            tester.multiclass_kwargs(p.parse_args(["--seg-classes", "3"] + bad))
        assert bad[0] in str(e.value)
        assert tester.multiclass_kwargs(p.parse_args(bad)) == {}
