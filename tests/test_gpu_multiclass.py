"""-m gpu: multi-class segmentation on the device — the softmax cross-entropy + per-class Dice loss and the argmax / confusion pass
(csrc/mcseg.hip) through the C ABI, mi355.nn.MultiClassSegLoss, a K-channel model, train(), the label transform and the tester.

Yardstick: tests/multiclass_ref.py, the fp64 restatement pinned to torch fp64 on the CPU (tests/test_multiclass_cpu.py).  Bounds
(derived, not measured): the kernels evaluate in double and round to float once, so
    |loss_i - ref| <= 2^-23 |ref| + 2^-40,      |dz - ref| <= 2^-23 |ref| + 2^-40 S,
S = |gscale| (ce_weight max w / sum w + dice_weight (max a_c + max b_c) / |S|) from the restatement: one float rounding (2^-24
relative) of a double evaluation whose own error sits many bits below 2^-40 of the coefficients.  Integers are exact."""
import os
import re

import numpy as np
import pytest
import torch

import multiclass_ref as R
from mi355.lib import lib
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGN = 255
ROW = 50                       # MI355_MCSEG_ROW
GUARD = 64
E23, E40 = 2.0 ** -23, 2.0 ** -40


def _chunk():
    """pixels one workgroup walks per trip, read off mi355_mcseg_rows: the largest HW one image still gives to one workgroup"""
    rows = lib.raw("mi355_mcseg_rows")
    lo, hi = 1, 1 << 20
    assert rows(1, lo) == 1 and rows(1, hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if rows(1, mid) == 1 else (lo, mid)
    return lo


def _poisoned(n, dtype, value):
    t = torch.empty(n + GUARD, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(value)
    return t


def _guard_intact(t, n, value):
    return bool((t[n:].view(torch.uint8) == value).all())


def op(z, y, C, weight=None, cw=1.0, dw=0.0, smooth=1.0, ps=False, bg=True, gscale=None, ign=IGN):
    """The C ABI as a caller sees it, outputs in poisoned buffers with a guard region behind them
    -> (loss [3], dz like z, conf [N, C, C], pred [N, HW])."""
    N = z.shape[0]
    HW = z.numel() // (N * C)
    rows = lib.mi355_mcseg_rows(N, HW)
    assert rows >= N
    partial = torch.full((rows * ROW,), float("nan"), dtype=torch.float64, device=DEV)
    state = torch.full((2 + 2 * N * C,), float("nan"), dtype=torch.float64, device=DEV)
    loss = torch.full((3,), float("nan"), dtype=torch.float32, device=DEV)
    w = None if weight is None else torch.tensor(weight, dtype=torch.float32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=DEV)
    lib.mi355_mcseg_loss_fwd(z, y, N, C, HW, w, ign, cw, dw, smooth, int(ps), int(bg), partial, state, loss)
    dz = _poisoned(z.numel(), torch.float32, 0xA5)
    lib.mi355_mcseg_loss_bwd(z, y, N, C, HW, w, ign, cw, dw, state, gs, dz)
    conf = _poisoned(N * C * C, torch.int32, 0x5A)
    pred = _poisoned(N * HW, torch.uint8, 0xEE)
    lib.mi355_mcseg_confusion(z, y, N, C, HW, ign, conf, pred)
    torch.cuda.synchronize()
    assert _guard_intact(dz, z.numel(), 0xA5) and _guard_intact(conf, N * C * C, 0x5A) and _guard_intact(pred, N * HW, 0xEE), "guard bytes"
    return loss, dz[: z.numel()].view(z.shape), conf[: N * C * C].view(N, C, C), pred[: N * HW].view(N, HW)


def _logits(kind, shape, seed):
    g = np.random.default_rng(seed)
    if kind == "normal":
        z = g.normal(0, 3, shape)
    elif kind == "saturated":
        z = np.where(g.random(shape) < 0.5, 80.0, -80.0)
    else:                                            # multiples of 0.5: argmax ties
        z = np.round(g.normal(0, 1, shape) * 2) / 2
    return z.astype(np.float32)


LABELS = ["random", "one class", "class absent", "ignore rows", "all ignored", "out of range"]


def _labels(kind, N, C, H, W, seed):
    g = np.random.default_rng(seed)
    y = g.integers(0, C, (N, H, W))
    if kind == "one class":
        y[:] = C - 1
    elif kind == "class absent":
        y[y == 1] = 0
    elif kind == "ignore rows":
        y.reshape(N, -1)[:, : max(1, (H * W) // 3)] = IGN
    elif kind == "all ignored":
        y[:] = IGN
    elif kind == "out of range":
        hit = g.random((N, H, W)) < 0.3
        y[hit] = g.integers(C, 255, int(hit.sum()))
    return y.astype(np.uint8)


def _weight(C):
    w = [0.5 + 0.25 * c for c in range(C)]
    w[min(2, C - 1)] = 0.0
    return w


CFG = [(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.5, 0.5, 1.0), (0.3, 0.7, 1e-3)]      # (ce_weight, dice_weight, smooth)
GSCALE = [None, 65536.0, 0.37]


def _check(tag, z, y, C, out, weight, cw, dw, smooth, ps, bg, gscale):
    loss, dz, conf, pred = out
    gs = 1.0 if gscale is None else float(np.float32(gscale))
    wq = None if weight is None else np.asarray(weight, dtype=np.float32).astype(np.float64)
    cwq, dwq, smq = float(np.float32(cw)), float(np.float32(dw)), float(np.float32(smooth))
    N = z.shape[0]
    zz = z.reshape(N, C, -1)
    (t, ce, dice), g64 = R.mc_loss(zz, y.reshape(N, -1), wq, cwq, dwq, smq, ps, bg, gs)
    S = R.grad_scale(zz, y.reshape(N, -1), wq, cwq, dwq, smq, ps, bg, gs)
    got = loss.cpu().numpy().astype(np.float64)
    for name, a, b in (("total", got[0], t), ("ce", got[1], ce), ("dice", got[2], dice)):
        assert abs(a - b) <= E23 * abs(b) + E40, (tag, name, a, b, abs(a - b))
    d = dz.cpu().numpy().astype(np.float64).reshape(g64.shape)
    err = np.abs(d - g64) - (E23 * np.abs(g64) + E40 * S)
    assert np.isfinite(d).all() and err.max() <= 0, (tag, "dz", float(err.max()), S)
    valid = (y.reshape(N, 1, -1) < C)
    bits = dz.cpu().view(torch.int32).numpy().reshape(N, C, -1)
    assert not bits[np.broadcast_to(~valid, bits.shape)].any(), (tag, "dz at ignored pixels is not +0")
    if not valid.any():
        assert got[1] == 0.0 and not bits.any(), (tag, "all ignored")
    rconf, rpred = R.confusion(zz, y.reshape(N, -1))
    assert np.array_equal(conf.cpu().numpy(), rconf), (tag, "conf")
    assert np.array_equal(pred.cpu().numpy(), rpred), (tag, "pred")


def _sweep(shape, offset=0):
    N, C, H, W = shape
    k = 0
    for lk in ("normal", "saturated", "ties"):
        z = _logits(lk, shape, 7 + k)
        if offset:                                   # the same logits through a base pointer `offset` floats past an aligned one
            buf = torch.empty(z.size + offset, dtype=torch.float32, device=DEV)
            zd = buf[offset:].view(shape)
            zd.copy_(torch.from_numpy(z))
            assert zd.data_ptr() % 16 == 4 * offset
        else:
            zd = torch.from_numpy(z).to(DEV)
        for yk in LABELS:
            y = _labels(yk, N, C, H, W, 100 + k)
            yd = torch.from_numpy(y).to(DEV)
            for ps in (False, True):
                for bg in (False, True):
                    cw, dw, smooth = CFG[k % 4]
                    gscale = GSCALE[k % 3]
                    weight = _weight(C) if (k // 2) % 2 else None
                    k += 1
                    tag = f"{shape} off={offset} {lk} / {yk} ps={ps} bg={bg} ({cw},{dw},{smooth}) gs={gscale} w={weight is not None}"
                    a = op(zd, yd, C, weight, cw, dw, smooth, ps, bg, gscale)
                    _check(tag, z, y, C, a, weight, cw, dw, smooth, ps, bg, gscale)
                    b = op(zd, yd, C, weight, cw, dw, smooth, ps, bg, gscale)
                    for u, v in zip(a, b):                                  # the same input gives the same bytes
                        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (tag, "not reproducible")
    return k


@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 3, 5, 7), (2, 4, 8, 8), (3, 5, 33, 65), (1, 16, 16, 20)])
def test_kernels_match_the_fp64_restatement(shape):
    assert _sweep(shape) == 72


@pytest.mark.parametrize("which", ["chunk + 1", "2 chunk - 1"])
def test_kernels_at_the_workgroup_chunk_edges(which):
    chunk = _chunk()
    hw = chunk + 1 if which == "chunk + 1" else 2 * chunk - 1
    assert lib.mi355_mcseg_rows(2, hw) == 4
    _sweep((2, 3, 1, hw))


def test_kernels_through_a_base_pointer_four_bytes_off():
    _sweep((2, 4, 8, 8), offset=1)


# ---- module ---------------------------------------------------------------------------------------------------------------------
def test_module_equals_the_abi_and_reports_its_terms():
    from mi355 import nn as mnn
    shape = (3, 5, 33, 65)
    z = _logits("normal", shape, 1)
    y = _labels("ignore rows", 3, 5, 33, 65, 2)
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    w = _weight(5)
    for ps, bg in ((False, True), (True, False)):
        loss, dz, conf, pred = op(zd, yd, 5, w, 0.5, 0.5, 1.0, ps, bg)
        crit = mnn.MultiClassSegLoss(5, 0.5, 0.5, class_weight=w, per_sample=ps, include_background=bg)
        for target in (yd, yd[:, None], yd.long()):                        # [N,H,W], [N,1,H,W], int64 converted once
            a = zd.clone().requires_grad_(True)
            l = crit(a, target)
            assert l.dim() == 0 and l.dtype == torch.float32 and l.is_cuda
            l.backward()
            torch.cuda.synchronize()
            assert torch.equal(l.reshape(1), loss[:1]) and torch.equal(a.grad, dz)
            assert torch.equal(torch.stack(crit.last_terms), loss[1:])
        assert torch.equal(crit.confusion(zd, yd), conf)
        vm = crit.val_metric(zd, yd)
        assert vm.dim() == 0 and vm.is_cuda and abs(float(vm) - R.val_metric(conf.cpu().numpy())) < 1e-6
    ld, dd, _, _ = op(zd, yd, 5, None, 0.0, 1.0, 1.0, False, True)
    a = zd.clone().requires_grad_(True)
    l = mnn.MultiClassDiceLoss(5)(a, yd)
    (3 * l).backward()
    _, d3, _, _ = op(zd, yd, 5, None, 0.0, 1.0, 1.0, False, True, gscale=3.0)
    torch.cuda.synchronize()
    assert torch.equal(l.reshape(1), ld[:1]) and torch.equal(a.grad, d3)


def test_module_raises_the_documented_errors():
    from mi355 import nn as mnn
    z = torch.randn(2, 3, 8, 8, device=DEV)
    y = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    crit = mnn.MultiClassSegLoss(3)
    with pytest.raises(ValueError, match=r"logits \[N, 3, H, W\]"):
        crit(torch.randn(2, 4, 8, 8, device=DEV), y)
    with pytest.raises(ValueError, match="target size"):
        crit(z, y[:1])
    with pytest.raises(ValueError, match="target size"):
        crit(z, torch.zeros(2, 8, 7, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="num_classes must be >= 2"):
        mnn.MultiClassSegLoss(1)
    big = y.long()
    big[0, 0, 0] = 256
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 255\]"):
        crit(z, big)
    with pytest.raises(ValueError, match="class-index labels"):
        crit(z, y.float())
    with pytest.raises(ValueError, match="ignore_index"):
        mnn.MultiClassSegLoss(3, ignore_index=2)


# ---- through a model ------------------------------------------------------------------------------------------------------------
def _labels3(mask):
    """three classes from the closed-form ellipse and a shifted copy of it: 0 outside both, 1 the ellipse, 2 where the copy covers it"""
    m = mask[:, 0] > 0.5
    s = mask.roll(5, dims=3)[:, 0] > 0.5
    lab = torch.zeros(m.shape, dtype=torch.uint8)
    lab[m] = 1
    lab[m & s] = 2
    return lab


def _model3():
    from models.segmentation_models.AttentionUNet import AttentionUNet
    m = AttentionUNet(out_channel=3)
    m.load_state_dict(nets.closed_form_state("AttentionUNet", out_channels=3))
    m.compute_dtype = torch.float32
    return m.to(DEV)


def test_loss_writes_into_the_plan_and_trains_a_three_class_model():
    from mi355 import nn as mnn, optim as moptim
    m = _model3().train()
    x, mask = otrain.closed_form_input(2, 32)
    lab = _labels3(mask)
    assert sorted(lab.unique().tolist()) == [0, 1, 2]
    xd, yd = x.to(DEV), lab.to(DEV)
    crit = mnn.MultiClassSegLoss(3, 0.5, 0.5)
    opt = moptim.AdamW(m.parameters(), lr=1e-3, weight_decay=5e-4)
    losses = []
    for step in range(6):
        opt.zero_grad(set_to_none=True)
        out = m(xd)
        plan = out._mi355_plan
        assert out.shape == (2, 3, 32, 32)
        loss = crit(out, yd)
        loss.backward()
        torch.cuda.synchronize()
        if step == 0:
            n = out.numel()
            z = out.detach().clone()
            _, dz, _, _ = op(z, yd, 3, None, 0.5, 0.5, 1.0, False, True, gscale=1.0)
            assert torch.equal(plan.dout[:n], dz.reshape(-1))                         # the node wrote into the plan's own buffer
            (t, _, _), _ = R.mc_loss(z.cpu().numpy(), lab.numpy(), None, 0.5, 0.5, 1.0, False, True)
            assert abs(float(loss.detach()) - t) <= E23 * abs(t) + E40
            for k, p in m.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        losses.append(float(loss.detach()))
        if step < 5:
            opt.step()
    print("loss over five AdamW steps:", [f"{v:.6f}" for v in losses])
    assert losses[5] < losses[0]


# ---- train(), checkpoint, tester ------------------------------------------------------------------------------------------------------
LOG = r"Ep(\d+): TrainLoss ([\d.]+) \| ValLoss ([\d.]+) \| IoU ([\d.]+)"


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """two epochs of train() on the three-class synthetic set -> (save dir, printed text, validation loader)"""
    import contextlib
    import io
    from torch.utils.data import DataLoader, Subset
    from mi355 import nn as mnn
    from utils import helpers, trainer
    d = str(tmp_path_factory.mktemp("mc"))
    full = trainer.synthetic_dataset("seg", 8, 32, classes=3)
    tr = DataLoader(Subset(full, range(6)), batch_size=2, shuffle=False)
    va = DataLoader(Subset(full, range(6, 8)), batch_size=2, shuffle=False)
    model = helpers.get_seg_model("attentionunet", classes=3)
    model.load_state_dict(nets.closed_form_state("AttentionUNet", out_channels=3))
    model.compute_dtype = torch.float32
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        best = helpers.train(model, tr, va, torch.device(DEV), 2, 1e-3, "AttentionUNet", d, seg=True, criterion=mnn.MultiClassSegLoss(3, 0.5, 0.5))
    return d, buf.getvalue(), va, best


def _reload(d):
    from utils import helpers
    m = helpers.get_seg_model("attentionunet", classes=3)
    m.load_state_dict(torch.load(os.path.join(d, "AttentionUNet_best_loss.pt"), map_location=DEV))
    m.compute_dtype = torch.float32
    return m.to(DEV).eval()


def test_train_logs_saves_and_the_checkpoint_reproduces_its_confusion(trained):
    from utils.multiclass import confusion_batch
    d, text, va, best = trained
    rows = re.findall(LOG, text)
    assert len(rows) == 2, text
    for ep, tl, vl, iou in rows:
        assert 0.0 <= float(iou) <= 1.0 and float(tl) > 0 and float(vl) > 0
    assert abs(best - min(float(r[2]) for r in rows)) < 1e-3
    assert os.path.exists(os.path.join(d, "AttentionUNet_best_loss.pt"))
    x, y = next(iter(va))
    confs = []
    for _ in range(2):                                   # two fresh models from the checkpoint agree with each other
        m = _reload(d)
        with torch.no_grad():
            out = m(x.to(DEV))
        conf, pred = confusion_batch(out, y.to(DEV), return_pred=True)
        assert conf.shape == (2, 3, 3) and conf.dtype == torch.int32 and pred.shape == (2, 32, 32) and pred.dtype == torch.uint8
        rconf, rpred = R.confusion(out.float().cpu().numpy(), y.numpy())
        assert np.array_equal(conf.cpu().numpy(), rconf) and np.array_equal(pred.cpu().numpy(), rpred)
        confs.append(conf)
    assert torch.equal(confs[0], confs[1]) and int(confs[0].sum()) == 2 * 32 * 32


def test_tester_multiclass_evaluation_equals_the_restatement(trained, capsys):
    from utils import tester
    d, _, va, _ = trained
    m = _reload(d)
    r = tester.evaluate_multiclass_segmentation_model(m, va, torch.device(DEV), "AttentionUNet", 3, 255, ["bg", "ring", "core"])
    text = capsys.readouterr().out
    x, y = next(iter(va))
    with torch.no_grad():
        out = m(x.to(DEV)).float().cpu().numpy()
    rconf, _ = R.confusion(out, y.numpy())
    ref = R.metrics(rconf)
    assert r["confusion_matrix"] == rconf.sum(0).tolist() and r["samples"] == 2 and r["class_names"] == ["bg", "ring", "core"]
    assert np.array_equal(np.asarray(r["dice_per_class"]), 100.0 * ref["dice_per_class"], equal_nan=True)
    assert np.array_equal(np.asarray(r["iou_per_class"]), 100.0 * ref["iou_per_class"], equal_nan=True)
    assert r["dice"] == 100.0 * ref["mean_dice"] and r["iou"] == 100.0 * ref["mean_iou"] and r["pixel_accuracy"] == 100.0 * ref["pixel_acc"]
    assert "ring" in text and "Mean IoU" in text


# ---- transform ------------------------------------------------------------------------------------------------------------------
def test_label_transform_keeps_labels_through_the_warps():
    from utils.gpu_transforms import SegBatchTransform
    g = torch.Generator().manual_seed(3)
    n, hs = 4, 48
    images = torch.randint(0, 256, (n, hs, hs, 3), dtype=torch.uint8, generator=g)
    vals = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8)
    masks = vals[torch.randint(0, 5, (n, hs // 4, hs // 4), generator=g)].repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    for elastic in (None, (64.0, 4.0, 1.0)):
        plain = SegBatchTransform(32, train=True, seed=5, device=DEV, elastic=elastic)
        params = plain.draw(n)
        if elastic is not None:
            params = (*params, plain.draw_elastic(n))
        x0, y0 = plain(images, masks, params=params)
        tl = SegBatchTransform(32, train=True, seed=5, device=DEV, elastic=elastic, labels=True)
        x1, y1 = tl(images, masks, params=params)
        assert y1.dtype == torch.uint8 and y1.shape == (n, 32, 32) and torch.equal(x0, x1)
        assert torch.equal(y1, torch.round(y0[:, 0] * 255).to(torch.uint8))          # the mask channel before the / 255
        assert set(y1.unique().tolist()) <= set(vals.tolist())                     # nearest sampling: no label is invented
        x2, y2 = SegBatchTransform(32, train=True, seed=5, device=DEV, elastic=elastic, labels=False)(images, masks, params=params)
        assert torch.equal(x2, x0) and torch.equal(y2, y0) and y2.dtype == torch.float32
    e0 = SegBatchTransform(32, train=False, device=DEV)(images, masks)
    e1 = SegBatchTransform(32, train=False, device=DEV, labels=True)(images, masks)
    assert torch.equal(e0[0], e1[0]) and torch.equal(e1[1], torch.round(e0[1][:, 0] * 255).to(torch.uint8))
