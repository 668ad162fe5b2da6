"""CPU: the numpy restatement tests/mix_ref.py pinned to torch and to hand-derived facts, the host side of utils/mix.py (draws, box
geometry, validation), the trainer's flags, and what the built library says about the two new entry points without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mix_ref as R
from mi355 import lib as L

BUILT = pytest.mark.skipif(not os.path.exists(L.SO_PATH), reason="libmi355conv.so not built (run __graft_entry__.build())")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _ce_case(B, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 3, (B, C))
    ya, yb = rng.integers(0, C, B), rng.integers(0, C, B)
    lam = rng.random(B)
    lam[0] = 1.0
    w = 0.5 + rng.random(C)
    return z, ya, yb, lam, w


@pytest.mark.parametrize("B,C", [(1, 3), (5, 3), (257, 7)])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sm", [0.0, 0.1])
def test_ce_mix_ref_is_torch_cross_entropy_with_probability_targets(B, C, weighted, sm):
    z, ya, yb, lam, w = _ce_case(B, C, 7 * B + C)
    w = w if weighted else None
    gscale = 3.0
    loss, dz = R.ce_mix_ref(z, ya, yb, lam, w, sm, gscale)
    cls = np.arange(C)[None, :]
    prob = lam[:, None] * (cls == ya[:, None]) + (1 - lam[:, None]) * (cls == yb[:, None])         # torch smooths it itself
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    want = F.cross_entropy(zt, torch.tensor(prob, dtype=torch.float64), weight=None if w is None else torch.tensor(w, dtype=torch.float64),
                           label_smoothing=sm)
    (want * gscale).backward()
    assert abs(loss - float(want.detach())) <= 1e-12
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12
    assert np.abs(R.soft_targets(ya, yb, lam, C, sm).sum(1) - 1).max() <= 1e-15


@pytest.mark.parametrize("B,C", [(1, 3), (5, 3), (257, 7)])
def test_ce_mix_ref_with_hard_labels_is_the_ce_smooth_formula(B, C):
    z, ya, _, _, _ = _ce_case(B, C, 11 * B + C)
    for sm in (0.0, 0.1):
        loss, dz = R.ce_mix_ref(z, ya, None, None, None, sm)
        l2, d2 = R.ce_smooth_formula(z, ya, sm)
        assert abs(loss - l2) <= 1e-12 and np.abs(dz - d2).max() <= 1e-12
        same = R.ce_mix_ref(z, ya, ya[::-1].copy(), np.ones(B), None, sm)                        # lam = 1: the partner's label has no say
        assert abs(same[0] - loss) <= 1e-15 and np.abs(same[1] - dz).max() <= 1e-15


def test_weighted_hard_labels_differ_from_torchs_class_index_normalisation():
    """the difference the header states: class-index targets with a weight are divided by the sum of the picked weights in torch, by B
    here"""
    z, ya, _, _, w = _ce_case(5, 3, 3)
    loss, _ = R.ce_mix_ref(z, ya, None, None, w, 0.0)
    t = F.cross_entropy(torch.tensor(z), torch.tensor(ya), weight=torch.tensor(w))
    assert abs(loss - float(t) * w[ya].sum() / 5) <= 1e-12 and abs(loss - float(t)) > 1e-3


def _x(shape, seed=0):
    return np.random.default_rng(seed).normal(0, 1, shape).astype(np.float32)


def test_mix_batch_ref_hand_derived_facts():
    x = _x((3, 2, 5, 7))
    perm = np.array([1, 2, 0])
    empty = np.zeros((3, 4), np.int64)
    ident = R.mix_batch_ref(x, perm, np.ones(3, np.float32), empty)
    assert np.array_equal(ident.view(np.int32), x.view(np.int32))                                # lam = 1, empty box: the identity
    full = R.mix_batch_ref(x, perm, np.full(3, 0.3, np.float32), np.tile([0, 0, 5, 7], (3, 1)))
    assert np.array_equal(full.view(np.int32), x[perm].view(np.int32))                           # a full box: the partner
    one = R.mix_batch_ref(x, perm, np.ones(3, np.float32), np.tile([2, 3, 3, 4], (3, 1)))
    diff = one != x
    assert diff.sum() == 3 * 2 and diff[:, :, 2, 3].all() and np.array_equal(one[:, :, 2, 3], x[perm][:, :, 2, 3])
    half = R.mix_batch_ref(x, perm, np.full(3, 0.5, np.float32), empty)                          # lam = 1/2: products are exact
    assert np.array_equal(half, (x.astype(np.float64) / 2 + x[perm].astype(np.float64) / 2).astype(np.float32))
    quarter = R.mix_batch_ref(x, perm, np.full(3, 0.3, np.float32), empty)                       # every operation rounded on its own
    l = np.float32(0.3)
    want = (l * x).astype(np.float32) + ((np.float32(1) - l) * x[perm]).astype(np.float32)
    assert np.array_equal(quarter.view(np.int32), want.view(np.int32))
    assert np.array_equal(R.mix_batch_ref(x, np.arange(3), np.full(3, 0.0, np.float32), empty), x + np.float32(0) * x)


# ---- draws --------------------------------------------------------------------------------------------------------------------------
def test_cutmix_box_geometry_and_clipping():
    from utils.mix import cutmix_box
    assert cutmix_box(8, 8, 0.75, 4, 4) == (2, 2, 6, 6) == R.cutmix_box_ref(8, 8, 0.75, 4, 4)[0]            # r = 1/2: a 4 x 4 box
    assert cutmix_box(8, 12, 0.75, 0, 11) == (0, 8, 2, 12)                                                # cy = 0 and cx = w - 1 clip
    assert R.cutmix_box_ref(8, 12, 0.75, 0, 11) == ((0, 8, 2, 12), 1 - 8 / 96)
    assert cutmix_box(8, 8, 1.0, 3, 3) == (3, 3, 3, 3) and cutmix_box(8, 8, 0.0, 7, 0) == (3, 0, 8, 4)
    rng = np.random.default_rng(0)
    for _ in range(200):
        h, w, lam0 = int(rng.integers(1, 40)), int(rng.integers(1, 40)), float(rng.random())
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        y0, x0, y1, x1 = b = cutmix_box(h, w, lam0, cy, cx)
        assert b == R.cutmix_box_ref(h, w, lam0, cy, cx)[0] and 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w


def test_cutmix_draw_adjusts_lam_to_the_exact_area_ratio():
    from utils.mix import BatchMix, kernel_lam
    m = BatchMix(cutmix_alpha=1.0, seed=5, per_sample=True)
    seen = 0
    for _ in range(20):
        perm, lam, boxes = m.draw(6, 16, 12)
        assert sorted(perm.tolist()) == list(range(6)) and lam.dtype == np.float32 and boxes.shape == (6, 4)
        for l, (y0, x0, y1, x1) in zip(lam, boxes):
            assert 0 <= y0 <= y1 <= 16 and 0 <= x0 <= x1 <= 12
            assert l == np.float32(1.0 - (y1 - y0) * (x1 - x0) / (16 * 12))
            seen += (y1 - y0) * (x1 - x0) > 0
        assert np.array_equal(kernel_lam(lam, boxes), np.ones(6, np.float32))
    assert seen > 60


def test_mixup_draw_has_empty_boxes_and_batch_draws_share_one_lam():
    from utils.mix import BatchMix, kernel_lam
    perm, lam, boxes = BatchMix(mixup_alpha=0.4, seed=1).draw(8, 16, 16)
    assert not boxes.any() and len(set(lam.tolist())) == 1 and 0 < lam[0] < 1 and np.array_equal(kernel_lam(lam, boxes), lam)
    assert sorted(perm.tolist()) == list(range(8))
    _, lam, _ = BatchMix(mixup_alpha=0.4, seed=1, per_sample=True).draw(8, 16, 16)
    assert len(set(lam.tolist())) == 8
    both = BatchMix(mixup_alpha=0.4, cutmix_alpha=1.0, seed=2, per_sample=True)
    _, lam, boxes = both.draw(64, 16, 16)
    cut = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
    assert 10 < cut.sum() < 54                                                                   # switch_p = 0.5: both schemes occur
    assert BatchMix(mixup_alpha=0.4, cutmix_alpha=1.0, switch_p=0.0, seed=2).draw(4, 16, 16)[2].any() == False  # noqa: E712


def test_p_zero_is_the_identity_and_the_same_seed_gives_the_same_draws():
    from utils.mix import BatchMix
    for per_sample in (False, True):
        perm, lam, boxes = BatchMix(mixup_alpha=0.2, cutmix_alpha=1.0, p=0.0, per_sample=per_sample).draw(5, 8, 8)
        assert perm.tolist() == [0, 1, 2, 3, 4] and (lam == 1).all() and not boxes.any()
    a, b, c = (BatchMix(mixup_alpha=0.2, cutmix_alpha=1.0, seed=s, per_sample=True) for s in (3, 3, 4))
    da, db, dc = ([m.draw(6, 32, 32) for _ in range(4)] for m in (a, b, c))
    assert all(np.array_equal(u, v) for x, y in zip(da, db) for u, v in zip(x, y))
    assert not all(np.array_equal(u, v) for x, y in zip(da, dc) for u, v in zip(x, y))
    part = BatchMix(cutmix_alpha=1.0, p=0.5, per_sample=True, seed=0).draw(64, 8, 8)
    off = part[0] == np.arange(64)
    assert 10 < off.sum() < 54 and (part[1][off] == 1).all() and not part[2][off].any()


def test_batchmix_leaves_torchs_global_generator_alone():
    from utils.mix import BatchMix
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    m = BatchMix(mixup_alpha=0.2, cutmix_alpha=1.0, per_sample=True, seed=9)
    for _ in range(3):
        m.draw(8, 16, 16)
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, dtype=torch.int64)
    assert m(x, y)[0] is x and m(x, y)[1] is y                                                   # N = 1: the inputs, nothing launched
    off = BatchMix()
    x8, y8 = torch.zeros(8, 3, 4, 4), torch.zeros(8, dtype=torch.int64)
    assert off(x8, y8)[0] is x8 and off(x8, y8)[1] is y8                                         # both alphas 0
    assert torch.equal(torch.get_rng_state(), before)


def test_bad_arguments():
    from utils.mix import BatchMix, MixedTarget, mix_batch
    with pytest.raises(ValueError, match="segmentation"):
        BatchMix(mixup_alpha=0.2, seg=True)
    BatchMix(cutmix_alpha=1.0, seg=True)
    for kw in ({"mixup_alpha": -1}, {"cutmix_alpha": float("nan")}, {"p": 1.5}, {"switch_p": -0.1}):
        with pytest.raises(ValueError):
            BatchMix(**kw)
    with pytest.raises(ValueError, match="GPU"):
        mix_batch(torch.zeros(2, 1, 4, 4), [0, 1], [1, 1], np.zeros((2, 4), int))
    t = MixedTarget(torch.tensor([0, 1, 2]), torch.tensor([2, 2, 0]), torch.tensor([0.5, 0.25, 1.0]))
    assert t.hard.tolist() == [0, 2, 2] and len(t) == 3 and t.size(0) == 3 and t.to("cpu").lam.dtype == torch.float32
    with pytest.raises(ValueError):
        MixedTarget(torch.zeros(3), torch.zeros(2), torch.zeros(3))


def test_mix_cross_entropy_checks_host_labels():
    from mi355 import nn as mnn
    crit = mnn.MixCrossEntropyLoss(0.1, weight=[1.0, 2.0, 0.5])
    assert crit.weight.dtype == torch.float32 and crit.accepts_mixed_target and "weight" in dict(crit.named_buffers())
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        crit(torch.zeros(2, 3), torch.tensor([0, 3]))
    with pytest.raises(ValueError):
        mnn.MixCrossEntropyLoss(weight=[1.0, -1.0])
    assert not getattr(mnn.CrossEntropyLoss(), "accepts_mixed_target", False)


# ---- parser ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_flags_and_mix_arg():
    from utils import trainer
    from utils.mix import BatchMix
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert (d.mixup_alpha, d.cutmix_alpha, d.mix_prob, d.mix_switch_prob, d.mix_per_sample, d.class_weight) == (0.0, 0.0, 1.0, 0.5, False, "none")
    assert trainer.mix_arg(d, "cls", 0) is None and trainer.mix_arg(d, "seg", 0) is None
    a = ap.parse_args("--task cls --mixup-alpha 0.2 --cutmix-alpha 1.0 --mix-prob 0.7 --mix-switch-prob 0.3 --mix-per-sample --class-weight balanced".split())
    m0, m1 = trainer.mix_arg(a, "cls", 0), trainer.mix_arg(a, "cls", 1)
    assert isinstance(m0, BatchMix) and not m0.seg and (m0.mixup_alpha, m0.cutmix_alpha, m0.p, m0.switch_p, m0.per_sample) == (0.2, 1.0, 0.7, 0.3, True)
    assert (m0.seed, m1.seed) == (0, 1)
    assert not all(np.array_equal(u, v) for u, v in zip(m0.draw(8, 16, 16), m1.draw(8, 16, 16)))       # ranks draw different mixes
    s = trainer.mix_arg(ap.parse_args("--task seg --cutmix-alpha 1.0".split()), "seg", 0)
    assert s.seg and s.mixup_alpha == 0
    for bad, task in (("--task seg --mixup-alpha 0.2", "seg"), ("--task both --mixup-alpha 0.2", "seg"), ("--mixup-alpha -1", "cls"),
                      ("--cutmix-alpha -0.5", "seg"), ("--cutmix-alpha 1 --mix-prob 2", "cls"), ("--cutmix-alpha 1 --mix-switch-prob -1", "cls")):
        with pytest.raises(ValueError):
            trainer.mix_arg(ap.parse_args(bad.split()), task, 0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--class-weight", "sqrt"])
    assert trainer.balanced_class_weights([0, 0, 0, 1, 2, 2], 3) == [6 / 9, 6 / 3, 6 / 6]
    said = []
    assert trainer.cls_criterion(a, m0, None, None, said.append) is None and "synthetic" in said[0]

    class Files:
        samples = [("a.png", 0), ("b.png", 0), ("c.png", 1), ("d.png", 2), ("e.png", 2), ("f.png", 0)]

    crit = trainer.cls_criterion(a, m0, Files(), [0, 1, 2, 3], said.append)                      # the training indices alone
    assert type(crit).__name__ == "MixCrossEntropyLoss" and crit.label_smoothing == 0.1
    assert crit.weight.tolist() == pytest.approx([4 / 6, 4 / 3, 4 / 3]) and "balanced" in said[1]
    assert trainer.cls_criterion(d, None, Files(), None, said.append) is None and len(said) == 2


def test_train_rejects_a_criterion_that_cannot_take_a_mixed_target():
    """the mixer reaches train() on the training loader (MixedBatches): train()'s parameter list is the one test_seg_loss_cpu.py pins"""
    from mi355 import nn as mnn
    from utils import helpers
    from utils.mix import BatchMix, MixedBatches
    model = torch.nn.Linear(2, 3)
    with pytest.raises(TypeError, match="MixedTarget"):
        helpers.train(model, MixedBatches([], BatchMix(0.2)), [], "cpu", 1, 1e-3, "m", "unused", seg=False, criterion=mnn.CrossEntropyLoss(0.1))
    with pytest.raises(ValueError, match="seg="):
        helpers.train(model, MixedBatches([], BatchMix(cutmix_alpha=1.0)), [], "cpu", 1, 1e-3, "m", "unused", seg=True)
    with pytest.raises(TypeError, match="BatchMix"):
        MixedBatches([], 0.2)


def test_mixed_batches_is_the_loader_with_its_mixer():
    from torch.utils.data import DataLoader, TensorDataset
    from utils.mix import BatchMix, MixedBatches
    dl = DataLoader(TensorDataset(torch.arange(24.0).view(6, 1, 2, 2), torch.arange(6)), batch_size=4)
    plain = MixedBatches(dl)                                                                     # no mixer: the loader's batches
    assert len(plain) == 2 and plain.dataset is dl.dataset and plain.loader is dl and plain.batch_mix is None
    for (x, y), (xw, yw) in zip(dl, plain):
        assert torch.equal(x, xw) and torch.equal(y, yw)
    off = MixedBatches(dl, BatchMix())                                                           # both alphas 0: launches nothing
    assert [y.tolist() for _, y in off] == [[0, 1, 2, 3], [4, 5]]


# ---- the library, without a GPU -------------------------------------------------------------------------------------------------------
@BUILT
def test_library_exports_both_symbols_and_the_plan_table_knows_them():
    protos = L.parse_header()
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name, n in (("mi355_mix_batch_f32", 10), ("mi355_ce_mix", 12)):
        assert name in protos and len(protos[name][1]) == n and protos[name][1][-1][1] == "s"
        assert hasattr(dll, name) and arity(name.encode()) == n


@BUILT
def test_mix_batch_rejects_bad_calls_before_touching_the_device():
    """null pointer, N = 0, out == x, a partial overlap: all refused from the arguments alone (the addresses are never dereferenced)"""
    L.lib.load()
    fn, err = L.lib.raw("mi355_mix_batch_f32"), L.lib.raw("mi355_last_error")
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    x, out, aux = base, base + 4 * 2048, base + 4 * 1024          # 2 x 1 x 4 x 4 = 32 floats per tensor: far apart
    ok_args = lambda **kw: [kw.get("x", x), kw.get("perm", aux), kw.get("lam", aux), kw.get("box", aux), kw.get("out", out),
                            kw.get("N", 2), 1, 4, 4, None]
    for kw, what in (({"x": None}, b"null"), ({"perm": None}, b"null"), ({"lam": None}, b"null"), ({"box": None}, b"null"),
                     ({"out": None}, b"null"), ({"N": 0}, b"sizes"), ({"N": -3}, b"sizes"), ({"out": x}, b"overlap"),
                     ({"out": x + 4 * 31}, b"overlap"), ({"out": x - 4 * 31}, b"overlap"), ({"out": x + 4}, b"overlap")):
        assert fn(*ok_args(**kw)) == -1, kw
        assert what in err(), (kw, err())
    assert fn(x, aux, aux, aux, out, 2, 0, 4, 4, None) == -1 and fn(x, aux, aux, aux, out, 2, 1, 4, 0, None) == -1
    assert fn(x, aux, aux, aux, out, 70000, 1, 4, 4, None) == -1
    ce = L.lib.raw("mi355_ce_mix")
    assert ce(None, aux, None, None, None, out, None, None, 2, 3, 0.1, None) == -1
    assert ce(x, aux, aux, None, None, out, None, None, 2, 3, 0.1, None) == -1 and b"together" in err()
    assert ce(x, aux, None, None, None, out, None, None, 0, 3, 0.1, None) == -1
