"""-m gpu: mixup / CutMix (csrc/mix.hip, utils/mix.py), the mixed-target cross-entropy (mi355_ce_mix, mi355.nn.MixCrossEntropyLoss) and
``utils.mix.MixedBatches`` through utils/helpers.py::train against the numpy restatement tests/mix_ref.py, which tests/test_mix_cpu.py pins
to torch's fp64 cross_entropy and to hand-derived facts.

The mixing kernel is + and * alone, every operation rounded on its own: it is compared byte for byte.

mi355_ce_mix evaluates everything in double and rounds to float32 once on store, so against the float64 restatement fed the same
float32 inputs (``smoothing`` and ``gscale`` included) a value may be off by
  - the one rounding to float32: at most u |v| = 2^-24 |v| for the double value v the kernel holds;
  - what the double arithmetic itself differs by (another summation order over the rows and classes, the device's exp and log at a
    few ulp of double, arguments of up to 60 in magnitude): below 1e-13 relative to the terms, which are at most 1024 * max weight
    here, and this can also move v across a float32 rounding boundary, i.e. cost one more u |ref|;
hence |got - ref| <= 2^-23 |ref| + 1e-12 for the loss and for every element of dz (mix_ref.ce_bound).

Every call through the ABI writes into buffers pre-filled with a sentinel between guard bands and is checked for intact guards, an
unchanged source and two bit-identical runs (the harness of tests/test_gpu_tta.py)."""
import functools
import re

import numpy as np
import pytest
import torch

import mix_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A


class Guarded:
    """``count`` elements of ``dtype`` filled with sentinel bytes between two guard bands; ``shift``: the view starts that many bytes
    off a 16-byte boundary"""

    def __init__(self, count, dtype=torch.float32, shift=0, fill=SENTINEL):
        self.nbytes = count * torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((self.nbytes + 2 * GUARD + shift,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + shift
        self.whole[self.lo:self.lo + self.nbytes] = fill
        self.t = self.whole[self.lo:self.lo + self.nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == shift % 16

    def intact(self):
        return bool((self.whole[:self.lo] == GUARD_BYTE).all()) and bool((self.whole[self.lo + self.nbytes:] == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.t.view(torch.uint8) == SENTINEL).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)


def _src(arr, dtype=torch.float32, shift=0):
    arr = np.array(arr)                                  # (a writable copy: torch.from_numpy wants one)
    g = Guarded(arr.size, dtype, shift)
    g.t.copy_(torch.from_numpy(arr).reshape(-1))
    return g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- mi355_mix_batch_f32 ---------------------------------------------------------------------------------------------------------
PERMS = {2: [1, 0], 3: [0, 2, 1], 4: [3, 2, 1, 0]}          # N = 3: a fixed point and a 2-cycle
LAMS = [0.0, 0.25, 0.3, 1.0]


def _boxes(kind, N, H, W):
    """one box per sample of the named kind; 'mixed' gives every sample another kind"""
    one = {"empty": (0, 0, 0, 0), "empty_row": (2, 1, 2, W), "full": (0, 0, H, W), "pixel": (H // 2, W // 2, H // 2 + 1, W // 2 + 1),
           "to_col_W": (1, W - 3, H - 1, W), "x0_1_x1_3": (0, 1, H, 3 if W < 7 else 7), "first_px": (0, 0, 1, 1)}
    if kind == "mixed":
        order = ["x0_1_x1_3", "empty", "to_col_W", "pixel"]
        return np.array([one[order[n % 4]] for n in range(N)], np.int32)
    return np.tile(np.array(one[kind], np.int32), (N, 1))


BOX_KINDS = ["empty", "empty_row", "full", "pixel", "to_col_W", "x0_1_x1_3", "first_px", "mixed"]


def _gpu_mix(x, perm, lam, boxes, shift=0, runs=2, dshift=None):
    """``shift`` / ``dshift``: bytes the source / the destination (default: like the source) start off a 16-byte boundary"""
    from mi355.lib import lib
    dshift = shift if dshift is None else dshift
    N, C, H, W = x.shape
    src = _src(x, shift=shift)
    pd, ld, bd = (_src(np.asarray(a, t), d) for a, t, d in ((perm, np.int32, torch.int32), (lam, np.float32, torch.float32),
                                                           (boxes, np.int32, torch.int32)))
    outs = []
    for _ in range(runs):
        dst = Guarded(x.size, torch.float32, dshift)
        lib.mi355_mix_batch_f32(src.t, pd.t, ld.t, bd.t, dst.t, N, C, H, W)
        torch.cuda.synchronize()
        assert dst.intact()
        outs.append(dst.numpy(x.shape))
    for o in outs[1:]:
        assert np.array_equal(_bits(o), _bits(outs[0]))
    assert src.intact() and np.array_equal(_bits(src.numpy(x.shape)), _bits(x))
    assert all(g.intact() for g in (pd, ld, bd)) and np.array_equal(pd.numpy(-1), np.asarray(perm, np.int32))
    return outs[0]


@pytest.mark.parametrize("shape,shift,dshift", [((3, 3, 5, 7), 0, 0), ((4, 1, 8, 8), 0, 0), ((2, 3, 16, 12), 0, 0), ((2, 3, 16, 12), 4, 4),
                                                ((2, 3, 16, 12), 4, 0), ((4, 1, 8, 8), 0, 8), ((3, 3, 5, 7), 4, 4), ((3, 3, 37, 41), 0, 0)])
def test_mix_batch_is_the_restatement_byte_for_byte(shape, shift, dshift):
    """scalar path (W = 7, 41; several workgroups per sample at 37 x 41), vector path (W = 8, 12), and W % 4 == 0 with source
    or destination (or both) off a 16-byte boundary, where the vector path must not be taken; every box kind (both parities of a float4:
    x0 % 4 = 1, x1 % 4 = 3, a box ending at column W, a single pixel, empty, full), lam in {0, 0.25, 0.3, 1} rotated over the samples"""
    N, C, H, W = shape
    x = np.random.default_rng(sum(shape)).normal(0, 1, shape).astype(np.float32)
    perm = PERMS[N]
    for k, kind in enumerate(BOX_KINDS):
        boxes = _boxes(kind, N, H, W)
        lam = np.array([LAMS[(n + k) % 4] for n in range(N)], np.float32)
        want = R.mix_batch_ref(x, perm, lam, boxes)
        got = _gpu_mix(x, perm, lam, boxes, shift, dshift=dshift)
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (kind, len(bad), bad[:5].tolist())
        if kind == "full":
            assert np.array_equal(_bits(got), _bits(x[perm]))


def test_mix_batch_strided_grid_on_a_large_sample():
    """2 x 4 x 512 x 516: more float4s per sample than the capped grid has threads, so the stride loop runs a second trip"""
    shape = (2, 4, 512, 516)
    x = np.random.default_rng(1).normal(0, 1, shape).astype(np.float32)
    boxes = np.array([[100, 129, 400, 515], [0, 0, 0, 0]], np.int32)
    lam = np.array([1.0, 0.3], np.float32)
    got = _gpu_mix(x, [1, 0], lam, boxes, runs=1)
    assert np.array_equal(_bits(got), _bits(R.mix_batch_ref(x, [1, 0], lam, boxes)))
    outside = np.ones(shape[2:], bool)
    outside[100:400, 129:515] = False
    assert np.array_equal(_bits(got[0][:, outside]), _bits(x[0][:, outside]))          # CutMix: outside the box the sample itself


def test_mix_batch_bad_arguments_and_the_python_wrapper():
    from mi355.lib import lib
    from utils.mix import mix_batch
    x = torch.randn(2, 1, 4, 4, device=DEV)
    i, f = torch.zeros(8, dtype=torch.int32, device=DEV), torch.ones(2, device=DEV)
    for args in ((None, i, f, i, torch.empty_like(x), 2, 1, 4, 4), (x, i, f, i, x, 2, 1, 4, 4), (x, i, f, i, torch.empty_like(x), 0, 1, 4, 4),
                 (x, None, f, i, torch.empty_like(x), 2, 1, 4, 4), (x, i, f, i, x.view(-1)[4:], 2, 1, 4, 4)):
        with pytest.raises(RuntimeError, match="mix_batch"):
            lib.mi355_mix_batch_f32(*args)
    ok = ([1, 0], [0.3, 1.0], [[0, 0, 0, 0], [1, 1, 3, 4]])
    got = mix_batch(x, *ok)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(R.mix_batch_ref(x.cpu().numpy(), *ok)))
    for perm, lam, boxes in (([2, 0], ok[1], ok[2]), ([-1, 0], ok[1], ok[2]), (ok[0], ok[1], [[0, 0, 5, 4], [0, 0, 0, 0]]),
                             (ok[0], ok[1], [[2, 0, 1, 4], [0, 0, 0, 0]]), (ok[0], [0.3], ok[2]), (ok[0], [0.3, float("nan")], ok[2])):
        with pytest.raises(ValueError, match="mix"):
            mix_batch(x, perm, lam, boxes)
    for bad in (x.double(), x[:, :, :, ::2], x.cpu(), x[0]):
        with pytest.raises(ValueError, match="mix"):
            mix_batch(bad, *ok)


# ---- mi355_ce_mix ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ce_inputs(B, C):
    rng = np.random.default_rng(100 * B + C)
    z = rng.normal(0, 3, (B, C)).astype(np.float32)
    z[0, 0], z[B - 1, C - 1] = 30.0, -30.0
    if B > 1:
        z[1, 1], z[1, 2] = -30.0, 30.0
    ya, yb = rng.integers(0, C, B), rng.integers(0, C, B)
    lam = rng.random(B).astype(np.float32)
    lam[0] = 1.0
    lam[B // 2] = 0.0
    w = (0.25 + 2 * rng.random(C)).astype(np.float32)
    for a in (z, ya, yb, lam, w):
        a.setflags(write=False)
    return z, ya, yb, lam, w


def _gpu_ce(z, ya, yb, lam, w, sm, gscale, want_dz=True):
    from mi355.lib import lib
    B, C = z.shape
    zs, yas = _src(z), _src(np.asarray(ya, np.int64), torch.int64)
    ybs = None if yb is None else _src(np.asarray(yb, np.int64), torch.int64)
    lams = None if lam is None else _src(lam)
    ws = None if w is None else _src(w)
    gs = None if gscale is None else _src(np.array([gscale], np.float32))
    ptr = lambda g: None if g is None else g.t
    outs = []
    for _ in range(2):
        loss, dz = Guarded(1), Guarded(B * C)
        lib.mi355_ce_mix(zs.t, yas.t, ptr(ybs), ptr(lams), ptr(ws), loss.t, dz.t if want_dz else None, ptr(gs), B, C, float(sm))
        torch.cuda.synchronize()
        assert loss.intact() and dz.intact()
        if not want_dz:
            assert dz.untouched()
        outs.append((loss.numpy(-1).copy(), dz.numpy((B, C)).copy()))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert zs.intact() and np.array_equal(_bits(zs.numpy(z.shape)), _bits(z))
    return float(outs[0][0][0]), outs[0][1].astype(np.float64)


@pytest.mark.parametrize("gscale", [None, 1.0, 1024.0])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,C", [(1, 3), (5, 3), (257, 7)])
def test_ce_mix_is_within_one_float32_rounding_of_the_restatement(B, C, weighted, mixed, gscale):
    """bound: this module's docstring (2^-23 |ref| + 1e-12, loss and every element of dz)"""
    z, ya, yb, lam, w = _ce_inputs(B, C)
    yb, lam = (yb, lam) if mixed else (None, None)
    w = w if weighted else None
    for sm in (0.0, 0.1):
        sm32 = float(np.float32(sm))
        ref_loss, ref_dz = R.ce_mix_ref(z, ya, yb, lam, w, sm32, 1.0 if gscale is None else gscale)
        loss, dz = _gpu_ce(z, ya, yb, lam, w, sm, gscale)
        e_loss, e_dz = abs(loss - ref_loss), np.abs(dz - ref_dz)
        print(f"B={B} C={C} w={weighted} mixed={mixed} gscale={gscale} sm={sm}: loss {loss:.7g} |d| {e_loss:.2e} (bound {R.ce_bound(ref_loss):.2e}), "
              f"dz worst |d| / bound {(e_dz / R.ce_bound(ref_dz)).max():.3f}")
        assert e_loss <= R.ce_bound(ref_loss)
        assert (e_dz <= R.ce_bound(ref_dz)).all(), np.argwhere(e_dz > R.ce_bound(ref_dz))[:5].tolist()
        only, none = _gpu_ce(z, ya, yb, lam, w, sm, gscale, want_dz=False)
        assert np.float32(only).view(np.int32) == np.float32(loss).view(np.int32)


def test_ce_mix_hard_unweighted_is_ce_smooth_and_bad_arguments():
    from mi355.lib import lib
    z, ya, yb, lam, _ = _ce_inputs(5, 3)
    zt, yt = torch.from_numpy(z.copy()).to(DEV), torch.from_numpy(ya.copy()).to(DEV)
    a, b = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
    lib.mi355_ce_smooth(zt, yt, a, None, None, 5, 3, 0.1)
    lib.mi355_ce_mix(zt, yt, None, None, None, b, None, None, 5, 3, 0.1)
    assert abs(float(a) - float(b)) <= 1e-5 * abs(float(b))             # (ce_smooth computes in float32 with fast exp / log)
    lt = torch.from_numpy(lam.copy()).to(DEV)
    for args in ((None, yt, None, None), (zt, None, None, None), (zt, yt, yt, None), (zt, yt, None, lt)):
        with pytest.raises(RuntimeError, match="ce_mix"):
            lib.mi355_ce_mix(*args, None, b, None, None, 5, 3, 0.1)


# ---- MixCrossEntropyLoss on a Net ------------------------------------------------------------------------------------------------
def _resnet18(seed=0):
    from utils.helpers import get_class_model
    torch.manual_seed(seed)
    m, head = get_class_model("resnet18")
    m.compute_dtype = torch.float32
    return m, head


@pytest.mark.parametrize("weighted", [False, True])
def test_mix_cross_entropy_writes_its_gradient_into_the_plans_dout(weighted):
    from mi355 import nn as mnn
    from utils.mix import MixedTarget
    B, C = 4, 3
    m, _ = _resnet18()
    m = m.to(DEV).train()
    x = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    ya, yb, lam = [0, 1, 2, 1], [2, 1, 0, 0], np.array([0.7, 1.0, 0.25, 0.0], np.float32)
    w = np.array([0.5, 2.0, 1.25], np.float32) if weighted else None
    crit = mnn.MixCrossEntropyLoss(label_smoothing=0.1, weight=w)
    out = m(x)
    plan = out._mi355_plan
    z = out.detach().float().cpu().numpy().copy()
    loss = crit(out, MixedTarget(torch.tensor(ya, device=DEV), torch.tensor(yb, device=DEV), torch.from_numpy(lam).to(DEV)))
    loss.backward()
    torch.cuda.synchronize()
    ref_loss, ref_dz = R.ce_mix_ref(z, ya, yb, lam, w, float(np.float32(0.1)))
    got = plan.dout[:B * C].float().cpu().numpy().astype(np.float64).reshape(B, C)
    assert abs(float(loss.detach()) - ref_loss) <= R.ce_bound(ref_loss)
    assert (np.abs(got - ref_dz) <= R.ce_bound(ref_dz)).all(), (got, ref_dz)
    grads = [p.grad for p in m.parameters() if p.requires_grad]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert all(float(g.abs().max()) > 0 for g in grads if g.dim() > 1)
    out2 = m(x)                                                            # (another dropout mask: its own logits)
    ref_hard = R.ce_mix_ref(out2.detach().float().cpu().numpy(), ya, None, None, w, float(np.float32(0.1)))[0]
    hard = crit(out2, torch.tensor(ya, device=DEV))                        # an int64 label tensor: hard labels
    assert abs(float(hard.detach()) - ref_hard) <= R.ce_bound(ref_hard)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        mnn.MixCrossEntropyLoss(check_labels=True)(out.detach(), torch.tensor([0, 1, 2, 3], device=DEV))


# ---- through train() -------------------------------------------------------------------------------------------------------------
def _strip_time(text):
    return re.sub(r"finished in [\d.]+ minutes", "finished", text)


def _cls_loaders():
    from torch.utils.data import DataLoader, TensorDataset
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(12, 3, 64, 64, generator=g), torch.randint(0, 3, (12,), generator=g)
    return (x, y, DataLoader(TensorDataset(x[:8], y[:8]), batch_size=4, shuffle=False),
            DataLoader(TensorDataset(x[8:], y[8:]), batch_size=4, shuffle=False))


def _recording(base):
    class Recording(base):
        """fixes every draw itself and keeps (input batch, input target, draw, output target)"""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.log = []

        def __call__(self, x, y, params=None):
            params = self.draw(x.size(0), x.size(2), x.size(3))
            xm, ym = super().__call__(x, y, params)
            self.log.append((x.cpu().numpy().copy(), y.cpu(), params, ym))
            return xm, ym

    return Recording


def _watch_inputs(model):
    seen = []
    model.register_forward_pre_hook(lambda mod, args: seen.append((mod.training, args[0].detach().cpu().numpy().copy())))
    return seen


def test_train_without_batch_mix_prints_what_it_printed(tmp_path, capsys):
    """MixedBatches(loader, None) against the plain loader, from the same initial state and dropout seed; compared as strictly as two
    runs on the plain loader compare with each other"""
    from utils import helpers
    from utils.mix import MixedBatches
    _, _, tr, va = _cls_loaders()
    texts = []
    for i, loader in enumerate((tr, tr, MixedBatches(tr, None))):
        m, head = _resnet18(seed=5)
        torch.manual_seed(7)
        best = helpers.train(m, loader, va, torch.device(DEV), 2, 1e-4, "resnet18", str(tmp_path / f"r{i}"), seg=False, cls_head_name=head)
        texts.append((_strip_time(capsys.readouterr().out), best))
    print("two runs on the plain loader identical:", texts[0] == texts[1])
    assert len(re.findall(r"Ep\d+: TrainLoss", texts[2][0])) == 2
    if texts[0] == texts[1]:
        assert texts[2] == texts[0]
    else:
        assert len(texts[2][0].splitlines()) == len(texts[0][0].splitlines())


def test_train_mixes_every_training_batch_and_no_validation_batch(tmp_path, capsys):
    from utils import helpers
    from utils.mix import BatchMix, MixedBatches, MixedTarget, kernel_lam
    x, y, tr, va = _cls_loaders()
    m, head = _resnet18(seed=5)
    seen = _watch_inputs(m)
    before = torch.get_rng_state().clone()
    mix = _recording(BatchMix)(mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, seed=11)
    state_after_init = torch.get_rng_state().clone()
    helpers.train(m, MixedBatches(tr, mix), va, torch.device(DEV), 2, 1e-4, "resnet18", str(tmp_path), seg=False, cls_head_name=head)
    text = capsys.readouterr().out
    assert torch.equal(before, state_after_init)
    train_in = [a for t, a in seen if t]
    val_in = [a for t, a in seen if not t]
    assert len(mix.log) == len(train_in) == 4 and len(val_in) == 2
    kinds = set()
    for k, ((xb, yb_, (perm, lam, boxes), ym), got) in enumerate(zip(mix.log, train_in)):
        lo = 4 * (k % 2)
        assert np.array_equal(_bits(xb), _bits(x[lo:lo + 4].numpy())) and torch.equal(yb_, y[lo:lo + 4])       # the loader's batch
        want = R.mix_batch_ref(xb, perm, kernel_lam(lam, boxes), boxes)
        assert np.array_equal(_bits(got), _bits(want)), k
        assert isinstance(ym, MixedTarget) and torch.equal(ym.ya.cpu(), yb_) and torch.equal(ym.yb.cpu(), yb_[torch.from_numpy(perm)])
        assert np.array_equal(ym.lam.cpu().numpy(), lam)
        kinds |= {"cut" if b[2] > b[0] and b[3] > b[1] else "mixup" for b in boxes}
        assert not np.array_equal(_bits(got), _bits(xb))
    assert kinds == {"cut", "mixup"}
    for a in val_in:
        assert np.array_equal(_bits(a), _bits(x[8:].numpy()))
    lines = re.findall(r"Ep\d+: TrainLoss ([\d.naninf]+) \(Acc ([\d.]+)%\) \| ValLoss ([\d.naninf]+) \| ValAcc", text)
    assert len(lines) == 2 and all(np.isfinite(float(v)) for l in lines for v in l)


def test_train_segmentation_with_cutmix_keeps_the_masks_binary(tmp_path, capsys):
    from torch.utils.data import DataLoader, TensorDataset
    from oracle import train as otrain
    from utils import helpers
    from utils.helpers import get_seg_model
    from utils.mix import BatchMix, MixedBatches
    b = [otrain.synthetic_batch(4, 32, seed=s) for s in (0, 1, 2)]
    x, y = torch.cat([v[0] for v in b]), torch.cat([v[1] for v in b])
    tr = DataLoader(TensorDataset(x[:8], y[:8]), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(x[8:], y[8:]), batch_size=4, shuffle=False)
    m = get_seg_model("attentionunet")
    m.compute_dtype = torch.float32
    seen = _watch_inputs(m)
    mix = _recording(BatchMix)(cutmix_alpha=1.0, seed=2, seg=True)
    helpers.train(m, MixedBatches(tr, mix), va, torch.device(DEV), 2, 1e-4, "AttentionUNet", str(tmp_path), seg=True)
    text = capsys.readouterr().out
    train_in = [a for t, a in seen if t]
    assert len(mix.log) == len(train_in) == 4 and sum(not t for t, _ in seen) == 2
    pasted = 0
    for k, ((xb, yb_, (perm, lam, boxes), ym), got) in enumerate(zip(mix.log, train_in)):
        ones = np.ones(4, np.float32)
        assert np.array_equal(_bits(got), _bits(R.mix_batch_ref(xb, perm, ones, boxes))), k
        ymn = ym.cpu().numpy()
        assert ymn.shape == (4, 1, 32, 32) and set(np.unique(ymn)) <= {0.0, 1.0}
        assert np.array_equal(_bits(ymn), _bits(R.mix_batch_ref(yb_.numpy(), perm, ones, boxes)))
        pasted += int(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).sum())
    assert pasted > 0
    for t, a in seen:
        if not t:
            assert np.array_equal(_bits(a), _bits(x[8:].numpy()))
    lines = re.findall(r"Ep\d+: TrainLoss ([\d.naninf]+) \| ValLoss ([\d.naninf]+) \| IoU ([\d.naninf]+)", text)
    assert len(lines) == 2 and all(np.isfinite(float(v)) for l in lines for v in l)
