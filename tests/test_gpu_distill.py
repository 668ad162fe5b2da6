"""-m gpu: the knowledge-distillation losses (csrc/distill.hip: mi355_kd_seg_*, mi355_ce_distill; mi355.nn.SegDistillationLoss /
DistillCrossEntropyLoss; utils/distill.py through helpers.train) on the device, against the fp64 restatement tests/distill_ref.py,
which tests/test_distill_cpu.py pins to torch's fp64 autograd.

Bounds.  Segmentation kernels: those of this loss family in tests/test_gpu_seg_loss.py, |loss_k - ref_k| < 1e-5 max(1, |ref_k|) for the
three outputs [total, hard, KD] and rel_err(dz, ref) < 1e-5 (the difference at the largest magnitude over the reference's largest
magnitude).  mi355_ce_distill computes in double and rounds to float32 once on store: 2^-23 |ref| + 1e-12 for every output, as
tests/test_gpu_mix.py derives it for mi355_ce_mix.

Every call through the ABI writes into buffers pre-filled with a sentinel between guard bands and is checked for intact guards,
unchanged sources and two bit-identical runs (the harness of tests/test_gpu_focal.py)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import distill_ref as R
import mix_ref
import seg_loss_ref
from gpu_util import gpu_kinks, rel_err
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A

# (bce, dice, kd) weights x T {0.5, 1, 2, 4} x smooth {1, 1e-3}, thinned: every value of every parameter occurs, kd alone, the hard
# terms alone (v = NULL) and mixtures
#        bw    dw    kw    T    smooth
GRID = [(0.5, 0.5, 0.5, 2.0, 1.0),
        (0.0, 0.0, 1.0, 0.5, 1.0),
        (1.0, 0.0, 0.0, 1.0, 1.0),
        (0.0, 1.0, 0.25, 4.0, 1e-3),
        (0.3, 0.7, 0.7, 1.0, 1.0),
        (1.0, 0.0, 1.0, 2.0, 1e-3),
        (0.25, 0.25, 0.5, 0.5, 1.0),
        (0.0, 1.0, 0.0, 4.0, 1.0),
        (2.0, 0.5, 0.1, 4.0, 1.0)]


def _f32(cfg):
    """the parameters as the kernels receive them (float arguments)"""
    return tuple(float(np.float32(v)) for v in cfg)


class Guarded:
    """``count`` float32 elements filled with sentinel bytes between two guard bands; ``shift``: the view starts that many bytes off a
    16-byte boundary"""

    def __init__(self, count, shift=0):
        self.nbytes = count * 4
        self.whole = torch.full((self.nbytes + 2 * GUARD + shift,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + shift
        self.whole[self.lo:self.lo + self.nbytes] = SENTINEL
        self.t = self.whole[self.lo:self.lo + self.nbytes].view(torch.float32)
        assert self.t.data_ptr() % 16 == shift % 16

    def intact(self):
        return bool((self.whole[:self.lo] == GUARD_BYTE).all()) and bool((self.whole[self.lo + self.nbytes:] == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.t.view(torch.uint8) == SENTINEL).all())


def _src(t, shift=0):
    g = Guarded(t.numel(), shift)
    g.t.copy_(t.reshape(-1))
    return g


def op(z, t, v, cfg, ps, gscale=None, shift=0, runs=2, sentinel_v=False):
    """The C ABI as a caller sees it -> (loss tensor [3], dz tensor of z's shape), both on the host.  z, t, v: host tensors; v None:
    a NULL pointer; ``sentinel_v``: v is a sentinel-filled buffer instead, which must come back untouched (kd_weight 0)."""
    from mi355.lib import lib
    bw, dw, kw, T, sm = cfg
    B, per = z.shape[0], z.numel() // z.shape[0]
    rows = lib.mi355_kd_seg_rows(B, per)
    assert rows >= B and rows % B == 0
    zs, ts = _src(z, shift), _src(t, shift)
    vs = Guarded(z.numel(), shift) if sentinel_v else (None if v is None else _src(v, shift))
    vt = None if vs is None else vs.t
    gs = None if gscale is None else torch.full((1,), gscale, device=DEV)
    outs = []
    for _ in range(runs):
        partial, state, loss, dz = Guarded(rows * 8), Guarded(2 * B), Guarded(3), Guarded(z.numel(), shift)
        lib.mi355_kd_seg_fwd(zs.t, ts.t, vt, B, per, bw, dw, sm, 1 if ps else 0, kw, T, partial.t, state.t, loss.t)
        torch.cuda.synchronize()
        assert dz.untouched() and dz.intact()
        lib.mi355_kd_seg_bwd(zs.t, ts.t, vt, B, per, bw, kw, T, state.t, gs, dz.t)
        torch.cuda.synchronize()
        assert partial.intact() and state.intact() and loss.intact() and dz.intact()
        outs.append((loss.t.cpu().clone(), dz.t.cpu().clone().view(z.shape)))
    for l, d in outs[1:]:
        assert torch.equal(l, outs[0][0]) and torch.equal(d, outs[0][1])
    assert zs.intact() and ts.intact() and torch.equal(zs.t.cpu(), z.reshape(-1)) and torch.equal(ts.t.cpu(), t.reshape(-1))
    if sentinel_v:
        assert vs.intact() and vs.untouched()
    elif vs is not None:
        assert vs.intact() and torch.equal(vs.t.cpu(), v.reshape(-1))
    return outs[0]


def ref(z, t, v, cfg, ps, gscale=None):
    bw, dw, kw, T, sm = cfg
    return R.kd_seg(z.numpy(), t.numpy(), None if v is None else v.numpy(), bw, dw, sm, ps, kw, T, 1.0 if gscale is None else gscale)


def check_loss(tag, loss, l64):
    l = loss.double().numpy()
    print(f"{tag}: loss {l.tolist()} ref {[float(f'{x:.8f}') for x in l64]} |d| {[float(f'{abs(a - b):.2e}') for a, b in zip(l, l64)]}")
    assert np.isfinite(l).all(), tag
    for k in range(3):
        assert abs(l[k] - l64[k]) < 1e-5 * max(1.0, abs(l64[k])), (tag, k, l[k], l64[k])


def check(tag, loss, dz, l64, g64):
    check_loss(tag, loss, l64)
    e = rel_err(dz.reshape(-1), torch.from_numpy(np.ascontiguousarray(g64)).reshape(-1))
    print(f"{tag}: dz rel_err {e:.2e}")
    assert bool(torch.isfinite(dz).all()), tag
    assert e < 1e-5, (tag, e)


@functools.lru_cache(maxsize=None)
def _data(shape, seed=11):
    g = torch.Generator().manual_seed(seed + sum(shape))
    z = (torch.randn(*shape, generator=g) * 2.0).float()
    t = (torch.rand(*shape, generator=g) < 0.35).float()
    v = (torch.randn(*shape, generator=g) * 2.0 + 0.5 * z).float()
    return z, t, v


SHAPES = [((3, 1, 17, 13), 0), ((1, 1, 64, 64), 0), ((2, 1, 96, 172), 0), ((2, 1, 96, 172), 4)]


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("shape,shift", SHAPES)
def test_parity_with_the_fp64_restatement(shape, shift, ps):
    """(3,1,17,13): per odd, scalar path, one workgroup per sample; (1,1,64,64): one exact four-vector trip; (2,1,96,172): per % 4 = 0,
    four workgroups per sample, some threads in the one-vector loop; the same at a 4-byte offset: the scalar path with per % 4 = 0"""
    from mi355.lib import lib
    z, t, v = _data(shape)
    B, per = shape[0], z.numel() // shape[0]
    assert lib.mi355_kd_seg_rows(B, per) // B == {221: 1, 4096: 1, 16512: 4}[per]
    for i, cfg in enumerate(GRID):
        cfg = _f32(cfg)
        vv = v if cfg[2] > 0 else None                                   # kd_weight 0: a NULL pointer
        for gscale in (None, 3.0, 65536.0) if i == 0 else ((None, 3.0, 65536.0)[i % 3],):          # all three at the first, then rotating
            check(f"abi {shape}+{shift} ps={ps} {cfg} gscale={gscale}", *op(z, t, vv, cfg, ps, gscale, shift), *ref(z, t, vv, cfg, ps, gscale))


def module(z, t, v, crit):
    from utils.distill import DistillTarget
    zz = z.to(DEV).requires_grad_(True)
    loss = crit(zz, t.to(DEV) if v is None else DistillTarget(t.to(DEV), v.to(DEV)))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), zz.grad.cpu()


@pytest.mark.parametrize("ps", [False, True])
def test_parity_at_the_flagship_shape_and_the_module_is_the_abi(ps):
    from mi355 import nn as mnn
    shape = (32, 1, 256, 256)
    z, t, v = _data(shape)
    bw, dw, k, T, sm = 0.5, 0.5, 0.5, 2.0, 1.0
    cfg = _f32(((1.0 - k) * bw, (1.0 - k) * dw, k, T, sm))               # what the module hands the ABI
    loss, dz = op(z, t, v, cfg, ps)
    check(f"abi {shape} ps={ps} {cfg}", loss, dz, *ref(z, t, v, cfg, ps))
    crit = mnn.SegDistillationLoss(bw, dw, sm, ps, kd_weight=k, temperature=T)
    lm, dm = module(z, t, v, crit)
    terms = crit.last_terms.cpu().clone()
    lm2, dm2 = module(z, t, v, crit)
    assert torch.equal(lm, lm2) and torch.equal(dm, dm2)
    assert torch.equal(terms, loss) and torch.equal(lm.reshape(1), loss[:1]) and torch.equal(dm, dz)          # bit for bit
    assert crit.last_terms.is_cuda and crit.last_terms.shape == (3,) and not crit.last_terms.requires_grad


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("shape,shift", SHAPES)
def test_identities(shape, shift, ps):
    """v == z: KD is exactly 0, loss[0] and dz have the bits of the same call with kd_weight 0 and v NULL; with kd_weight 0 a
    sentinel-filled v is never touched and the result agrees with mi355_seg_loss_fwd / _bwd within the family's bounds"""
    from mi355.lib import lib
    z, t, _ = _data(shape)
    B, per = shape[0], z.numel() // shape[0]
    for bw, dw, kw, T, sm in GRID:
        cfg = _f32((bw, dw, kw if kw > 0 else 0.5, T, sm))
        same = op(z, t, z.clone(), cfg, ps, 3.0, shift)
        cfg0 = cfg[:2] + (0.0,) + cfg[3:]
        none = op(z, t, None, cfg0, ps, 3.0, shift)
        assert float(same[0][2]) == 0.0 and float(none[0][2]) == 0.0
        assert torch.equal(same[0][:2], none[0][:2]) and torch.equal(same[0][0], same[0][1])
        assert torch.equal(same[1], none[1]), (cfg, float((same[1] - none[1]).abs().max()))
        sent = op(z, t, None, cfg0, ps, 3.0, shift, runs=1, sentinel_v=True)
        assert torch.equal(sent[0], none[0]) and torch.equal(sent[1], none[1])
    # against the Dice loss's own launches
    cfg0 = _f32((0.5, 0.5, 0.0, 2.0, 1.0))
    l, d = op(z, t, None, cfg0, ps, None, shift, runs=1)
    zs, ts = _src(z, shift), _src(t, shift)
    rows = lib.mi355_seg_loss_rows(B, per)
    buf, dz = torch.empty(rows * 4 + 2 * B + 1, device=DEV), Guarded(z.numel(), shift)
    lib.mi355_seg_loss_fwd(zs.t, ts.t, B, per, 0.5, 0.5, 1.0, 1 if ps else 0, buf[:rows * 4], buf[rows * 4:rows * 4 + 2 * B], buf[rows * 4 + 2 * B:])
    lib.mi355_seg_loss_bwd(zs.t, ts.t, B, per, 0.5, buf[rows * 4:rows * 4 + 2 * B], None, dz.t)
    torch.cuda.synchronize()
    ls = float(buf[-1])
    e = rel_err(d.reshape(-1), dz.t.cpu())
    print(f"kd_weight 0 vs mi355_seg_loss {shape}+{shift} ps={ps}: |dloss| {abs(float(l[0]) - ls):.2e}, dz rel_err {e:.2e}")
    assert abs(float(l[0]) - ls) < 1e-5 * max(1.0, abs(ls)) and abs(float(l[1]) - ls) < 1e-5 * max(1.0, abs(ls)) and e < 1e-5


def test_plain_tensor_targets_take_the_undistilled_launches():
    """the validation loop: SegDistillationLoss on a mask = CombinedLoss, DistillCrossEntropyLoss on labels = MixCrossEntropyLoss, bit
    for bit and unscaled by 1 - kd_weight"""
    from mi355 import nn as mnn
    z, t, _ = _data((2, 1, 96, 172))
    for ps in (False, True):
        a = module(z, t, None, mnn.SegDistillationLoss(0.3, 0.7, 1e-3, ps, kd_weight=0.9, temperature=3.0))
        b = module(z, t, None, mnn.CombinedLoss(0.3, 0.7, 1e-3, ps))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    zc, y, _, w = _ce_inputs(257, 3)
    for weight in (None, w):
        a = module(torch.from_numpy(zc), torch.from_numpy(y), None, mnn.DistillCrossEntropyLoss(0.9, 3.0, 0.1, weight))
        b = module(torch.from_numpy(zc), torch.from_numpy(y), None, mnn.MixCrossEntropyLoss(0.1, weight))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


SAT_GRID = [(0.5, 0.5, 0.5, 2.0, 1.0), (0.0, 0.0, 1.0, 0.5, 1.0), (1.0, 0.0, 0.5, 1.0, 1.0), (0.0, 1.0, 0.5, 4.0, 1.0), (0.0, 1.0, 0.0, 2.0, 1.0)]


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("shape", [(4, 1, 32, 32), (3, 1, 17, 13)])
def test_saturated_logits_and_constant_targets_stay_finite_and_right(shape, ps):
    """|z|, |v| in {30, 100}: the teacher on the student's side everywhere (agreeing) and on the other side everywhere (opposing), the
    student on its target's side; all-zero and all-one targets on random logits.  Everything is finite and the three losses are within
    the bound everywhere; the gradient is compared wherever bce_weight > 0 or kd_weight > 0 — the Dice term alone on saturated logits
    has an fp64 gradient below float32's range (p (1 - p) = 1e-13 .. 1e-44 times a coefficient), as in tests/test_gpu_focal.py."""
    g = torch.Generator().manual_seed(3)
    t = (torch.rand(*shape, generator=g) < 0.5).float()
    z0, v0 = torch.randn(*shape, generator=g) * 2, torch.randn(*shape, generator=g) * 2
    side = torch.where(t > 0, 1.0, -1.0)
    cases = {"all-zero target": (z0, torch.zeros(shape), v0), "all-one target": (z0, torch.ones(shape), v0)}
    for zm in (30.0, 100.0):
        for vm in (30.0, 100.0):
            cases[f"z +-{zm:g}, v +-{vm:g} agreeing"] = (side * zm, t, side * vm)
            cases[f"z +-{zm:g}, v +-{vm:g} opposing"] = (side * zm, t, -side * vm)
    for tag, (z, t_, v) in cases.items():
        for cfg in SAT_GRID:
            cfg = _f32(cfg)
            vv = v if cfg[2] > 0 else None
            l64, g64 = ref(z, t_, vv, cfg, ps)
            loss, dz = op(z, t_, vv, cfg, ps, runs=1)
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all()), (tag, cfg)
            check_loss(f"{tag} {shape} ps={ps} {cfg}", loss, l64)
            if cfg[0] > 0 or cfg[2] > 0 or "target" in tag:
                check(f"{tag} {shape} ps={ps} {cfg}", loss, dz, l64, g64)


def test_module_surface(tmp_path):
    from torch.utils.data import DataLoader, TensorDataset
    from mi355 import amp as mamp, nn as mnn
    from utils import helpers
    from utils.distill import Distilled, DistillTarget
    from utils.mix import BatchMix, MixedBatches
    z = torch.randn(2, 17, 13, device=DEV)
    t = (torch.rand(2, 17, 13, device=DEV) < 0.5).float()
    v = torch.randn(2, 17, 13, device=DEV)
    crit = mnn.SegDistillationLoss()
    with pytest.raises(ValueError, match="teacher logits .* must match the student's output"):
        crit(z, DistillTarget(t, v[:, :16]))
    with pytest.raises(ValueError, match="must match input size"):
        crit(z[:, None], DistillTarget(t[:, :16], v[:, None]))
    with pytest.raises(ValueError, match="teacher logits .* must match the student's output"):
        mnn.DistillCrossEntropyLoss()(torch.randn(4, 3, device=DEV), DistillTarget(torch.zeros(4, dtype=torch.int64, device=DEV), torch.randn(4, 2, device=DEV)))
    with pytest.raises(ValueError, match="mixed target"):
        from utils.mix import MixedTarget
        y = torch.zeros(4, dtype=torch.int64, device=DEV)
        mnn.DistillCrossEntropyLoss()(torch.randn(4, 3, device=DEV), MixedTarget(y, y, torch.ones(4, device=DEV)))
    l3, g3 = module(z.cpu(), t.cpu(), v.cpu(), crit)
    l4, g4 = module(z.cpu()[:, None], t.cpu()[:, None], v.cpu()[:, None], crit)          # [N, H, W] and [N, 1, H, W]: the same memory
    assert torch.equal(l3, l4) and torch.equal(g3.reshape(-1), g4.reshape(-1)) and g3.shape == z.shape
    # the upstream gradient and the loss scale enter as one factor
    a = z.clone().requires_grad_(True)
    sc = mamp.GradScaler()
    assert sc.get_scale() == 65536.0
    sc.scale(crit(a, DistillTarget(t, v))).backward()
    torch.cuda.synchronize()
    assert rel_err(a.grad.cpu(), g3 * 65536.0) < 1e-6
    zc = torch.randn(5, 3, device=DEV)
    yc, vc = torch.tensor([0, 1, 2, 1, 0], device=DEV), torch.randn(5, 3, device=DEV)
    ce = mnn.DistillCrossEntropyLoss(label_smoothing=0.1)
    b = zc.clone().requires_grad_(True)
    ce(b, DistillTarget(yc, vc)).backward()
    c = zc.clone().requires_grad_(True)
    sc.scale(ce(c, DistillTarget(yc, vc))).backward()
    torch.cuda.synchronize()
    assert rel_err(c.grad.cpu(), b.grad.cpu() * 65536.0) < 1e-6

    # train(): what a Distilled loader cannot be combined with
    x, y = torch.randn(4, 3, 32, 32), torch.randint(0, 3, (4,))
    dl = DataLoader(TensorDataset(x, y), batch_size=4)
    teacher = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 32 * 32, 3)).to(DEV)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 32 * 32, 3))
    with pytest.raises(TypeError, match="DistillTarget, which CrossEntropyLoss cannot take.*DistillCrossEntropyLoss"):
        helpers.train(model, Distilled(dl, teacher), dl, DEV, 1, 1e-3, "x", str(tmp_path), criterion=mnn.CrossEntropyLoss())
    with pytest.raises(TypeError, match="DistillTarget, which CombinedLoss cannot take.*SegDistillationLoss"):
        helpers.train(model, Distilled(dl, teacher), dl, DEV, 1, 1e-3, "x", str(tmp_path), seg=True, criterion=mnn.CombinedLoss())
    with pytest.raises(ValueError, match="MixedTarget.*not built"):
        helpers.train(model, Distilled(MixedBatches(dl, BatchMix(mixup_alpha=0.2)), teacher), dl, DEV, 1, 1e-3, "x", str(tmp_path))
    assert not os.listdir(str(tmp_path))


# ---- mi355_ce_distill ----------------------------------------------------------------------------------------------------------------
def ce_bound(ref):
    """tests/mix_ref.py::ce_bound: one float32 rounding of a value computed in double"""
    return 2.0 ** -23 * np.abs(ref) + 1e-12


@functools.lru_cache(maxsize=None)
def _ce_inputs(B, C):
    rng = np.random.default_rng(100 * B + C)
    z = rng.normal(0, 3, (B, C)).astype(np.float32)
    v = (0.5 * z + rng.normal(0, 3, (B, C))).astype(np.float32)
    y = rng.integers(0, C, B)
    z[0] = rng.normal(0, 1, C)
    z[0, 0] += 60.0                                      # one logit 60 above the rest in z: the true class of row 0 ...
    y[0] = 0
    if B > 1:
        v[B - 1] = rng.normal(0, 1, C)
        v[B - 1, C - 1] += 60.0                          # ... and one in v, on the last row
    else:
        v[0, C - 1] += 60.0
    w = (0.25 + 2 * rng.random(C)).astype(np.float32)
    return z, y, v, w


def _gpu_ce_distill(z, y, v, w, s, hw, kw, T, gscale, want_dz=True, sentinel_v=False):
    from mi355.lib import lib
    B, C = z.shape
    zs = _src(torch.from_numpy(z.copy()))
    vs = Guarded(B * C) if sentinel_v else (None if v is None else _src(torch.from_numpy(v.copy())))
    yt = torch.from_numpy(np.asarray(y, np.int64).copy()).to(DEV)
    ws = None if w is None else _src(torch.from_numpy(w.copy()))
    gs = None if gscale is None else torch.full((1,), gscale, device=DEV)
    outs = []
    for _ in range(2):
        loss, dz = Guarded(3), Guarded(B * C)
        lib.mi355_ce_distill(zs.t, yt, None if vs is None else vs.t, None if ws is None else ws.t, loss.t, dz.t if want_dz else None, gs, B, C,
                             float(s), float(hw), float(kw), float(T))
        torch.cuda.synchronize()
        assert loss.intact() and dz.intact() and (want_dz or dz.untouched())
        outs.append((loss.t.cpu().clone(), dz.t.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert zs.intact() and torch.equal(zs.t.cpu().view(B, C), torch.from_numpy(z)) and (ws is None or ws.intact())
    if sentinel_v:
        assert vs.intact() and vs.untouched()
    elif vs is not None:
        assert vs.intact() and torch.equal(vs.t.cpu().view(B, C), torch.from_numpy(v))
    return outs[0][0], outs[0][1].double().numpy().reshape(B, C)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_ce_distill_is_within_one_float32_rounding_of_the_restatement(B, C, weighted):
    from mi355.lib import lib
    z, y, v, w = _ce_inputs(B, C)
    w = w if weighted else None
    f = lambda x: float(np.float32(x))
    for T, s, hw, kw, gscale in ((1.0, 0.0, f(0.5), f(0.5), None), (4.0, f(0.1), f(0.25), f(0.75), 1024.0), (4.0, 0.0, 0.0, 1.0, None),
                                 (1.0, f(0.1), 1.0, 0.0, 3.0)):
        vv = v if kw > 0 else None
        l64, g64 = R.ce_distill(z, y, vv, w, s, hw, kw, T, 1.0 if gscale is None else gscale)
        loss, dz = _gpu_ce_distill(z, y, vv, w, s, hw, kw, T, gscale)
        e_loss, e_dz = np.abs(loss.double().numpy() - np.array(l64)), np.abs(dz - g64)
        print(f"B={B} C={C} w={weighted} T={T} s={s} hw={hw} kw={kw} gscale={gscale}: loss {loss.tolist()} |d| / bound "
              f"{(e_loss / ce_bound(np.array(l64))).max():.3f}, dz worst |d| / bound {(e_dz / ce_bound(g64)).max():.3f}")
        assert (e_loss <= ce_bound(np.array(l64))).all(), (loss.tolist(), l64)
        assert (e_dz <= ce_bound(g64)).all(), np.argwhere(e_dz > ce_bound(g64))[:5].tolist()
        only, _ = _gpu_ce_distill(z, y, vv, w, s, hw, kw, T, gscale, want_dz=False)          # dz = NULL: the loss alone, the same bits
        assert torch.equal(only, loss)
        if kw == 0:                                      # = hard_weight x mi355_ce_mix on hard labels; v is never read
            sent, dsent = _gpu_ce_distill(z, y, None, w, s, hw, kw, T, gscale, sentinel_v=True)
            assert torch.equal(sent, loss) and np.array_equal(dsent, dz) and float(loss[2]) == 0.0
            zt, yt = torch.from_numpy(z.copy()).to(DEV), torch.from_numpy(np.asarray(y, np.int64).copy()).to(DEV)
            wt = None if w is None else torch.from_numpy(w.copy()).to(DEV)
            lm, dm = torch.empty(1, device=DEV), torch.empty(B * C, device=DEV)
            lib.mi355_ce_mix(zt, yt, None, None, wt, lm, dm, torch.full((1,), gscale, device=DEV), B, C, s)
            torch.cuda.synchronize()
            rl, rd = mix_ref.ce_mix_ref(z, y, None, None, w, s, gscale)
            assert abs(float(lm.double()) - float(loss[1].double())) <= ce_bound(rl) and abs(float(lm.double()) - float(loss[0].double())) <= ce_bound(rl)
            assert (np.abs(dm.cpu().double().numpy().reshape(B, C) - dz) <= ce_bound(rd)).all()
    same, _ = _gpu_ce_distill(z, y, z.copy(), w, 0.1, 0.5, 0.5, 4.0, None)                   # v == z
    assert float(same[2]) == 0.0 and float(same[1]) > 0


def test_ce_distill_module_is_the_abi():
    from mi355 import nn as mnn
    from utils.distill import DistillTarget
    z, y, v, w = _ce_inputs(257, 3)
    k, T, s = 0.25, 4.0, 0.1
    crit = mnn.DistillCrossEntropyLoss(k, T, s, w)
    a = torch.from_numpy(z.copy()).to(DEV).requires_grad_(True)
    l = crit(a, DistillTarget(torch.from_numpy(y.copy()).to(DEV), torch.from_numpy(v.copy()).to(DEV)))
    (3 * l).backward()
    torch.cuda.synchronize()
    lo, do = _gpu_ce_distill(z, y, v, w, s, 1.0 - k, k, T, 3.0)
    assert torch.equal(crit.last_terms.cpu(), lo) and torch.equal(l.detach().cpu().reshape(1), lo[:1])
    assert np.array_equal(a.grad.cpu().double().numpy(), do)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        mnn.DistillCrossEntropyLoss(check_labels=True)(a.detach(), DistillTarget(torch.full((257,), 3, device=DEV), torch.from_numpy(v.copy()).to(DEV)))


# ---- whole model ---------------------------------------------------------------------------------------------------------------------
KD_MODEL = dict(bce_weight=0.5, dice_weight=0.5, kd_weight=0.5, temperature=2.0)


def _kd_model_ref(z, t, v):
    """what SegDistillationLoss(**KD_MODEL) computes: the hard weights times 1 - kd_weight"""
    k = KD_MODEL["kd_weight"]
    return R.kd_seg(z, t, v, (1 - k) * KD_MODEL["bce_weight"], (1 - k) * KD_MODEL["dice_weight"], 1.0, False, k, KD_MODEL["temperature"])


def test_whole_model_gradients_match_fp64_oracle_on_the_same_masks():
    """tests/test_gpu_focal.py's statement and bounds for AttentionUNet 64 x 64 in fp32, under SegDistillationLoss(0.5, 0.5,
    kd_weight=0.5, temperature=2) with a fixed synthetic teacher-logit tensor: logits 1e-4, loss 1e-5, plan.dout 1e-3, parameter
    gradients median <= 5e-5, max <= 1e-3, >= 97 % of the tensors <= 3e-4 of their maximum.  The gradients are right only if
    dloss/dlogits really landed in the plan's dout buffer."""
    from mi355 import nn as mnn
    from utils.distill import DistillTarget
    from utils.helpers import get_seg_model
    name = "AttentionUNet"
    sd = nets.closed_form_state(name)
    m = get_seg_model("attentionunet")
    m.load_state_dict(sd)
    m.compute_dtype = torch.float32
    m = m.to(DEV).train()
    x, y = otrain.closed_form_input(2, 64)
    v = (torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(5)) * 2.0).float()
    out = m(x.to(DEV))
    plan = out._mi355_plan
    crit = mnn.SegDistillationLoss(**KD_MODEL)
    loss = crit(out, DistillTarget(y.to(DEV), v.to(DEV)))          # ([N, H, W] logits next to [N, 1, H, W] targets: the same map)
    loss.backward()
    torch.cuda.synchronize()
    relu, pool = gpu_kinks(plan)
    assert len(pool) == 4
    n = out.numel()
    zg = out.detach().float().cpu().numpy()
    lg, dzg = _kd_model_ref(zg, y.numpy().reshape(zg.shape), v.numpy().reshape(zg.shape))
    check("plan.dout on the GPU's logits", crit.last_terms.cpu(), plan.dout[:n].cpu().view(zg.shape), lg, dzg)
    # the fp64 oracle replayed on the GPU's ReLU / max-pool decisions
    s64 = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in sd.items()}
    pk = nets.param_keys(s64)
    for k in pk:
        s64[k].requires_grad_(True)
    nets.Kinks.start("replay", relu, pool)
    try:
        o64 = nets.NETS[name](s64, x.double(), True)
        if o64.dim() == 3:
            o64 = o64.unsqueeze(1)
        l64, dz64 = _kd_model_ref(o64.detach().numpy(), y.double().numpy().reshape(o64.shape), v.double().numpy().reshape(o64.shape))
        o64.backward(torch.from_numpy(dz64))
    finally:
        _, _, used = nets.Kinks.stop()
    assert used == (len(relu), len(pool)), (used, len(relu), len(pool))
    o64 = o64.detach()
    g64 = {k: s64[k].grad for k in pk if s64[k].grad is not None}
    e_dout = rel_err(plan.dout[:n].cpu(), torch.from_numpy(dz64).reshape(-1))
    e_out = float((out.detach().cpu().double().reshape(o64.shape) - o64).abs().max() / o64.abs().max())
    print(f"SegDistillationLoss AttentionUNet 64: logits {e_out:.2e}, loss |d| {abs(float(loss.detach()) - l64[0]):.2e}, plan.dout {e_dout:.2e}")
    assert e_dout < 1e-3
    assert e_out < 1e-4
    assert abs(float(loss.detach()) - l64[0]) < 1e-5
    gmax = max(float(t.abs().max()) for t in g64.values())
    errs = {}
    for k, p in m.named_parameters():
        r = g64[k]
        sc = float(r.abs().max())
        if sc < 1e-6 * gmax:
            assert float(p.grad.abs().max()) <= 1e-5 * gmax, k          # conv bias in front of a train-mode BN: exactly zero
            continue
        errs[k] = float((p.grad.cpu().double() - r).abs().max()) / sc
    e = np.array(list(errs.values()))
    worst = max(errs, key=errs.get)
    print(f"  parameter gradients: median {np.median(e):.2e}, max {e.max():.2e} ({worst}), {100 * np.mean(e <= 3e-4):.1f} % <= 3e-4")
    assert np.median(e) <= 5e-5, np.median(e)
    assert e.max() <= 1e-3, (worst, errs[worst])
    assert np.mean(e <= 3e-4) >= 0.97, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


# ---- train() -------------------------------------------------------------------------------------------------------------------------
LOG = r"Ep(\d+): TrainLoss ([\d.]+) \| ValLoss ([\d.]+) \| IoU ([\d.]+)"
KD_LOG = r"Ep(\d+): Distill hard ([\d.]+) \| KD ([\d.]+)"


def test_train_with_a_distilled_loader_follows_the_cpu_protocol(tmp_path, capsys):
    """helpers.train(Distilled(loader, teacher), criterion=SegDistillationLoss(0.5, 0.5, kd_weight=0.5, temperature=2)) on the fixed
    synthetic loader of tests/test_gpu_focal.py: the teacher an AttentionUNet on closed_form_state in fp32, frozen, in eval mode, the
    student an AttentionUNet from the same state.  The CPU fp64 loop is built from oracle.nets, oracle.train.AdamW / clip_grad_norm /
    cosine_lr and tests/distill_ref.py, the teacher's logits from the fp64 oracle in eval mode; bounds as there: both sides three-decimal
    numbers as the log prints them, training loss 2e-3, validation loss (the hard loss alone) 2e-3 (relative above 1), IoU 5e-3, best
    validation loss 2e-3 relative; the Distill line carries the CPU loop's two means within 2e-3.  The teacher's state_dict is
    bit-identical afterwards and its mode restored."""
    from torch.utils.data import DataLoader, TensorDataset
    from mi355 import nn as mnn
    from models.segmentation_models.AttentionUNet import AttentionUNet
    from utils import helpers
    from utils.distill import Distilled
    name = "AttentionUNet"
    zf = np.load(os.path.join(G, "train_traj_AttentionUNet.npz"))
    hw, epochs, lr = int(zf["hw"]), int(zf["epochs"]), float(zf["lr"])
    b = [otrain.synthetic_batch(4, hw, seed=s) for s in (0, 1, 2)]
    tr = DataLoader(TensorDataset(torch.cat([b[0][0], b[1][0]]), torch.cat([b[0][1], b[1][1]])), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(b[2][0], b[2][1]), batch_size=4, shuffle=False)
    teacher = AttentionUNet()
    teacher.load_state_dict(nets.closed_form_state(name))
    teacher.compute_dtype = torch.float32
    teacher = teacher.to(DEV).eval()
    for p in teacher.parameters():
        p.requires_grad = False
    before = {k: t.detach().clone() for k, t in teacher.state_dict().items()}
    m = AttentionUNet()
    m.load_state_dict(nets.closed_form_state(name))
    m.compute_dtype = torch.float32
    best = helpers.train(m.to(DEV), Distilled(tr, teacher), va, torch.device(DEV), epochs, lr, name, str(tmp_path), seg=True,
                         criterion=mnn.SegDistillationLoss(**KD_MODEL))
    text = capsys.readouterr().out
    rows, kd_rows = re.findall(LOG, text), re.findall(KD_LOG, text)
    assert len(rows) == epochs and len(kd_rows) == epochs
    assert os.path.exists(os.path.join(str(tmp_path), f"{name}_best_loss.pt"))
    after = teacher.state_dict()
    assert not teacher.training and list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    teacher.train()
    helpers.train(m, Distilled(tr, teacher), va, torch.device(DEV), 1, lr, name, str(tmp_path), seg=True)      # criterion=None: SegDistillationLoss(1, 0)
    assert teacher.training and len(re.findall(KD_LOG, capsys.readouterr().out)) == 1                         # the mode it came with

    sd0 = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in nets.closed_form_state(name).items()}
    sd = {k: t.clone() for k, t in sd0.items()}
    fn = nets.NETS[name]
    pk = nets.param_keys(sd)
    opt = otrain.AdamW(pk, lr)
    b = [(x.double(), y.double()) for x, y in b]
    train_b, val_b = b[:2], b[2:]
    with torch.no_grad():
        teach = [fn(sd0, x, False).reshape(y.shape).numpy() for x, y in train_b]
    n_train, n_val = sum(x.shape[0] for x, _ in train_b), sum(x.shape[0] for x, _ in val_b)
    hist, ref_best = [], float("inf")
    for ep in range(1, epochs + 1):
        run = run_h = run_k = 0.0
        for (x, y), v in zip(train_b, teach):
            for k in pk:
                sd[k].requires_grad_(True)
                sd[k].grad = None
            out = fn(sd, x, True)
            if out.dim() == 3:
                out = out.unsqueeze(1)
            l, dz = _kd_model_ref(out.detach().numpy(), y.numpy(), v)
            out.backward(torch.from_numpy(dz).to(out.dtype))
            grads = {k: sd[k].grad.detach().clone() for k in pk if sd[k].grad is not None}
            for k in pk:
                sd[k].requires_grad_(False)
                sd[k].grad = None
            otrain.clip_grad_norm(list(grads.values()), 1.0)
            with torch.no_grad():
                opt.step(sd, grads)
            run, run_h, run_k = run + l[0] * x.shape[0], run_h + l[1] * x.shape[0], run_k + l[2] * x.shape[0]
        vl = vm = 0.0
        with torch.no_grad():
            for x, y in val_b:
                out = fn(sd, x, False)
                vl += seg_loss_ref.seg_loss(out.numpy().reshape(y.shape), y.numpy(), 0.5, 0.5)[0] * x.shape[0]      # the hard loss alone, unscaled
                vm += otrain.iou_train(torch.sigmoid(out).reshape(y.shape), y)
        vl /= n_val
        hist.append((run / n_train, vl, vm / len(val_b), run_h / n_train, run_k / n_train))
        opt.lr = otrain.cosine_lr(lr, ep, epochs)
        ref_best = min(ref_best, vl)
    for row, kd_row, want in zip(rows, kd_rows, hist):
        got = [float(t) for t in row] + [float(t) for t in kd_row[1:]]
        want = tuple(float(f"{t:.3f}") for t in want)            # what the CPU loop's own log lines would print
        print(f"Ep{int(got[0])}: GPU train {got[1]:.3f} val {got[2]:.3f} IoU {got[3]:.3f} hard {got[4]:.3f} KD {got[5]:.3f} | CPU {want}")
        assert abs(got[1] - want[0]) <= 2e-3 + 1e-9 and abs(got[2] - want[1]) <= 2e-3 * max(1, want[1]) + 1e-9 and \
            abs(got[3] - want[2]) <= 5e-3 + 1e-9, (got, want)
        assert abs(got[4] - want[3]) <= 2e-3 + 1e-9 and abs(got[5] - want[4]) <= 2e-3 + 1e-9, (got, want)
    assert abs(best - ref_best) < 2e-3 * ref_best


def test_train_one_classifier_epoch_with_a_teacher(tmp_path, capsys):
    """One epoch of helpers.train on ResNet18 (a plain Linear head: no dropout draw to match), 8 synthetic 64 x 64 samples in two
    batches, stage 1 (the head alone, AdamW(1e-4)), distilled from a ResNet18 on closed_form_state in eval mode under
    DistillCrossEntropyLoss(0.5, 4, label_smoothing=0.1).  The CPU loop is the same protocol in fp64 from oracle.nets / oracle.train and
    tests/distill_ref.py; the printed training loss is within 2e-3 of it, and so are the two terms of the Distill line."""
    from torch.utils.data import DataLoader, TensorDataset
    from mi355 import nn as mnn
    from models.classification_models.ResNet import ResNet18
    from utils import helpers
    from utils.distill import Distilled
    name = "ResNet18"
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(12, 3, 64, 64, generator=gen), torch.randint(0, 3, (12,), generator=gen)
    tr = DataLoader(TensorDataset(x[:8], y[:8]), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(x[8:], y[8:]), batch_size=4, shuffle=False)
    state = nets.closed_form_state(name)
    teacher = ResNet18(num_classes=3)
    teacher.load_state_dict(state)
    teacher.compute_dtype = torch.float32
    teacher = teacher.to(DEV).eval()
    before = {k: t.detach().clone() for k, t in teacher.state_dict().items()}
    m = ResNet18(num_classes=3)
    m.load_state_dict(state)
    m.compute_dtype = torch.float32
    helpers.train(m, Distilled(tr, teacher), va, torch.device(DEV), 1, 1e-4, name, str(tmp_path), seg=False, cls_head_name="fc",
                  criterion=mnn.DistillCrossEntropyLoss(0.5, 4.0, label_smoothing=0.1))
    text = capsys.readouterr().out
    rows = re.findall(r"Ep1: TrainLoss ([\d.]+) \(Acc ([\d.]+)%\) \| ValLoss ([\d.]+) \|", text)
    kd_rows = re.findall(KD_LOG, text)
    assert len(rows) == 1 and len(kd_rows) == 1
    got_train, got_acc, got_val = float(rows[0][0]), float(rows[0][1]), float(rows[0][2])
    after = teacher.state_dict()
    assert not teacher.training and all(torch.equal(after[k], before[k]) for k in before)

    sd0 = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in state.items()}
    sd = {k: t.clone() for k, t in sd0.items()}
    head = ["fc.weight", "fc.bias"]
    opt = otrain.AdamW(head, 1e-4)
    run = run_h = run_k = hits = 0.0
    for lo in (0, 4):
        xb, yb = x[lo:lo + 4].double(), y[lo:lo + 4]
        with torch.no_grad():
            v = nets.NETS[name](sd0, xb, False).numpy()
        for k in head:
            sd[k].requires_grad_(True)
            sd[k].grad = None
        out = nets.NETS[name](sd, xb, True)
        l, dz = R.ce_distill(out.detach().numpy(), yb.numpy(), v, None, float(np.float32(0.1)), 0.5, 0.5, 4.0)
        hits += float((out.detach().argmax(1) == yb).sum())
        out.backward(torch.from_numpy(dz))
        grads = {k: sd[k].grad.detach().clone() for k in head}
        for k in head:
            sd[k].requires_grad_(False)
            sd[k].grad = None
        otrain.clip_grad_norm(list(grads.values()), 1.0)
        with torch.no_grad():
            opt.step(sd, grads)
        run, run_h, run_k = run + l[0] * 4, run_h + l[1] * 4, run_k + l[2] * 4
    print(f"GPU train {got_train:.3f} (acc {got_acc:.2f}) val {got_val:.3f} hard {kd_rows[0][1]} KD {kd_rows[0][2]} | "
          f"CPU train {run / 8:.4f} hard {run_h / 8:.4f} KD {run_k / 8:.4f} acc {100 * hits / 8:.2f}")
    assert abs(got_train - float(f"{run / 8:.3f}")) <= 2e-3 + 1e-9, (got_train, run / 8)
    assert abs(float(kd_rows[0][1]) - float(f"{run_h / 8:.3f}")) <= 2e-3 + 1e-9 and abs(float(kd_rows[0][2]) - float(f"{run_k / 8:.3f}")) <= 2e-3 + 1e-9
    assert np.isfinite(got_val)
